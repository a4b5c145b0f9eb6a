"""Stacked tremor density maps of a step-5 run on the GPU: every window's location posterior, one unit of mass per window,
summed on a map grid -- where the tremor is, and with time bins how it moves (kernels in
hypotremormcmc_amd/csrc/htm_density.hpp).

    python -m hypotremormcmc_amd.density <parameter file> --cell DX [DY DZ] [--bounds x0 x1 y0 y1 z0 z1] [--time-bins N]
                                         [--removed] [--volume] [--level 0.68 0.95]

run in the directory of the step-5 outputs, writes `tremor_density.xy.dat`, `.xz.dat`, `.yz.dat` (and `.vol.dat` with
--volume): one line per cell with the layer (time bin), the cell's indices and centre, the number of samples in it, the
expected number of windows there (count / n_mod) and the smallest --level whose highest-density region of the layer holds the
cell (0: none).  Without --bounds the box is the stations' bounding box widened by prior_width_xy on every side and
prior_z .. prior_z + 5 prior_width_z in depth.  --time-bins N splits the window ids into N equal spans, one layer each;
--removed counts only the windows that hypo.stat.removed keeps.  The share of every layer's samples outside the box is
printed: widen the box when it is large.  The samples go to the device in batches of rows under HTM_DENSITY_MB MiB (default
1024); the result does not depend on it.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import _lib
from .grid import MAX_CELLS, add_grid_arguments, centres, default_bounds, grid9, grid_counts, grid_from_args, make_grid  # noqa: F401
from .run_files import Step5Run
from .statistics import INT_MAX, as_printed, hypo_rows, quantiles, remove_double_counts, sample_matrix

LDS_MAX_CELLS = 8192      # nx ny + nx nz + ny nz of a grid the LDS path takes: kDensLdsCells (tests/test_density.py keeps them equal)
MAPS = ("xy", "xz", "yz", "vol")
# the axes of a map, fastest first
AXES = {"xy": (0, 1), "xz": (0, 2), "yz": (1, 2), "vol": (0, 1, 2)}


def lds_fits(grid) -> bool:
    """whether the LDS path takes the grid"""
    nx, ny, nz = grid_counts(grid)
    return nx * ny + nx * nz + ny * nz <= LDS_MAX_CELLS


def density(hypo, grid, layer=None, n_layer: int = 1, volume: bool = False, device: int = 0):
    """hypo [n_mod][3 n_win] (window w in columns 3w .. 3w+2; NaN and inf count as outside), grid = x0, dx, nx, y0, dy, ny, z0,
    dz, nz, layer [n_win] ints or None, on the GPU.  Returns a dict of uint64 arrays: xy [n_layer][ny][nx], xz
    [n_layer][nz][nx], yz [n_layer][nz][ny], vol [n_layer][nz][ny][nx] (None without `volume`), tally [n_layer][2] =
    inside, outside."""
    x, n_mod = sample_matrix(hypo, "htm_hypo_density takes", n_seq=None, name="hypo", layout="[n_mod][columns]", finite=False)
    n_col = x.shape[1]
    if n_mod < 1 or n_col < 3 or n_col % 3:
        raise ValueError(f"hypo is {x.shape}: need at least one row and x, y, z of every window")
    n_win = n_col // 3
    g = grid9(grid)
    nx, ny, nz = grid_counts(g)
    n_layer = int(n_layer)
    if n_layer < 1:
        raise ValueError(f"n_layer = {n_layer}: need at least 1")
    lay = None
    if layer is None:
        if n_layer != 1:
            raise ValueError(f"n_layer = {n_layer} without a layer per window")
    else:
        lay = np.ascontiguousarray(layer, dtype=np.int32)
        if lay.shape != (n_win,):
            raise ValueError(f"layer is {lay.shape}: need one per window ({n_win})")
    cells = nx * ny + nx * nz + ny * nz + (nx * ny * nz if volume else 0)
    if n_layer * cells > INT_MAX:
        raise ValueError(f"{n_layer} layers of {cells} cells: more than 2^31 - 1 counters")
    out = {"xy": np.empty((n_layer, ny, nx), dtype=np.uint64), "xz": np.empty((n_layer, nz, nx), dtype=np.uint64),
           "yz": np.empty((n_layer, nz, ny), dtype=np.uint64), "vol": np.empty((n_layer, nz, ny, nx), dtype=np.uint64) if volume else None,
           "tally": np.empty((n_layer, 2), dtype=np.uint64)}
    u = lambda a: None if a is None else a.ctypes.data_as(_lib.u64p)
    _lib.check(_lib.load().htm_hypo_density(device, _lib.ptr(x), n_mod, n_win, None if lay is None else lay.ctypes.data_as(_lib.ip),
                                            n_layer, _lib.ptr(g), u(out["xy"]), u(out["xz"]), u(out["yz"]), u(out["vol"]), u(out["tally"])))
    return out


# ---- host helpers, on map-sized data -----------------------------------------------------------------------------------
def hpd_levels(counts, levels):
    """per cell of one layer's map the smallest of `levels` whose highest-density region holds the cell, 0 where none does.
    The region of a level is the smallest set of cells, taken in descending count, whose mass reaches that share of the
    map's sum (the layer's `inside`); cells of equal count enter together, so the region is unique.  Empty cells are in no
    region."""
    c = np.asarray(counts)
    levels = sorted(float(v) for v in levels)
    if any(not 0.0 < v <= 1.0 for v in levels):
        raise ValueError(f"levels {levels}: need 0 < level <= 1")
    out = np.zeros(c.shape)
    total = int(c.sum(dtype=np.uint64))
    if total == 0 or not levels:
        return out
    vals, inv, mult = np.unique(c.reshape(-1), return_inverse=True, return_counts=True)
    order = np.argsort(vals)[::-1]                                    # the distinct counts, descending
    mass = [int(vals[k]) * int(mult[k]) for k in order]
    before = np.concatenate([[0], np.cumsum(np.array(mass, dtype=object))[:-1]])          # mass of the groups that entered earlier
    lev_of = np.zeros(len(vals))
    for rank, k in enumerate(order):
        if vals[k] == 0:
            continue
        # the group enters the region of every level that the earlier groups did not reach
        for v in levels:
            if int(before[rank]) < v * total:
                lev_of[k] = v
                break
    return lev_of[inv.reshape(-1)].reshape(c.shape)


def time_layers(win_id, n_bins: int):
    """[min id, max id] in n_bins equal spans: the layer of every window (int32), exact in integers"""
    w = np.asarray(win_id, dtype=np.int64)
    n_bins = int(n_bins)
    if n_bins < 1 or w.ndim != 1 or not len(w):
        raise ValueError(f"need n_bins >= 1 and at least one window id (got {n_bins}, {w.shape})")
    lo, span = int(w.min()), int(w.max()) - int(w.min()) + 1
    return ((w - lo) * n_bins // span).astype(np.int32)


def removed_layer(layer, keep):
    """`layer` with -1 (takes no part) for every window that is not in `keep` (indices, as remove_double_counts returns them)"""
    lay = np.full(len(layer), -1, dtype=np.int32)
    keep = np.asarray(list(keep), dtype=np.int64)
    lay[keep] = np.asarray(layer, dtype=np.int32)[keep]
    return lay


def kept_windows(win_id, hypo, device: int = 0):
    """the windows that hypo.stat.removed keeps: statistics' medians and intervals, rounded as hypo.stat prints them"""
    return remove_double_counts([int(w) for w in win_id], as_printed(hypo_rows(quantiles(hypo, None, device))))


HEADERS = {nm: "# layer, cell " + " ".join("i" + "xyz"[a] for a in AXES[nm]) + ", centre " + " ".join("xyz"[a] for a in AXES[nm])
               + ", samples, expected windows (samples / n_mod), smallest level whose region holds the cell (0: none)" for nm in MAPS}


def map_text(name, counts, grid, n_mod, levels) -> str:
    """the text of tremor_density.<name>.dat from counts [n_layer][...] of map `name` (slowest axis first, as `density`
    returns it)"""
    g = grid9(grid)
    c = np.asarray(counts)
    axes = AXES[name]
    cen = [centres(g, a) for a in axes]
    lines = [HEADERS[name]]
    for L in range(c.shape[0]):
        lev = hpd_levels(c[L], levels)
        for idx in np.ndindex(*c.shape[1:]):
            cell = idx[::-1]                                         # fastest axis first
            centre = [v[i] for v, i in zip(cen, cell)]
            n = int(c[L][idx])
            lines.append("%5d" % L + "".join("%6d" % i for i in cell) + "".join("%14.6f" % v for v in centre)
                         + "%12d%14.6f%8.4f" % (n, n / float(n_mod), lev[idx]))
    return "\n".join(lines) + "\n"


def summary_text(tally) -> str:
    lines = []
    for L, (n_in, n_out) in enumerate(np.asarray(tally).tolist()):
        tot = n_in + n_out
        share = "NaN" if tot == 0 else "%.2f %%" % (100.0 * n_out / tot)
        lines.append(f"layer {L}: {n_in} samples inside the box, {n_out} outside ({share})")
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m hypotremormcmc_amd.density", description=__doc__.split("\n\n")[0])
    ap.add_argument("parameter_file")
    add_grid_arguments(ap)
    ap.add_argument("--time-bins", type=int, default=1, help="layers of equal spans of window ids")
    ap.add_argument("--removed", action="store_true", help="only the windows that hypo.stat.removed keeps")
    ap.add_argument("--volume", action="store_true", help="also the 3-D counts")
    ap.add_argument("--level", type=float, nargs="+", default=[0.68, 0.95], help="shares of a layer's mass for the regions")
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if any(not 0.0 < v <= 1.0 for v in args.level):
        ap.error("--level must lie in (0, 1]")
    if args.time_bins < 1:
        ap.error("--time-bins must be at least 1")
    run = Step5Run.open(args.parameter_file)
    grid = grid_from_args(ap, args, run.par)
    hypo = run.samples(("hypo",))[1]["hypo"]
    layer = time_layers(run.win_id, args.time_bins)
    if args.removed:
        layer = removed_layer(layer, kept_windows(run.win_id, hypo, run.device))
    res = density(hypo, grid, layer=layer, n_layer=args.time_bins, volume=args.volume, device=run.device)
    for nm in MAPS:
        if res[nm] is not None:
            with open(os.path.join(run.work, "tremor_density.%s.dat" % nm), "w") as fh:
                fh.write(map_text(nm, res[nm], grid, len(hypo), args.level))
    sys.stdout.write(summary_text(res["tally"]))


if __name__ == "__main__":
    main()
