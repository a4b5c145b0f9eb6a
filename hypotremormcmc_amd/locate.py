"""Locate windows on a grid under a FIXED structure on the GPU: with vs, qs and the station corrections fixed (a calibration
run's medians), a window's location posterior is a function of its position alone and is tabulated at the cell centres of a
grid -- no MCMC, any number of windows (kernels in hypotremormcmc_amd/csrc/htm_locate.hpp).

    python -m hypotremormcmc_amd.locate <parameter file> --cell DX [DY DZ] [--bounds x0 x1 y0 y1 z0 z1] [--structure DIR]
                                        [--windows FILE] [--flat-prior] [--volume-of WIN] [--draws K [--draw-weights]]
                                        [--precision fp64|fp32]
                                        [--stack [--time-bins N] [--stack-volume] [--stack-resolved] [--level 0.68 0.95]]
                                        [--residuals] [--refine F [--refine-radius R]]

run in the data directory (station file, opt_data.NNNNNN.dat).  --structure DIR holds `uniform_structure.stat` and
`station_corrections.stat` of the calibration run (default: the parameter file's directory); --windows FILE lists the window
ids in its first column (default `selected_win.dat`).  Without --bounds the box is grid.default_bounds.  The prior is step
5's: Gaussians of prior_width_xy about the station of largest amplitude in x and y, the depth prior of prior_z and
prior_width_z; --flat-prior turns it off.  use_time / use_amp come from the parameter file.  Writes `hypo_grid.stat` (the
layout of hypo.stat: median, 2.5 % and 97.5 % of every axis, from the marginals) and `hypo_grid.best.dat` (one line per
window: the best cell's centre, its log posterior and log-likelihood term, the log evidence, the posterior mean, and 1 when
the best cell lies on a face of the box: that window is not resolved by this grid).  --volume-of WIN also writes that
window's log posterior of every cell to `hypo_grid.WIN.vol.dat`.  The windows go to the device in batches whose workspace
stays under HTM_LOCATE_MB MiB (default 1024); the result does not depend on it.

A fixed structure leaves the structure's uncertainty out of the intervals of `hypo_grid.stat`.  --draws K marginalises it
(DESIGN.md §3.11): K records, evenly thinned, of the calibration run's sample files `vs.RR.out`, `qs.RR.out`, `t_corr.RR.out`
and `a_corr.RR.out` in --structure DIR (read_structure_draws) stand for its posterior, a cell's term becomes
log((1 / K) sum_k exp(l_k)) over them (locate_marginal, one kernel for all draws), and the results are written next to the
others, in the same layouts: `hypo_grid_marginal.stat`, `hypo_grid_marginal.best.dat`, `hypo_grid_marginal.WIN.vol.dat`.
Without --draws nothing changes.

Whether K was enough is a question per window: the mixture of a window can be carried by one or two draws, and its intervals
are then a fixed structure's again.  --draws K --draw-weights answers it: the log evidence of every window
under every draw (draw_evidence, one kernel for all draws), the normalised weights w_k of the draws per window and their
effective number n_eff = 1 / sum_k w_k^2.  It writes `hypo_grid_marginal.draws.dat` (one line per window: n_eff, n_eff / K, the
largest weight, the stacked record number of the draw that has it, the mixture's log evidence, and 1 when that weight is above
0.5: one draw outweighs all the others together, K was too small for this window) and `hypo_grid_marginal.structure.dat` (one
line per draw: its record number, vs, qs, and its joint weight over all windows -- the windows are independent given the
structure, so the log weights add: which draws of the calibration posterior the located windows prefer), and adds one line to
the summary.  Without --draw-weights nothing is written or printed that was not before.

--precision fp32 evaluates everything that the invocation evaluates with the single-precision forward: the
synthetic travel time and amplitude of a (cell, station) in fp32, the observations, every sum and everything behind a cell's
term in fp64.  File names and layouts are unchanged; the summary gains one line that names the precision.  The default is
fp64, and without the option nothing is written or printed that was not before.  The parameter file's `forward_precision` and
HTM_FORWARD_PRECISION are step 5's and do not switch this program.

--stack also makes the map product of `density` for the located windows: every window's grid posterior,
normalised to one unit of mass, summed per time layer on the device (`stack`, htm_forward_locate_stack), in the same
evaluation that `<stem>.stat` and `<stem>.best.dat` are written from (<stem>: hypo_grid, or hypo_grid_marginal with --draws;
either --precision).  It writes `<stem>.density.xy.dat`, `.xz.dat`, `.yz.dat` and with --stack-volume `.vol.dat`: one line per
cell in the order and formats of tremor_density.*.dat -- layer, indices, centre, the expected number of windows in the cell and
the smallest --level whose highest-density region of the layer holds the cell -- without a sample count, for there are no
samples.  --time-bins N gives the layers (density.time_layers).  --stack-resolved leaves out every window whose best cell lies
on a face of the box (a first evaluation finds them; the summary says how many).  One summary line per layer: windows
stacked, windows without an included cell, and the share of the layer's mass on the faces of the box.  The other options of
this paragraph without --stack are argument errors.

--residuals says how well every window fits where it lies (`residuals`, htm_forward_locate_residuals): per
station the residual that the demeaning leaves (observation minus demeaned synthetic) at the best cell and as a mean over the
window's posterior, and per window the two offsets that the demeaning takes away -- the precision-weighted mean time residual,
an origin-time shift, and the mean amplitude residual, minus the log source amplitude -- with their posterior spread, and chi2.
It writes `hypo_grid.residuals.dat` (one line per window and station), `hypo_grid.fit.dat` (one line per window) and
`hypo_grid.stations.dat` (one line per station over all windows: does the calibration run's correction hold for these
windows?), and one summary line that names the station with the largest mean residual.  Without --stack the one evaluation
serves `hypo_grid.stat` and `hypo_grid.best.dat` too; with --stack it is a second one.  It takes a fixed structure: with
--draws it is an argument error.  Without --residuals nothing is written or printed that was not before.

--refine F gives the resolution of a grid F times as fine where it matters, for a few thousand cells per window (DESIGN.md
§3.16; `refine`, htm_forward_locate_boxes): after the evaluation that the invocation makes anyway, on the same Forward, every
window is evaluated again on a box of its own about that evaluation's best cell -- 2 R + 1 coarse cells per axis (R:
--refine-radius, default 2), snapped to the coarse cells' edges, shifted inwards where it would cross the outer box, in cells
of 1 / F of the coarse size (refine_boxes) -- with the same structure or draws, prior and precision, in one launch per batch.
It writes `<stem>.refined.stat` (hypo.stat's layout, from the fine marginals: the intervals are CONDITIONAL ON THE BOX, and
the header says so) and `<stem>.refined.best.dat` (best.dat's columns on the fine grid, then the box's lower corner, a lower
bound of the coarse posterior's mass inside the box from the coarse marginals (box_mass_bound), 1 when the best fine cell lies
on a face of its box that is no face of the outer box -- the box is too small: raise the radius --, and 1 when it lies on a
face of the outer box), and one more summary line: the box in coarse and in fine cells, the windows with a best cell on an
inner face, and the windows whose mass bound is below 0.99.  A window without an included coarse cell is not refined: NaN.
Why R = 2: on noise-free data with truths at fine cell centres (6 windows x 40 seeds, 10 x 10 x 5 coarse cells, F = 4) R = 1
left 32 of 240 refined best cells off the truth -- in all 32 the best COARSE cell lay two or more cells from the truth; all 32
were flagged on an inner face, and 7 exact windows were flagged too -- and R = 2 none, with no flag.  The products of --stack,
--residuals, --draw-weights and --volume-of remain the coarse grid's.  --refine-radius without --refine is an argument error.
Without --refine nothing is written or printed that was not before.
"""
from __future__ import annotations

import argparse
import contextlib
import os
import sys

import numpy as np

from . import _lib
from .density import AXES, MAPS, time_layers
from .forward import Forward
from .grid import add_grid_arguments, centres, grid9, grid_counts, grid_from_args
from .obs_data import ObsData
from .run_files import Step5Run, field
from .statistics import HYPO_HEADER, INT_MAX

DRAWS_HEADER = ("# window ID, effective number of the draws n_eff, n_eff / K, largest weight, record number of the draw that has it, "
                "log evidence of the mixture, 1: that weight is above 0.5 (the intervals are one structure's)")
STRUCTURE_HEADER = "# record number of the draw, vs, qs, joint log weight over all windows relative to the best draw, normalised joint weight"
RESIDUALS_HEADER = ("# window ID, station, 1: the station's data are missing for the window, then per data type in use (time, amplitude): "
                    "residual (observation minus demeaned synthetic) at the best cell, its posterior mean, the best cell's over the standard deviation")
FIT_HEADER = ("# window ID, stations with data, then per data type in use (time, amplitude): offset (weighted mean of synthetic minus observation) "
              "at the best cell, its posterior mean and standard deviation, chi2 at the best cell, its posterior mean; "
              "with amplitudes last: log source amplitude (minus the mean amplitude offset)")
STATIONS_HEADER = ("# station, windows with data, then per data type in use (time, amplitude): precision-weighted mean over those windows of the "
                   "posterior-mean residual, its standard error, its weighted rms, largest |best-cell residual / standard deviation| and its window ID")
FIT_NAMES = tuple(f"{q}_{d}{s}" for d in "ta" for q, s in (("m", "_best"), ("m", "_mean"), ("m", "_sd"), ("chi2", "_best"), ("chi2", "_mean")))
REFINED_STAT_HEADER = ("# refined: every window on a box of its own about its best cell of the coarse grid; the intervals are conditional "
                       "on that box (its lower corner and a bound of the coarse posterior's mass inside it: the .refined.best.dat file)")
REFINED_BEST_TAIL = (" (here: of the window's own box, in fine cells), the box's lower corner x y z, lower bound of the coarse posterior's mass "
                     "inside the box, 1: the best cell lies on a face of its box that is no face of the outer box (the box is too small), "
                     "1: it lies on a face of the outer box")
MASS_BOUND_LOW = 0.99       # the summary counts the windows whose box may hold less than this of the coarse posterior's mass
BEST_HEADER = ("# window ID, best cell's centre x y z, log posterior there, log-likelihood term there, log evidence, "
               "posterior mean x y z, 1: the best cell lies on a face of the box")


def _corrections(t_corr, vs, a_corr, qs, S, draws):
    """K and t_corr, vs, a_corr, qs as the library takes them.  A fixed structure (K = 0): one t_corr and a_corr per station and
    the scalars vs, qs as arrays of one; draws: K of vs and qs, K x S of the corrections"""
    tc, ac = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (t_corr, a_corr))
    if not draws:
        if tc.size != S or ac.size != S:
            raise ValueError(f"t_corr and a_corr have {tc.size} and {ac.size} values: need one per station ({S})")
        return 0, tc, np.array([float(vs)]), ac, np.array([float(qs)])
    v, q = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (vs, qs))
    K = v.size
    if q.size != K or tc.size != K * S or ac.size != K * S:
        raise ValueError(f"{K} draws of vs: need as many of qs (got {q.size}) and one t_corr and a_corr per draw and station "
                         f"({K} x {S}; got {tc.size} and {ac.size} values)")
    return K, tc, v, ac, q


def _has_draws(t_corr, vs):
    """whether a structure is draws of it, a 1-D vs or a 2-D t_corr"""
    return np.ndim(vs) >= 1 or np.ndim(t_corr) == 2


class _Call:
    """One call's inputs as the library takes them, checked, and the outputs every call has: the grid `g` and its counts nx, ny,
    nz (at most 2^31 - 1 cells), the structure K, tc, vs, ac, qs (_corrections), the prior [E][5] or None, loc [E][16], marg
    [E][nx + ny + nz] and vol [E][nz][ny][nx] (None where not asked for)"""

    def __init__(self, fwd, t_corr, vs, a_corr, qs, grid, prior, draws, marginals=True, volume=False):
        self.fwd, E = fwd, fwd.n_events
        self.g = grid9(grid)
        self.nx, self.ny, self.nz = nx, ny, nz = grid_counts(self.g)
        if nx * ny * nz > INT_MAX:
            raise ValueError(f"{nx} x {ny} x {nz} cells: more than 2^31 - 1")
        self.K, self.tc, self.vs, self.ac, self.qs = _corrections(t_corr, vs, a_corr, qs, fwd.n_sta, draws)
        self.prior = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
        if prior is not None and self.prior.shape != (E, 5):
            raise ValueError(f"prior is {self.prior.shape}: need mu_x, mu_y, w_xy, z0, w_z of every event ({E})")
        self.loc = np.empty((E, 16))
        self.marg = np.empty((E, nx + ny + nz)) if marginals else None
        self.vol = np.empty((E, nz, ny, nx)) if volume else None

    def run(self, entry, precision, *outputs, scalars=False, origins=None):
        """the library's `entry` on the Forward: the structure (`scalars`: vs and qs by value and no K, as the entry points of a
        fixed structure take it), the grid, `origins` behind it where the entry point takes a box per event, the prior, then
        `outputs` (float64 arrays or None by their pointers, anything else as it is).  precision: None, the Forward's locate
        precision as it is; "fp32" or "fp64": that one for this call, and the previous setting back after it"""
        p = _lib.ptr
        head = (p(self.tc), float(self.vs[0]), p(self.ac), float(self.qs[0])) if scalars else (self.K, p(self.tc), p(self.vs), p(self.ac), p(self.qs))
        tail = [p(a) if a is None or isinstance(a, np.ndarray) else a for a in outputs]
        if precision is not None:
            before = self.fwd.locate_precision
            self.fwd.set_locate_precision(precision)
        try:
            boxes = [] if origins is None else [p(origins)]
            _lib.check(getattr(_lib.load(), entry)(self.fwd.handle, *head, p(self.g), *boxes, p(self.prior), *tail))
        finally:
            if precision is not None:
                self.fwd.set_locate_precision(before)

    def result(self):
        """the dict of `locate` from the library's arrays"""
        loc, marg, nx, ny = self.loc, self.marg, self.nx, self.ny
        cov = np.empty((loc.shape[0], 3, 3))
        for (i, j), k in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(10, 16)):
            cov[:, i, j] = cov[:, j, i] = loc[:, k]
        return {"index": loc[:, 0].astype(np.int64), "best": loc[:, 1:4].copy(), "lp": loc[:, 4].copy(), "ell": loc[:, 5].copy(),
                "log_evidence": loc[:, 6].copy(), "mean": loc[:, 7:10].copy(), "cov": cov, "loc": loc,
                "marg_x": None if marg is None else marg[:, :nx], "marg_y": None if marg is None else marg[:, nx:nx + ny],
                "marg_z": None if marg is None else marg[:, nx + ny:], "vol": self.vol}


def locate(fwd, t_corr, vs, a_corr, qs, grid, prior=None, marginals=True, volume=False, precision=None):
    """The location posterior of every event of the Forward `fwd` on `grid` = x0, dx, nx, y0, dy, ny, z0, dz, nz under the fixed
    structure t_corr [n_sta], vs, a_corr [n_sta], qs; prior [n_events][5] = mu_x, mu_y, w_xy, z0, w_z or None (flat).  Returns
    a dict: index [E] (int64; the best cell's ix + nx (iy + ny iz), -1: every cell excluded), best [E][3] its centre, lp and
    ell [E] the log posterior and the log-likelihood term there, log_evidence [E], mean [E][3], cov [E][3][3], loc [E][16]
    the library's record, marg_x / marg_y / marg_z [E][n] (None without `marginals`), vol [E][nz][ny][nx] (None without
    `volume`).  precision: None, the Forward's own setting (Forward.set_locate_precision; "fp64" unless it was changed), or
    "fp32" / "fp64" for this call, the previous setting put back after it."""
    c = _Call(fwd, t_corr, vs, a_corr, qs, grid, prior, False, marginals, volume)
    c.run("htm_forward_locate", precision, c.loc, c.marg, c.vol, scalars=True)
    return c.result()


def locate_marginal(fwd, t_corr, vs, a_corr, qs, grid, prior=None, marginals=True, volume=False, precision=None):
    """`locate` with the structure marginalised over K draws of it: t_corr [K][n_sta], vs [K], a_corr [K][n_sta], qs [K].  A
    cell's log-likelihood term is log((1 / K) sum_k exp(l_k)), l_k the term `locate` takes under draw k; one kernel evaluates
    all draws (htm_forward_locate_marginal).  Returns the dict of `locate`; K = 1 gives its very bits, in
    either precision (`precision`: as `locate`'s)."""
    c = _Call(fwd, t_corr, vs, a_corr, qs, grid, prior, True, marginals, volume)
    c.run("htm_forward_locate_marginal", precision, c.loc, c.marg, c.vol)
    return c.result()


def draw_evidence(fwd, t_corr, vs, a_corr, qs, grid, prior=None, precision=None):
    """The inputs of `locate_marginal`, `precision` included.  Returns a dict: log_z [E][K], the log evidence `locate` gives under draw k alone
    (-inf: no cell under that draw); with the normalised weights w_k = exp(log_z_k) / sum exp(log_z): n_eff [E] = 1 / sum_k
    w_k^2, w_max [E], k_max [E] (int64; the lowest index of the largest weight, -1 for a window without a cell, whose n_eff,
    w_max and log_evidence are NaN), log_evidence [E] = log((1 / K) sum_k exp(log_z_k)), `locate_marginal`'s
    (htm_forward_locate_draw_evidence)."""
    c = _Call(fwd, t_corr, vs, a_corr, qs, grid, prior, True, marginals=False)
    log_z, summ = np.empty((fwd.n_events, c.K)), np.empty((fwd.n_events, 4))
    c.run("htm_forward_locate_draw_evidence", precision, log_z, summ)
    return {"log_z": log_z, "n_eff": summ[:, 0].copy(), "w_max": summ[:, 1].copy(), "k_max": summ[:, 2].astype(np.int64),
            "log_evidence": summ[:, 3].copy()}


def stack(fwd, t_corr, vs, a_corr, qs, grid, prior=None, layer=None, n_layer=1, volume=False, precision=None):
    """The stacked density of the windows' posteriors on `grid` (htm_forward_locate_stack): every window of
    layer L = layer[e] in 0 .. n_layer - 1 that has an included cell adds exp(lp - lp_best) / W, one unit of mass, to the
    layer's stack, in event order, on the device; no per-window volume comes back.  The inputs of `locate`, or, with t_corr
    [K][n_sta] and vs [K] (a 2-D t_corr or a 1-D vs), of `locate_marginal`.  layer [E] ints or None (n_layer must be 1: every
    window in layer 0); a window whose layer is outside 0 .. n_layer - 1 takes no part.  Returns the dict of `locate` (its
    very bits; vol None) plus xy [n_layer][ny][nx], xz [n_layer][nz][nx], yz [n_layer][nz][ny], tally [n_layer][2] = windows
    stacked, windows without an included cell, and stack [n_layer][nz][ny][nx] (None without `volume`)."""
    c = _Call(fwd, t_corr, vs, a_corr, qs, grid, prior, _has_draws(t_corr, vs))
    nx, ny, nz, E = c.nx, c.ny, c.nz, fwd.n_events
    n_layer = int(n_layer)
    if n_layer < 1:
        raise ValueError(f"n_layer = {n_layer}: need at least 1")
    lay = None
    if layer is None:
        if n_layer != 1:
            raise ValueError(f"n_layer = {n_layer} without a layer per window")
    else:
        lay = np.ascontiguousarray(layer, dtype=np.int32)
        if lay.shape != (E,):
            raise ValueError(f"layer is {lay.shape}: need one per window ({E})")
    if n_layer * (nx * ny * nz + nx * ny + nx * nz + ny * nz + 2) > INT_MAX:
        raise ValueError(f"{n_layer} layers of {nx} x {ny} x {nz} cells, their maps and tallies: more than 2^31 - 1 values")
    out = {"xy": np.empty((n_layer, ny, nx)), "xz": np.empty((n_layer, nz, nx)), "yz": np.empty((n_layer, nz, ny)),
           "stack": np.empty((n_layer, nz, ny, nx)) if volume else None, "tally": np.empty((n_layer, 2))}
    c.run("htm_forward_locate_stack", precision, None if lay is None else lay.ctypes.data_as(_lib.ip), n_layer, c.loc, c.marg, out["xy"], out["xz"],
          out["yz"], out["stack"], out["tally"])
    return dict(c.result(), **out)


def residuals(fwd, t_corr, vs, a_corr, qs, grid, prior=None, precision=None):
    """The stations' residuals, the source terms and the fit of every window where `locate` puts it
    (htm_forward_locate_residuals): the inputs of `locate`.  Returns the dict of `locate` (its very bits; vol
    None) plus res_t_best, res_t_mean, res_a_best, res_a_mean [E][S] -- station j's residual rho = offset - (synthetic -
    observation) at the best cell and its mean over the window's posterior, per data type -- and fit [E][10] = per data type,
    time first, the offset m at the best cell, its posterior mean and standard deviation, chi2 at the best cell and its
    posterior mean, with a view per column under FIT_NAMES (m_t_best, m_t_mean, m_t_sd, chi2_t_best, chi2_t_mean, m_a_best,
    ...).  A data type that the Forward does not use is NaN, a window without an included cell NaN throughout."""
    c = _Call(fwd, t_corr, vs, a_corr, qs, grid, prior, False)
    res, fit = np.empty((fwd.n_events, fwd.n_sta, 4)), np.empty((fwd.n_events, 10))
    c.run("htm_forward_locate_residuals", precision, c.loc, c.marg, res, fit, scalars=True)
    out = dict(c.result(), res=res, fit=fit, res_t_best=res[:, :, 0], res_t_mean=res[:, :, 1], res_a_best=res[:, :, 2], res_a_mean=res[:, :, 3])
    out.update({nm: fit[:, k] for k, nm in enumerate(FIT_NAMES)})
    return out


def locate_boxes(fwd, t_corr, vs, a_corr, qs, grid, origins, prior=None, marginals=True, volume=False, precision=None):
    """`locate` -- or, with t_corr [K][n_sta] and vs [K] (a 2-D t_corr or a 1-D vs), `locate_marginal` -- with a box of its own
    per event (htm_forward_locate_boxes): origins [E][3], absolute; event e is evaluated on the grid
    origins[e][0], dx, nx, origins[e][1], dy, ny, origins[e][2], dz, nz, the cell sizes and counts `grid`'s, whose own three
    origins are checked and otherwise not read.  One launch serves the batch.  Row e of every result is bit for bit what
    `locate` / `locate_marginal` returns in row e with that event's grid: `index` is the cell within the event's box, `best` and
    `mean` are absolute coordinates.  Returns the dict of `locate` plus origin [E][3]."""
    c = _Call(fwd, t_corr, vs, a_corr, qs, grid, prior, _has_draws(t_corr, vs), marginals, volume)
    org = np.ascontiguousarray(origins, dtype=np.float64)
    if org.shape != (fwd.n_events, 3):
        raise ValueError(f"origins is {org.shape}: need x0, y0, z0 of every event ({fwd.n_events})")
    c.run("htm_forward_locate_boxes", precision, c.loc, c.marg, c.vol, origins=org)
    return dict(c.result(), origin=org)


def _cell_ijk(index, counts):
    """(ix, iy, iz) [E][3] of the linear indices ix + nx (iy + ny iz); a window without a cell (-1) gives cell 0"""
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    idx = np.where(idx < 0, 0, idx)
    nx, ny, _ = counts
    return np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], axis=1)


def refine_boxes(index, grid, factor, radius):
    """The refinement policy, stated once: every window's fine box about its best coarse cell `index` [E] of `grid`.  Per axis a
    with n_a coarse cells of size dv_a from v0_a, b_a the best cell's index on it, R = radius, F = factor: the box is
    w_a = min(2 R + 1, n_a) coarse cells wide and begins at the coarse cell i0_a = clamp(b_a - R, 0, n_a - w_a) -- snapped to
    the coarse cells' edges, and where it would cross the outer box shifted inwards, not cut --, its origin is
    v0_a + i0_a * dv_a (one multiplication, then one addition), its cells are dv_a / F wide and w_a F of them: every window has
    the same fine counts, so one grid and one launch serve a batch.  A window without an included coarse cell (index -1) gets
    i0 = 0 and is marked.  Returns a dict: fine_grid (grid9, the coarse grid's origins in the three slots that
    `locate_boxes` does not read), origins [E][3], i0 [E][3] (int64), widths (w_x, w_y, w_z), none [E] (bool)."""
    g, F, R = grid9(grid), int(factor), int(radius)
    if F != factor or R != radius or F < 1 or R < 0:
        raise ValueError(f"factor {factor}, radius {radius}: need integers, factor >= 1 and radius >= 0")
    n = grid_counts(g)
    none = np.asarray(index, dtype=np.int64).reshape(-1) < 0
    b = _cell_ijk(index, n)
    widths = tuple(min(2 * R + 1, n[a]) for a in range(3))
    i0 = np.stack([np.clip(b[:, a] - R, 0, n[a] - widths[a]) for a in range(3)], axis=1)
    i0[none] = 0
    origins = np.stack([g[3 * a] + i0[:, a].astype(np.float64) * g[3 * a + 1] for a in range(3)], axis=1)
    fine = np.array([v for a in range(3) for v in (g[3 * a], g[3 * a + 1] / F, float(widths[a] * F))])
    return {"fine_grid": fine, "origins": origins, "i0": i0, "widths": widths, "none": none}


def box_mass_bound(marg_x, marg_y, marg_z, i0, widths):
    """[E]: a lower bound of the coarse posterior's mass inside every window's box, from what the coarse pass already returns.
    With m_a the coarse axis marginal's mass in the box's cells i0_a .. i0_a + w_a - 1 on axis a, the mass outside the box is
    at most sum_a (1 - m_a) (a cell outside it is outside on one axis at the least), so the mass inside is at least
    max(0, 1 - sum_a (1 - m_a)).  NaN for a window whose marginals are NaN."""
    i0 = np.asarray(i0, dtype=np.int64).reshape(-1, 3)
    out = np.ones(i0.shape[0])
    for a, m in enumerate((marg_x, marg_y, marg_z)):
        m = np.asarray(m, dtype=np.float64).reshape(i0.shape[0], -1)
        inside = np.array([m[e, i0[e, a]:i0[e, a] + widths[a]].sum() for e in range(i0.shape[0])])
        out -= 1.0 - inside
    return np.where(np.isnan(out), np.nan, np.maximum(out, 0.0))


def box_faces(index, fine_grid, i0, widths, grid):
    """(inner_face, outer_face) [E] of the best fine cells `index` within their boxes: whether the cell lies on a face of its
    box that is not a face of the outer box `grid`, and whether it lies on a face of the outer box (False for index -1)"""
    nf, n = grid_counts(fine_grid), grid_counts(grid)
    i0 = np.asarray(i0, dtype=np.int64).reshape(-1, 3)
    has = np.asarray(index, dtype=np.int64).reshape(-1) >= 0
    f = _cell_ijk(index, nf)
    inner, outer = np.zeros(has.size, dtype=bool), np.zeros(has.size, dtype=bool)
    for a in range(3):
        for on, at_outer in ((f[:, a] == 0, i0[:, a] == 0), (f[:, a] == nf[a] - 1, i0[:, a] + widths[a] == n[a])):
            inner |= has & on & ~at_outer
            outer |= has & on & at_outer
    return inner, outer


def refine(fwd, t_corr, vs, a_corr, qs, grid, factor, radius=2, prior=None, coarse=None, precision=None):
    """Coarse to fine: the evaluation on `grid` (`locate`, or `locate_marginal` for draws as `locate_boxes`
    tells them) unless its result is handed in as `coarse`, then `refine_boxes` about its best cells, then `locate_boxes` on
    those boxes: cells of 1 / factor of the coarse size, 2 radius + 1 coarse cells per axis.  Returns the fine result
    (`locate_boxes`' dict; `index` within the window's box) plus coarse_index [E], i0 [E][3] and widths, fine_grid, mass_bound
    [E] (box_mass_bound; None when `coarse` has no marginals), inner_face [E] -- the best fine cell lies on a face of its box
    that is not a face of the outer box: the box is too small, raise the radius -- and outer_face [E].  A window without an
    included coarse cell comes back as a window without a cell (index -1, NaN): the coarse pass gave nothing to refine about.
    The fine posterior is conditional on the box."""
    if coarse is None:
        coarse = (locate_marginal if _has_draws(t_corr, vs) else locate)(fwd, t_corr, vs, a_corr, qs, grid, prior=prior, precision=precision)
    bx = refine_boxes(coarse["index"], grid, factor, radius)
    res = locate_boxes(fwd, t_corr, vs, a_corr, qs, bx["fine_grid"], bx["origins"], prior=prior, precision=precision)
    none = bx["none"]
    if none.any():
        res["index"] = np.where(none, -1, res["index"])
        for key in ("best", "lp", "ell", "log_evidence", "mean", "cov", "marg_x", "marg_y", "marg_z", "vol"):
            if res.get(key) is not None:
                res[key][none] = np.nan
        if res.get("loc") is not None:
            res["loc"][none, 0], res["loc"][none, 1:] = -1.0, np.nan
    inner, outer = box_faces(res["index"], bx["fine_grid"], bx["i0"], bx["widths"], grid)
    mass = None if coarse.get("marg_x") is None else box_mass_bound(coarse["marg_x"], coarse["marg_y"], coarse["marg_z"], bx["i0"], bx["widths"])
    if mass is not None:
        mass = np.where(none, np.nan, mass)                # (nothing was refined: no box to speak of)
    res.update(coarse_index=np.asarray(coarse["index"], dtype=np.int64).copy(), i0=bx["i0"], widths=bx["widths"], fine_grid=bx["fine_grid"],
               mass_bound=mass, inner_face=inner, outer_face=outer)
    return res


JOBS = {"fixed": 0, "marginal": 1, "draw_evidence": 2}      # HTM_LOCATE_FIXED .. of include/htm_hip.h


def plan(n_sta, n_events, grid, job="fixed", n_draws=0, volume=False, prior=False, n_layer=0, layer=False, precision="fp64", residuals=False,
         boxes=False):
    """The workspace and the batches of a call of that shape under the HTM_LOCATE_MB of the environment, without a Forward and
    without a GPU (htm_forward_locate_plan, which states the formula): job "fixed" (`locate`), "marginal" (`locate_marginal`) or
    "draw_evidence" with n_draws; volume and prior: whether the call has them; n_layer >= 1: `stack`, with a layer per window
    or not; residuals: `residuals` (job "fixed", no volume, no stack), whose dict alone has per_event's rbase, rpart, res and fit;
    boxes: `locate_boxes` (jobs "fixed" and "marginal", no stack, no residuals), whose dict alone has per_event's org.
    Returns a dict: rows, tpl, stride, cells, n_tiles, n_marg, map_cells, n_draws, n_draws_padded; per_event and
    per_call, the elements of every device array by name; per_event_bytes, table_bytes, fixed_bytes; nb_limit [4] and nb, the
    events per batch.  A shape that the call would refuse raises HtmError with the call's message."""
    if job not in JOBS:
        raise ValueError(f"job {job!r}: need one of {sorted(JOBS)}")
    if precision not in ("fp32", "fp64"):
        raise ValueError(f"locate precision {precision!r}: need 'fp32' or 'fp64'")
    rq = _lib.LocateRequest(int(n_sta), int(n_events), JOBS[job], int(n_draws), int(bool(volume)), int(bool(prior)), int(n_layer),
                            int(bool(layer)), int(precision == "fp32"), int(bool(residuals)), int(bool(boxes)))
    g = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)
    if g.size != 9:
        raise ValueError(f"grid has {g.size} values: need x0, dx, nx, y0, dy, ny, z0, dz, nz")
    p = _lib.LocatePlan()
    _lib.check(_lib.load().htm_forward_locate_plan(rq, _lib.ptr(g), p))
    d = {n: int(getattr(p, n)) for n in _lib.LocatePlan.INTS + ("nb",)}
    d.update({n: float(getattr(p, n)) for n in _lib.LocatePlan.BYTES})
    d["per_event"] = {n: int(getattr(p, "len_" + n)) for n in _lib.LocatePlan.PER_EVENT}
    d["per_call"] = {n: int(getattr(p, "len_" + n)) for n in _lib.LocatePlan.PER_CALL}
    if residuals:
        d["per_event"].update({n: int(getattr(p, "len_" + n)) for n in _lib.LocatePlan.RESIDUALS})
    if boxes:
        d["per_event"]["org"] = int(p.len_org)
    d["nb_limit"] = [int(v) for v in p.nb_limit]
    return d


def draw_weights(log_z):
    """log_z [E][K] (or one row) -> the normalised weights of the draws per window, exp(log_z - max) over their sum; NaN for a
    window without a cell (every log_z -inf)"""
    z = np.asarray(log_z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        w = np.exp(z - np.max(z, axis=-1, keepdims=True))
    return w / np.sum(w, axis=-1, keepdims=True)


def joint_draw_weights(log_z):
    """log_z [E][K] -> (log_w [K], w [K]): the windows are independent given the structure, so a draw's joint log weight is
    sum_w log_z[w][k] over the windows that have a cell; log_w is that minus its maximum, w = exp(log_w) normalised.  NaN when
    no window has a cell, or no draw keeps a cell in all of them."""
    z = np.asarray(log_z, dtype=np.float64)
    z = z.reshape(-1, z.shape[-1])
    tot = z[np.max(z, axis=1) > -np.inf].sum(axis=0)
    if not (np.max(z, axis=1) > -np.inf).any() or not np.max(tot) > -np.inf:
        return np.full(z.shape[1], np.nan), np.full(z.shape[1], np.nan)
    log_w = tot - np.max(tot)
    w = np.exp(log_w)
    return log_w, w / w.sum()


def marginal_quantiles(marg, grid, levels=(0.025, 0.5, 0.975), origin=None):
    """marg [E][nx + ny + nz] (or one row): the quantiles of the three axis marginals, [E][3][len(levels)].  On an axis the
    quantile q lies in the first cell k whose cumulative mass c_k reaches q, and linearly inside it:
    v0 + dv (k + (q - c_{k-1}) / m_k).  A marginal of NaN gives NaN.  origin [E][3] (or one row): every event's own v0
    (`locate_boxes`) in the place of the grid's."""
    g = grid9(grid)
    n = grid_counts(g)
    m = np.asarray(marg, dtype=np.float64)
    one = m.ndim == 1
    m = m.reshape(-1, sum(n))
    out = np.full((m.shape[0], 3, len(levels)), np.nan)
    v0 = np.tile(g[0::3], (m.shape[0], 1)) if origin is None else np.asarray(origin, dtype=np.float64).reshape(m.shape[0], 3)
    off = 0
    for a in range(3):
        for e in range(m.shape[0]):
            ma = m[e, off:off + n[a]]
            if np.isnan(ma).any():
                continue
            c = np.cumsum(ma)
            for j, q in enumerate(levels):
                k = min(int(np.searchsorted(c, q, side="left")), n[a] - 1)
                while k > 0 and ma[k] == 0.0:          # (rounding left the last cells' sum below q: the last cell with mass)
                    k -= 1
                before = c[k - 1] if k > 0 else 0.0
                out[e, a, j] = v0[e, a] + g[3 * a + 1] * (k + min((q - before) / ma[k], 1.0))
        off += n[a]
    return out[0] if one else out


def read_structure(directory, station_names):
    """vs, qs, t_corr [n_sta], a_corr [n_sta]: the medians of `uniform_structure.stat` and `station_corrections.stat` in
    `directory` (the first and fourth number of a data line), the stations matched by name with `station_names`"""
    def data_lines(name):
        path = os.path.join(directory, name)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: --structure names the directory of a calibration run's .stat files")
        return path, [ln.split() for ln in open(path) if ln.strip() and not ln.lstrip().startswith("#")]

    path, rows = data_lines("uniform_structure.stat")
    if not rows or len(rows[0]) < 6:
        raise ValueError(f"{path}: no data line of six numbers")
    vs, qs = float(rows[0][0]), float(rows[0][3])
    path, rows = data_lines("station_corrections.stat")
    by_name = {}
    for r in rows:
        if len(r) < 7:
            raise ValueError(f"{path}: a data line is a station name and six numbers, got {' '.join(r)!r}")
        by_name[r[0]] = (float(r[1]), float(r[4]))
    tc, ac = [], []
    for nm in station_names:
        key = str(nm).strip()[:12]                 # (station_corrections.stat keeps 12 characters of a name)
        if key not in by_name:
            raise ValueError(f"station {str(nm).strip()} of the station file is not in {path}")
        tc.append(by_name[key][0])
        ac.append(by_name[key][1])
    return vs, qs, np.array(tc), np.array(ac)


def draw_records(n_rec: int, n_draws: int):
    """the records an even thinning of n_rec to n_draws keeps: floor((i + 0.5) n_rec / n_draws), i = 0 .. n_draws - 1"""
    return [((2 * i + 1) * n_rec) // (2 * n_draws) for i in range(n_draws)]


def read_structure_draws(directory, station_names, n_sta, n_draws, records=False):
    """vs [K], qs [K], t_corr [K][n_sta], a_corr [K][n_sta]: K = n_draws records of the calibration run's sample files
    `vs.RR.out`, `qs.RR.out`, `t_corr.RR.out`, `a_corr.RR.out` in `directory`, the ranks RR = 00, 01, ... as far as `vs.RR.out`
    is there, stacked in rank order (Step5Run.samples: a rank's four files must record the same iterations) and thinned evenly
    (draw_records; no random numbers).  The sample files carry no station names: `station_corrections.stat` of the same
    directory must list the stations of the station file, in its order.  With `records` the numbers of the kept records in the
    stacked sample (draw_records) come fifth."""
    from types import SimpleNamespace

    K = int(n_draws)
    if K < 1:
        raise ValueError(f"{K} draws: need at least one")
    n_procs = 0
    while os.path.exists(os.path.join(directory, "vs.%02d.out" % n_procs)):
        n_procs += 1
    if n_procs == 0:
        raise FileNotFoundError(f"{os.path.join(directory, 'vs.00.out')} is missing: --draws needs the sample files of the calibration run "
                                "in the directory that --structure names")
    path = os.path.join(directory, "station_corrections.stat")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: it is what says which station a column of t_corr.RR.out belongs to")
    listed = [ln.split()[0] for ln in open(path) if ln.strip() and not ln.lstrip().startswith("#")]
    want = [str(nm).strip()[:12] for nm in station_names]              # (station_corrections.stat keeps 12 characters of a name)
    if len(want) != n_sta or listed != want:
        k = next((i for i, (a, b) in enumerate(zip(listed, want)) if a != b), min(len(listed), len(want)))
        raise ValueError(f"{path} lists {len(listed)} stations, the station file {len(want)}; they must be the same, in the same order "
                         f"(the first difference: entry {k + 1}, {listed[k] if k < len(listed) else 'none'!r} against "
                         f"{want[k] if k < len(want) else 'none'!r})")
    run = Step5Run(SimpleNamespace(get_n_procs=lambda: n_procs, n_stations=n_sta), directory, [])
    _, smp = run.samples(["vs", "qs", "t_corr", "a_corr"])
    n_rec = smp["vs"].shape[0]
    if K > n_rec:
        raise ValueError(f"{K} draws asked for, {directory} holds {n_rec} records in {n_procs} rank(s)")
    keep = draw_records(n_rec, K)
    out = (smp["vs"][keep, 0].copy(), smp["qs"][keep, 0].copy(), smp["t_corr"][keep].copy(), smp["a_corr"][keep].copy())
    return out + (keep,) if records else out


def step5_prior(par, obs):
    """[n_events][5] = mu_x, mu_y, w_xy, z0, w_z as step 5 sets the hypocentre priors (the station of largest amplitude)"""
    mu_x, mu_y = obs.make_initial_guess()
    p = np.empty((obs.n_events, 5))
    p[:, 0], p[:, 1] = mu_x, mu_y
    p[:, 2], p[:, 3], p[:, 4] = par.get_prior_width_xy(), par.get_prior_z(), par.get_prior_width_z()
    return p


def stat_text(win_id, quant) -> str:
    """the text of hypo_grid.stat from quant [E][3][3] = 2.5 %, 50 %, 97.5 % of x, y, z: hypo.stat's header and layout (median,
    2.5 %, 97.5 % per axis); NaN is written as NaN in the field's width"""
    lines = [HYPO_HEADER]
    for w, q in zip(win_id, np.asarray(quant, dtype=np.float64)):
        lines.append("%9d" % w + "".join(field(q[a][j], 13) for a in range(3) for j in (1, 0, 2)))
    return "\n".join(lines) + "\n"


def on_face(index, grid):
    """per window whether the best cell lies on a face of the box (False for a window without a cell)"""
    nx, ny, nz = grid_counts(grid)
    idx = np.asarray(index, dtype=np.int64)
    ix, iy, iz = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    return (idx >= 0) & ((ix == 0) | (ix == nx - 1) | (iy == 0) | (iy == ny - 1) | (iz == 0) | (iz == nz - 1))


def best_text(win_id, res, grid) -> str:
    """the text of hypo_grid.best.dat from locate's result"""
    flag = on_face(res["index"], grid)
    lines = [BEST_HEADER]
    for i, w in enumerate(win_id):
        vals = list(res["best"][i]) + [res["lp"][i], res["ell"][i], res["log_evidence"][i]] + list(res["mean"][i])
        lines.append("%9d" % w + "".join(field(v, 15) for v in vals) + "%3d" % int(flag[i]))
    return "\n".join(lines) + "\n"


# ---- the residuals' files (--residuals) --------------------------------------------------------------------------------------
MISSING_STDV = 1.0e-16      # the reference's missing-data rule (cls_forward.f90:76-92): keyed on t_stdv alone


def _types(use):
    """(column of res, column of fit, index of the standard deviations) per data type in use"""
    return [(2 * d, 5 * d, d) for d in range(2) if use[d]]


def residuals_text(win_id, names, res, t_stdv, a_stdv, use=(True, True)) -> str:
    """the text of hypo_grid.residuals.dat from `residuals`' res [E][S][4]: one line per (window, station); a missing station's
    columns, and a window's without a cell, are NaN"""
    sd = (np.asarray(t_stdv, dtype=np.float64), np.asarray(a_stdv, dtype=np.float64))
    lines = [RESIDUALS_HEADER]
    for e, w in enumerate(win_id):
        for j, nm in enumerate(names):
            miss = bool(sd[0][e, j] <= MISSING_STDV)
            line = "%9d %-12s%3d" % (w, str(nm).strip()[:12], int(miss))
            for r, _, d in _types(use):
                best, mean = (np.nan, np.nan) if miss else (res[e, j, r], res[e, j, r + 1])
                line += field(best, 15) + field(mean, 15) + field(np.nan if miss else best / sd[d][e, j], 13, 4)
            lines.append(line)
    return "\n".join(lines) + "\n"


def fit_text(win_id, fit, t_stdv, use=(True, True)) -> str:
    """the text of hypo_grid.fit.dat from `residuals`' fit [E][10]: one line per window"""
    n_data = (np.asarray(t_stdv, dtype=np.float64) > MISSING_STDV).sum(axis=1)
    lines = [FIT_HEADER]
    for e, w in enumerate(win_id):
        line = "%9d%6d" % (w, n_data[e])
        for _, f, _ in _types(use):
            line += "".join(field(fit[e, f + k], 15) for k in range(5))
        if use[1]:
            line += field(-fit[e, 6], 15)
        lines.append(line)
    return "\n".join(lines) + "\n"


def station_statistics(win_id, res, t_stdv, a_stdv, use=(True, True)):
    """per station over the windows that have its data and a cell, from `residuals`' res [E][S][4]: n [S], and per data type d
    (0 time, 1 amplitude; NaN where not in use, or no such window) mean [2][S] the precision-weighted mean of the posterior-mean
    residual, se [2][S] its standard error 1 / sqrt(sum p), rms [2][S] the weighted rms, zmax [2][S] the largest |best-cell
    residual / standard deviation| and zwin [2][S] its window id (-1: none)"""
    res = np.asarray(res, dtype=np.float64)
    E, S = res.shape[:2]
    sd = (np.asarray(t_stdv, dtype=np.float64), np.asarray(a_stdv, dtype=np.float64))
    ok = (sd[0] > MISSING_STDV) & ~np.isnan(res).all(axis=2)
    out = {"n": ok.sum(axis=0), "mean": np.full((2, S), np.nan), "se": np.full((2, S), np.nan), "rms": np.full((2, S), np.nan),
           "zmax": np.full((2, S), np.nan), "zwin": np.full((2, S), -1, dtype=np.int64)}
    ids = np.asarray(win_id, dtype=np.int64)
    for r, _, d in _types(use):
        for j in range(S):
            k = np.nonzero(ok[:, j])[0]
            if k.size == 0:
                continue
            p = 1.0 / sd[d][k, j] ** 2
            out["mean"][d, j] = (p * res[k, j, r + 1]).sum() / p.sum()
            out["se"][d, j] = 1.0 / np.sqrt(p.sum())
            out["rms"][d, j] = np.sqrt((p * res[k, j, r + 1] ** 2).sum() / p.sum())
            z = np.abs(res[k, j, r] / sd[d][k, j])
            out["zmax"][d, j], out["zwin"][d, j] = z.max(), ids[k[int(np.argmax(z))]]
    return out


def stations_text(win_id, names, res, t_stdv, a_stdv, use=(True, True)) -> str:
    """the text of hypo_grid.stations.dat (station_statistics): one line per station"""
    st = station_statistics(win_id, res, t_stdv, a_stdv, use)
    lines = [STATIONS_HEADER]
    for j, nm in enumerate(names):
        line = "%-12s%6d" % (str(nm).strip()[:12], st["n"][j])
        for _, _, d in _types(use):
            line += field(st["mean"][d, j], 15) + field(st["se"][d, j], 15) + field(st["rms"][d, j], 15) + field(st["zmax"][d, j], 13, 4) + "%9d" % st["zwin"][d, j]
        lines.append(line)
    return "\n".join(lines) + "\n"


def stations_summary_text(win_id, names, res, t_stdv, a_stdv, use=(True, True)) -> str:
    """the summary's line about the stations: per data type in use the station with the largest absolute mean residual"""
    st = station_statistics(win_id, res, t_stdv, a_stdv, use)
    parts = []
    for _, _, d in _types(use):
        m = np.abs(st["mean"][d])
        if np.isnan(m).all():
            parts.append(f"{('time', 'amplitude')[d]}: no station has a window with data and a cell")
            continue
        j = int(np.nanargmax(m))
        parts.append(f"{('time', 'amplitude')[d]}: station {str(names[j]).strip()} {st['mean'][d, j]:.6f} ({st['mean'][d, j] / st['se'][d, j]:.2f} standard errors, "
                     f"{int(st['n'][j])} windows)")
    return "largest mean residual of a station over the located windows -- " + "; ".join(parts) + "\n"


def refined_stat_text(win_id, fine) -> str:
    """the text of <stem>.refined.stat from `refine`'s result: hypo.stat's layout from the fine marginals, every window's
    quantiles from its own box's origin, behind a line that says what they are conditional on"""
    marg = np.concatenate([fine["marg_x"], fine["marg_y"], fine["marg_z"]], axis=1)
    return REFINED_STAT_HEADER + "\n" + stat_text(win_id, marginal_quantiles(marg, fine["fine_grid"], origin=fine["origin"]))


def refined_best_text(win_id, fine) -> str:
    """the text of <stem>.refined.best.dat from `refine`'s result: best.dat's columns on the fine grid (its flag: a face of the
    window's own box), then the box's lower corner, mass_bound, inner_face, outer_face"""
    lines = [BEST_HEADER + REFINED_BEST_TAIL]
    for i, w in enumerate(win_id):
        vals = list(fine["best"][i]) + [fine["lp"][i], fine["ell"][i], fine["log_evidence"][i]] + list(fine["mean"][i])
        mass = np.nan if fine["mass_bound"] is None else fine["mass_bound"][i]
        lines.append("%9d" % w + "".join(field(v, 15) for v in vals) + "%3d" % int(fine["inner_face"][i] or fine["outer_face"][i])
                     + "".join(field(v, 15) for v in fine["origin"][i]) + field(mass, 13, 9) + "%3d%3d" % (int(fine["inner_face"][i]), int(fine["outer_face"][i])))
    return "\n".join(lines) + "\n"


def refined_summary_text(fine, factor, radius) -> str:
    """the summary's line about the refinement"""
    nf = grid_counts(fine["fine_grid"])
    mass = fine["mass_bound"]
    low = 0 if mass is None else int((mass < MASS_BOUND_LOW).sum())
    return (f"refined by {factor} about the best cells (radius {radius}): boxes of {' x '.join(str(w) for w in fine['widths'])} coarse cells, "
            f"{' x '.join(str(c) for c in nf)} fine cells; {int(np.sum(fine['inner_face']))} windows with the best fine cell on an inner face of their box "
            f"(the box is too small: raise --refine-radius), {low} whose box is not known to hold {MASS_BOUND_LOW} of the coarse posterior's mass\n")


def volume_text(vol, grid) -> str:
    """the text of hypo_grid.WIN.vol.dat from one window's vol [nz][ny][nx]: linear index, cell centre, log posterior"""
    nx, ny, nz = grid_counts(grid)
    x, y, z = (centres(grid, a) for a in range(3))
    lines = ["# cell ix + nx (iy + ny iz), centre x y z, log posterior (NaN, -inf: excluded)"]
    v = np.asarray(vol).reshape(nz, ny, nx)
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                lines.append("%10d%14.6f%14.6f%14.6f %.17g" % (ix + nx * (iy + ny * iz), x[ix], y[iy], z[iz], v[iz, iy, ix]))
    return "\n".join(lines) + "\n"


def draws_text(win_id, ev, records) -> str:
    """the text of hypo_grid_marginal.draws.dat from draw_evidence's result and the draws' record numbers"""
    K = len(records)
    lines = [DRAWS_HEADER]
    for i, w in enumerate(win_id):
        k = int(ev["k_max"][i])
        lines.append("%9d" % w + field(ev["n_eff"][i], 15) + field(ev["n_eff"][i] / K, 15) + field(ev["w_max"][i], 15, 9)
                     + "%9d" % (records[k] if k >= 0 else -1) + field(ev["log_evidence"][i], 15) + "%3d" % int(ev["w_max"][i] > 0.5))
    return "\n".join(lines) + "\n"


def structure_text(records, vs, qs, log_z) -> str:
    """the text of hypo_grid_marginal.structure.dat: the draws' joint weights over all windows (joint_draw_weights)"""
    log_w, w = joint_draw_weights(log_z)
    lines = [STRUCTURE_HEADER]
    for k, r in enumerate(records):
        lines.append("%9d" % r + field(vs[k], 13) + field(qs[k], 13) + field(log_w[k], 15) + field(w[k], 15, 9))
    return "\n".join(lines) + "\n"


def draws_summary_text(ev, n_draws) -> str:
    """the summary's line about the draws' weights"""
    n_eff = ev["n_eff"][~np.isnan(ev["n_eff"])]
    if n_eff.size == 0:
        return f"the {n_draws} draws' effective number: no window has a cell\n"
    return (f"the {n_draws} draws' effective number per window: median {np.median(n_eff):.2f}, smallest {n_eff.min():.2f}; "
            f"{int((ev['w_max'] > 0.5).sum())} windows where one draw outweighs all the others (w_max > 0.5: their intervals are one structure's)\n")


# ---- the stacked density's files (--stack) ----------------------------------------------------------------------------------
def hpd_levels_mass(mass, levels):
    """`density.hpd_levels` for non-negative floats: per cell of one layer's map the smallest of `levels` whose highest-density
    region holds the cell, 0 where none does.  The region of a level is the smallest set of cells, taken in descending mass,
    whose mass reaches that share of the map's sum; cells of equal mass enter together, so the region is unique.  Empty cells
    are in no region.  On integer-valued input it gives what density.hpd_levels gives."""
    m = np.asarray(mass, dtype=np.float64)
    levels = sorted(float(v) for v in levels)
    if any(not 0.0 < v <= 1.0 for v in levels):
        raise ValueError(f"levels {levels}: need 0 < level <= 1")
    if not np.all(m >= 0.0):
        raise ValueError("masses must be non-negative numbers")
    out = np.zeros(m.shape)
    vals, inv, mult = np.unique(m.reshape(-1), return_inverse=True, return_counts=True)
    order = np.argsort(vals)[::-1]                                    # the distinct masses, descending
    group = vals[order] * mult[order]
    total = float(group.sum())
    if total == 0.0 or not levels:
        return out
    before = np.concatenate([[0.0], np.cumsum(group)[:-1]])           # mass of the groups that entered earlier
    lev_of = np.zeros(len(vals))
    for rank, k in enumerate(order):
        if vals[k] == 0.0:
            continue
        for v in levels:                                             # the group enters the region of every level not yet reached
            if before[rank] < v * total:
                lev_of[k] = v
                break
    return lev_of[inv.reshape(-1)].reshape(m.shape)


STACK_HEADERS = {nm: "# layer, cell " + " ".join("i" + "xyz"[a] for a in AXES[nm]) + ", centre " + " ".join("xyz"[a] for a in AXES[nm])
                     + ", expected windows (the stacked grid posteriors' mass; there are no samples, so no sample count), "
                     "smallest level whose region holds the cell (0: none)" for nm in MAPS}


def stack_map_text(name, mass, grid, levels) -> str:
    """the text of <stem>.density.<name>.dat from mass [n_layer][...] of map `name` ("xy", "xz", "yz", "vol"; slowest axis
    first, as `stack` returns it): tremor_density.<name>.dat's order and formats without the sample count"""
    g = grid9(grid)
    m = np.asarray(mass, dtype=np.float64)
    axes = AXES[name]
    cen = [centres(g, a) for a in axes]
    lines = [STACK_HEADERS[name]]
    for L in range(m.shape[0]):
        lev = hpd_levels_mass(m[L], levels)
        for idx in np.ndindex(*m.shape[1:]):
            cell = idx[::-1]                                         # fastest axis first
            lines.append("%5d" % L + "".join("%6d" % i for i in cell) + "".join("%14.6f" % v[i] for v, i in zip(cen, cell))
                         + "%14.6e%8.4f" % (m[L][idx], lev[idx]))
    return "\n".join(lines) + "\n"


def resolved_layer(layer, index, grid):
    """`layer` with -1 (takes no part) for every window whose best cell `index` lies on a face of the box (on_face): the grid
    does not resolve it"""
    return np.where(on_face(index, grid), -1, np.asarray(layer, dtype=np.int32)).astype(np.int32)


def face_share(stack_vol):
    """per layer of stack [n_layer][nz][ny][nx] the share of its mass in the cells on a face of the box (NaN: an empty layer)"""
    s = np.asarray(stack_vol, dtype=np.float64)
    inner = s[:, 1:-1, 1:-1, 1:-1].sum(axis=(1, 2, 3))
    total = s.sum(axis=(1, 2, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0.0, (total - inner) / total, np.nan)


def stack_summary_text(tally, share, n_unresolved=None) -> str:
    """one line per layer: windows stacked, windows without an included cell, the share of the layer's mass on the faces of the
    box; with --stack-resolved a first line says how many windows were left out"""
    lines = [] if n_unresolved is None else [f"{n_unresolved} windows left out of the stack: their best cell lies on a face of the box"]
    for L, ((n_in, n_none), sh) in enumerate(zip(np.asarray(tally).tolist(), share)):
        on = "NaN" if np.isnan(sh) else "%.2f %%" % (100.0 * sh)
        lines.append(f"layer {L}: {int(n_in)} windows stacked, {int(n_none)} without an included cell, {on} of the mass on the faces of the box")
    return "\n".join(lines) + "\n"


def summary_text(res, grid, n_draws=None, precision="fp64") -> str:
    n = len(res["index"])
    how = "" if n_draws is None else f", the structure marginalised over {n_draws} draws"
    prec = "" if precision == "fp64" else f"forward precision: {precision} (the synthetics in single precision, every sum in fp64)\n"
    return (f"{n} windows located on {' x '.join(str(c) for c in grid_counts(grid))} cells{how}\n"
            f"{int(on_face(res['index'], grid).sum())} with the best cell on a face of the box (not resolved by this grid), "
            f"{int((res['index'] < 0).sum())} without an included cell\n" + prec)


@contextlib.contextmanager
def _forward(r5, args, ids):
    """(obs, fwd, prior): the data of the windows `ids` of the run `r5`, a Forward on them at the invocation's precision, closed
    at the end of the block, and their prior (None: --flat-prior)"""
    par = r5.par
    obs = ObsData(ids, par.n_stations, par.sta_x, par.sta_y, directory=r5.work)
    fwd = Forward(par.n_stations, len(ids), par.sta_x, par.sta_y, par.sta_z, obs, use_amp=par.get_use_amp(), use_time=par.get_use_time(),
                  device=r5.device)
    try:
        fwd.set_locate_precision(args.precision)
        yield obs, fwd, None if args.flat_prior else step5_prior(par, obs)
    finally:
        fwd.close()


def _evaluate(r5, args, ids, grid, evaluate, structure, n_bins):
    """Everything the invocation computes of the windows `ids`, on one Forward; evaluate: `locate` or `locate_marginal`, structure:
    t_corr, vs, a_corr, qs as it takes them.  Returns (res, ev, resid, n_unresolved): the result that .stat and .best.dat are
    written from; draw_evidence's with --draw-weights; with --residuals (`residuals`' result, the windows' t_stdv, a_stdv); with
    --stack-resolved the number of windows left out of the stack; with --refine `refine`'s result about the best cells of `res`,
    the last call on the Forward.  None for what was not asked for."""
    ev = resid = n_unresolved = fine = None
    with _forward(r5, args, ids) as (obs, fwd, prior):
        if args.stack:
            # one evaluation gives the maps and what the .stat and .best.dat files are written from; --stack-resolved needs
            # the best cells before it, from an evaluation of their own
            layer = time_layers(ids, n_bins)
            if args.stack_resolved:
                first = evaluate(fwd, *structure, grid, prior=prior, marginals=False)
                layer = resolved_layer(layer, first["index"], grid)
                n_unresolved = int((layer < 0).sum())
            res = stack(fwd, *structure, grid, prior=prior, layer=layer, n_layer=n_bins, volume=True)
            if args.residuals:          # a second evaluation: the stack's call keeps no residuals
                resid = (residuals(fwd, *structure, grid, prior=prior), obs.t_stdv, obs.a_stdv)
        elif args.residuals:            # the one evaluation serves .stat and .best.dat too
            res = residuals(fwd, *structure, grid, prior=prior)
            resid = (res, obs.t_stdv, obs.a_stdv)
        else:
            res = evaluate(fwd, *structure, grid, prior=prior, volume=False)
        if args.draw_weights:
            ev = draw_evidence(fwd, *structure, grid, prior=prior)
        if args.refine is not None:
            fine = refine(fwd, *structure, grid, args.refine, args.refine_radius, prior=prior, coarse=res)
    return res, ev, resid, n_unresolved, fine


def _volume_of(r5, args, grid, evaluate, structure):
    """the log posterior [nz][ny][nx] of the window --volume-of, from a Forward of that one window"""
    with _forward(r5, args, [args.volume_of]) as (_, fwd, prior):
        return evaluate(fwd, *structure, grid, prior=prior, volume=True)["vol"][0]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m hypotremormcmc_amd.locate", description=__doc__.split("\n\n")[0])
    ap.add_argument("parameter_file")
    add_grid_arguments(ap)
    ap.add_argument("--structure", metavar="DIR", help="directory of uniform_structure.stat and station_corrections.stat")
    ap.add_argument("--windows", metavar="FILE", help="window ids in the first column (default selected_win.dat)")
    ap.add_argument("--flat-prior", action="store_true", help="no prior on the position")
    ap.add_argument("--volume-of", type=int, metavar="WIN", help="also write this window's log posterior of every cell")
    ap.add_argument("--draws", type=int, metavar="K", help="marginalise the structure over K evenly thinned records of the sample files "
                    "in --structure DIR; writes hypo_grid_marginal.*")
    ap.add_argument("--draw-weights", action="store_true", help="with --draws: also write what every draw weighs per window and their "
                    "effective number (hypo_grid_marginal.draws.dat) and the draws' joint weights (hypo_grid_marginal.structure.dat)")
    ap.add_argument("--precision", choices=("fp64", "fp32"), default="fp64", help="fp32: the synthetic travel times and amplitudes in single "
                    "precision, every sum in fp64 (default fp64)")
    ap.add_argument("--stack", action="store_true", help="also stack the windows' posteriors on the device into density maps: writes "
                    "<stem>.density.xy.dat, .xz.dat and .yz.dat")
    ap.add_argument("--time-bins", type=int, metavar="N", help="with --stack: layers of equal spans of window ids (default 1)")
    ap.add_argument("--stack-volume", action="store_true", help="with --stack: also the 3-D stack, <stem>.density.vol.dat")
    ap.add_argument("--stack-resolved", action="store_true", help="with --stack: leave out the windows whose best cell lies on a face of the box "
                    "(a first evaluation finds them)")
    ap.add_argument("--level", type=float, nargs="+", metavar="P", help="with --stack: shares of a layer's mass for the regions (default 0.68 0.95)")
    ap.add_argument("--residuals", action="store_true", help="also write every station's residual per window, the windows' source terms and fit, "
                    "and the stations' mean residuals: hypo_grid.residuals.dat, .fit.dat and .stations.dat (a fixed structure: not with --draws)")
    ap.add_argument("--refine", type=int, metavar="F", help="also evaluate every window on a box of its own about its best cell, in cells of 1 / F "
                    "of the size (F >= 2): writes <stem>.refined.stat and <stem>.refined.best.dat")
    ap.add_argument("--refine-radius", type=int, metavar="R", help="with --refine: the box reaches R cells to either side of the best cell (default 2)")
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if args.refine_radius is not None and args.refine is None:
        ap.error("--refine-radius needs --refine F: it is the size of the refinement's boxes")
    if args.refine is not None and args.refine < 2:
        ap.error(f"--refine {args.refine}: need a factor of at least 2")
    if args.refine_radius is not None and args.refine_radius < 0:
        ap.error(f"--refine-radius {args.refine_radius}: need at least 0")
    if args.refine_radius is None:
        args.refine_radius = 2
    if args.residuals and args.draws is not None:
        ap.error("--residuals takes a fixed structure: the residuals under draws of the structure are not computed (leave out --draws)")
    if args.draws is not None and args.draws < 1:
        ap.error(f"--draws {args.draws}: need at least one draw")
    if args.draw_weights and args.draws is None:
        ap.error("--draw-weights needs --draws K: the weights are those of the K draws")
    if not args.stack:
        for given, name in ((args.time_bins is not None, "--time-bins"), (args.stack_volume, "--stack-volume"),
                            (args.stack_resolved, "--stack-resolved"), (args.level is not None, "--level")):
            if given:
                ap.error(f"{name} needs --stack: it is an option of the stacked density")
    n_bins = 1 if args.time_bins is None else args.time_bins
    levels = [0.68, 0.95] if args.level is None else args.level
    if n_bins < 1:
        ap.error("--time-bins must be at least 1")
    if any(not 0.0 < v <= 1.0 for v in levels):
        ap.error("--level must lie in (0, 1]")
    r5 = Step5Run.open(args.parameter_file, windows=args.windows)
    par, work, win_id = r5.par, r5.work, r5.win_id
    grid = grid_from_args(ap, args, par)
    structure = args.structure if args.structure else work
    if args.draws is None:
        vs, qs, t_corr, a_corr = read_structure(structure, par.stations)
        evaluate, stem = locate, "hypo_grid"
    else:
        vs, qs, t_corr, a_corr, records = read_structure_draws(structure, par.stations, par.n_stations, args.draws, records=True)
        evaluate, stem = locate_marginal, "hypo_grid_marginal"
    if not win_id:
        raise SystemExit("ERROR: no window to locate")

    res, ev, resid, n_unresolved, fine = _evaluate(r5, args, win_id, grid, evaluate, (t_corr, vs, a_corr, qs), n_bins)

    def write(name, text):
        with open(os.path.join(work, stem + name), "w") as fh:
            fh.write(text)

    write(".stat", stat_text(win_id, marginal_quantiles(np.concatenate([res["marg_x"], res["marg_y"], res["marg_z"]], axis=1), grid)))
    write(".best.dat", best_text(win_id, res, grid))
    if args.volume_of is not None:
        if args.volume_of not in win_id:
            raise SystemExit(f"ERROR: --volume-of {args.volume_of} is not among the windows")
        write(".%d.vol.dat" % args.volume_of, volume_text(_volume_of(r5, args, grid, evaluate, (t_corr, vs, a_corr, qs)), grid))
    sys.stdout.write(summary_text(res, grid, args.draws, args.precision))
    if args.stack:
        for nm in MAPS:
            if nm != "vol" or args.stack_volume:
                write(".density.%s.dat" % nm, stack_map_text(nm, res["stack" if nm == "vol" else nm], grid, levels))
        sys.stdout.write(stack_summary_text(res["tally"], face_share(res["stack"]), n_unresolved))
    if resid is not None:
        rr, t_stdv, a_stdv = resid
        use = (bool(par.get_use_time()), bool(par.get_use_amp()))
        write(".residuals.dat", residuals_text(win_id, par.stations, rr["res"], t_stdv, a_stdv, use))
        write(".fit.dat", fit_text(win_id, rr["fit"], t_stdv, use))
        write(".stations.dat", stations_text(win_id, par.stations, rr["res"], t_stdv, a_stdv, use))
        sys.stdout.write(stations_summary_text(win_id, par.stations, rr["res"], t_stdv, a_stdv, use))
    if ev is not None:
        write(".draws.dat", draws_text(win_id, ev, records))
        write(".structure.dat", structure_text(records, vs, qs, ev["log_z"]))
        sys.stdout.write(draws_summary_text(ev, args.draws))
    if fine is not None:
        write(".refined.stat", refined_stat_text(win_id, fine))
        write(".refined.best.dat", refined_best_text(win_id, fine))
        sys.stdout.write(refined_summary_text(fine, args.refine, args.refine_radius))


if __name__ == "__main__":
    main()
