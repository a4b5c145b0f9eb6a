"""What tests/test_locate_refine.py (CPU) and tests/test_gpu_locate_refine.py (the device) share: the noise-free recovery
construction of the coarse-to-fine refinement, a plain numpy evaluation of a window's log posterior under a
flat prior with both data types, and the refinement carried out with it, so that the construction is re-checked on the CPU
before the device is held to it."""
import functools

import numpy as np

from hypotremormcmc_amd import locate as lc
from tests import locate_cases as cases
from tests import locate_restatement as lr

RECOVERY_SEED, RECOVERY_FACTOR = 97, 4


def fine_whole_grid(grid, factor):
    """the whole-box grid of cell dv / factor"""
    g = np.asarray(grid, dtype=np.float64)
    return np.array([v for a in range(3) for v in (g[3 * a], g[3 * a + 1] / factor, g[3 * a + 2] * factor)])


@functools.lru_cache(maxsize=None)
def recovery_case(seed=RECOVERY_SEED, factor=RECOVERY_FACTOR):
    """6 windows, 12 stations drawn as cases.recovery_case draws them; every truth on a centre of the whole-box fine grid, the
    observations the restatement's own forward there"""
    rng = np.random.default_rng(seed)
    S, E = 12, 6
    sta = (rng.uniform(-50, 50, S), rng.uniform(-50, 50, S), rng.uniform(0, 2, S))
    tc, vs, ac, qs = cases.structure(S, seed)
    grid = cases.RECOVERY_GRID
    fine = fine_whole_grid(grid, factor)
    n = lr.counts(fine)
    cell = np.stack([rng.integers(0, n[a], E) for a in range(3)], axis=1)
    truth = np.stack([lr.centres(fine, a)[cell[:, a]] for a in range(3)], axis=1)
    t, a = lr.synthetics(sta, truth, tc, vs, ac, qs)
    obs = (t, np.full_like(t, 0.1), a, np.full_like(a, 0.05))
    return {"sta": sta, "obs": obs, "grid": grid, "factor": factor, "structure": (tc, vs, ac, qs), "truth": truth, "cell": cell}


def numpy_lp(sta, obs, structure, grid, origin=None):
    """[E][nz][ny][nx]: every window's log-likelihood term at the cell centres up to its constant (flat prior, both data types,
    no missing data): -0.5 sum_j p_j (demeaned residual_j)^2 per data type, in plain numpy.  origin [E][3]: every window on
    the grid's cells from its own origin"""
    tc, vs, ac, qs = structure
    t_obs, t_stdv, a_obs, a_stdv = obs
    E = t_obs.shape[0]
    nx, ny, nz = lr.counts(grid)
    out = np.empty((E, nz, ny, nx))
    for e in range(E):
        g = np.array(grid, dtype=np.float64)
        if origin is not None:
            g[0::3] = origin[e]
        xyz = lr.cell_xyz(g).reshape(-1, 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_syn, a_syn = lr.synthetics(sta, xyz, tc, vs, ac, qs)
            lp = np.zeros(xyz.shape[0])
            for syn, ob, sd in ((t_syn, t_obs[e], t_stdv[e]), (a_syn, a_obs[e], a_stdv[e])):
                p = 1.0 / sd ** 2
                r = syn - ob[None]
                m = (p[None] * r).sum(axis=1) / p.sum()
                lp -= 0.5 * (p[None] * (r - m[:, None]) ** 2).sum(axis=1)
        out[e] = lp.reshape(nz, ny, nx)
    return out


def first_best(vol):
    """[E] the first of the largest cells of vol [E][...], NaN left out"""
    flat = np.where(np.isnan(vol), -np.inf, vol).reshape(vol.shape[0], -1)
    return np.argmax(flat, axis=1)


def numpy_refine(rec, radius):
    """the refinement of a recovery case with numpy_lp in the place of the device: a dict of index [E] (within the box), best
    [E][3], inner_face [E], i0, fine_grid, gap [E] (best minus second lp of the fine pass) and coarse_index"""
    coarse = first_best(numpy_lp(rec["sta"], rec["obs"], rec["structure"], rec["grid"]))
    bx = lc.refine_boxes(coarse, rec["grid"], rec["factor"], radius)
    vol = numpy_lp(rec["sta"], rec["obs"], rec["structure"], bx["fine_grid"], bx["origins"])
    idx = first_best(vol)
    nf = lr.counts(bx["fine_grid"])
    ijk = np.stack([idx % nf[0], (idx // nf[0]) % nf[1], idx // (nf[0] * nf[1])], axis=1)
    best = np.stack([bx["origins"][:, a] + (ijk[:, a] + 0.5) * bx["fine_grid"][3 * a + 1] for a in range(3)], axis=1)
    inner, _ = lc.box_faces(idx, bx["fine_grid"], bx["i0"], bx["widths"], rec["grid"])
    srt = np.sort(vol.reshape(vol.shape[0], -1), axis=1)
    return {"index": idx, "best": best, "inner_face": inner, "i0": bx["i0"], "fine_grid": bx["fine_grid"], "gap": srt[:, -1] - srt[:, -2],
            "coarse_index": coarse}


def truth_index(rec, i0, fine_grid):
    """[E] the truth's linear index within the box that begins at coarse cell i0, -1 where the truth lies outside it"""
    nf = lr.counts(fine_grid)
    rel = rec["cell"] - np.asarray(i0) * rec["factor"]
    inside = np.all((rel >= 0) & (rel < np.array(nf)[None]), axis=1)
    return np.where(inside, rel[:, 0] + nf[0] * (rel[:, 1] + nf[1] * rel[:, 2]), -1)
