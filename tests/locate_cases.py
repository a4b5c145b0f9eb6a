"""The data sets, structures and grids that tests/test_locate.py (CPU: the restatement's side of every precondition) and
tests/test_gpu_locate.py (the device) share, and the restatement's results for them, computed once per process."""
import functools

import numpy as np

from hypotremormcmc_amd import synth
from tests import helpers
from tests import locate_restatement as lr

GRIDS = {
    "1x1x1": np.array([-3.0, 6.0, 1, 2.0, 5.0, 1, 4.0, 3.0, 1]),
    "5x3x2": np.array([-30.0, 12.0, 5, -20.0, 13.0, 3, 1.0, 7.0, 2]),
    # a row longer than a wave; 1005 cells: no multiple of a wave, a workgroup or a tile
    "67x3x5": np.array([-44.0, 1.3, 67, -21.0, 14.0, 3, 0.5, 3.1, 5]),
    # tiles of 58 rows, two per layer, the second ragged (2 rows): 16 cells per thread in four chunks, marginals and mixed moments
    # over several tiles
    "70x60x2": np.array([-42.0, 1.2, 70, -36.0, 1.2, 60, 2.0, 6.0, 2]),
    # a row longer than a workgroup: 13 rows per tile would fit, the layer has 3
    "300x3x1": np.array([-45.0, 0.3, 300, -10.0, 9.0, 3, 5.0, 2.0, 1]),
}
MODES = {"both": (True, True), "time": (True, False), "amp": (False, True)}


def arrays(data, n_events=None):
    """(sta, obs) of a SynthData: (sx, sy, sz), (t_obs, t_stdv, a_obs, a_stdv), the first n_events events"""
    e = slice(0, n_events)
    return (data.sta_x, data.sta_y, data.sta_z), (data.t_obs[e], data.t_stdv[e], data.a_obs[e], data.a_stdv[e])


def structure(n_sta, seed):
    """t_corr, vs, a_corr, qs: a structure that is not the one the data were made with"""
    rng = np.random.default_rng(1000 + seed)
    return rng.normal(0.0, 0.2, n_sta), 3.2, rng.normal(0.0, 0.05, n_sta), 230.0


def prior_of(sta, obs, seed):
    """[E][5] = mu_x, mu_y, w_xy, z0, w_z: every event its own, z0 below the grids' lowest centre"""
    rng = np.random.default_rng(2000 + seed)
    E = obs[0].shape[0]
    return np.stack([rng.uniform(-20, 20, E), rng.uniform(-20, 20, E), rng.uniform(10, 40, E), rng.uniform(-2, 0.4, E), rng.uniform(5, 15, E)], axis=1)


@functools.lru_cache(maxsize=None)
def parity_case(n_sta, n_events, grid_name, mode):
    """data, structure, prior and the restatement's volumes of one parity case: ell and abs [E][nz][ny][nx] (flat prior), and
    with the prior lp_prior and abs_prior"""
    seed = 7 * n_sta + n_events
    data = synth.make_synthetic(n_events, n_sta, seed)
    return _case(data, n_events, grid_name, mode, seed)


@functools.lru_cache(maxsize=None)
def missing_case(grid_name="5x3x2"):
    """the `missing` golden fixture (the missing-data rule), its first five events"""
    _, data, _ = helpers.load_case("missing")
    return _case(data, 5, grid_name, "both", 3)


def _case(data, n_events, grid_name, mode, seed):
    sta, obs = arrays(data, n_events)
    ut, ua = MODES[mode]
    grid = GRIDS[grid_name]
    tc, vs, ac, qs = structure(data.n_sta, seed)
    prior = prior_of(sta, obs, seed)
    ell = lr.ell_volume(sta, obs, ut, ua, tc, vs, ac, qs, grid)
    ab = lr.abs_terms(sta, obs, ut, ua, tc, vs, ac, qs, grid)
    pr = [lr.log_prior(grid, p) for p in prior]
    with np.errstate(invalid="ignore"):
        lp_prior = ell + np.stack([p[0] for p in pr])
    return {"sta": sta, "obs": obs, "use": (ut, ua), "grid": grid, "structure": (tc, vs, ac, qs), "prior": prior, "ell": ell, "abs": ab,
            "lp_prior": lp_prior, "abs_prior": ab + np.stack([p[1] for p in pr])}


@functools.lru_cache(maxsize=None)
def excluded_case():
    """5 x 3 x 2 cells, both data types, three events: station 0 sits exactly on the centre of cell (1, 1, 0) (log 0 in the
    amplitude term), and the prior's z0 is the lowest layer's centre for event 0 (z = z0: excluded), above it for event 1 and
    above the whole grid for event 2 (no cell left)"""
    data = synth.make_synthetic(3, 6, 41)
    grid = GRIDS["5x3x2"]
    x, y, z = (lr.centres(grid, a) for a in range(3))
    data.sta_x[0], data.sta_y[0], data.sta_z[0] = x[1], y[1], z[0]
    sta, obs = arrays(data)
    tc, vs, ac, qs = structure(6, 41)
    prior = prior_of(sta, obs, 41)
    prior[:, 3] = [z[0], z[0] + 1.0, z[1] + 0.5]
    ell = lr.ell_volume(sta, obs, True, True, tc, vs, ac, qs, grid)
    pr = [lr.log_prior(grid, p) for p in prior]
    with np.errstate(invalid="ignore"):
        lp = ell + np.stack([p[0] for p in pr])
    ab0 = lr.abs_terms(sta, obs, True, True, tc, vs, ac, qs, grid)
    return {"sta": sta, "obs": obs, "use": (True, True), "grid": grid, "structure": (tc, vs, ac, qs), "prior": prior, "ell": ell, "abs": ab0,
            "lp_prior": lp, "abs_prior": ab0 + np.stack([p[1] for p in pr])}


# ---- noise-free recovery ---------------------------------------------------------------------------------------------
RECOVERY_GRID = np.array([-40.0, 8.0, 10, -40.0, 8.0, 10, 2.0, 3.0, 5])


@functools.lru_cache(maxsize=None)
def recovery_case():
    """6 windows, 12 stations; every truth exactly on a cell centre, the observations the restatement's own forward there"""
    rng = np.random.default_rng(77)
    S, E = 12, 6
    sta = (rng.uniform(-50, 50, S), rng.uniform(-50, 50, S), rng.uniform(0, 2, S))
    tc, vs, ac, qs = structure(S, 77)
    n = lr.counts(RECOVERY_GRID)
    cell = np.stack([rng.integers(0, n[a], E) for a in range(3)], axis=1)
    truth = np.stack([lr.centres(RECOVERY_GRID, a)[cell[:, a]] for a in range(3)], axis=1)
    t, a = lr.synthetics(sta, truth, tc, vs, ac, qs)
    obs = (t, np.full_like(t, 0.1), a, np.full_like(a, 0.05))
    index = cell[:, 0] + n[0] * (cell[:, 1] + n[1] * cell[:, 2])
    return {"sta": sta, "obs": obs, "grid": RECOVERY_GRID, "structure": (tc, vs, ac, qs), "truth": truth, "index": index}


def write_structure(d, names, tc, ac, vs=3.1, qs=240.0):
    """uniform_structure.stat and station_corrections.stat as step 6 writes them"""
    import os

    from hypotremormcmc_amd.statistics import CORR_HEADER, VQ_HEADER

    with open(os.path.join(d, "uniform_structure.stat"), "w") as fh:
        fh.write(VQ_HEADER + "\n" + "".join("%13.6f" % v for v in (vs, vs - 0.1, vs + 0.1, qs, qs - 9, qs + 9)) + "\n")
    with open(os.path.join(d, "station_corrections.stat"), "w") as fh:
        fh.write(CORR_HEADER + "\n")
        for nm, t, a in zip(names, tc, ac):
            fh.write("%12s" % nm + "".join("%13.6f" % v for v in (t, t - 1, t + 1, a, a - 1, a + 1)) + "\n")


# ---- end to end ------------------------------------------------------------------------------------------------------
# (5 x 5 x 2 km cells are wider than these windows' posteriors: an interval is little more than the best cell, and a truth near
# a cell's edge falls outside it; seeds 2, 9 and 10 of 1..12 keep every window's truth inside on two axes at the least)
E2E_SEED = 2
E2E_BOUNDS = [-45.0, 45.0, -45.0, 45.0, 0.0, 20.0]
E2E_CELL = [5.0, 5.0, 2.0]


def e2e_data():
    return synth.make_synthetic(8, 16, E2E_SEED)


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """the restatement's quantiles [8][3][3] of the end-to-end job: the structure the data were made with (vs 3, qs 250, no
    corrections), step 5's prior from the default parameters"""
    from hypotremormcmc_amd.grid import make_grid
    from hypotremormcmc_amd.obs_data import ObsData

    data = e2e_data()
    sta, obs = arrays(data)
    grid = make_grid(E2E_BOUNDS, E2E_CELL)
    zero = np.zeros(16)
    mu_x, mu_y = ObsData.from_arrays(data.sta_x, data.sta_y, *obs).make_initial_guess()
    p = synth.DEFAULT_PARAMS
    ell = lr.ell_volume(sta, obs, True, True, zero, 3.0, zero, 250.0, grid)
    quant = []
    for e in range(8):
        lp = ell[e] + lr.log_prior(grid, [mu_x[e], mu_y[e], p["prior_width_xy"], p["prior_z"], p["prior_width_z"]])[0]
        quant.append(lr.quantiles(lr.summarise(lp, grid)["marg"], grid))
    return {"grid": grid, "quant": np.array(quant), "truth": data.ev_xyz}
