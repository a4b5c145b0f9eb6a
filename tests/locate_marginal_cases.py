"""The draws of the structure and the reference volumes that tests/test_locate_marginal.py (CPU: the reference's side of every
precondition) and tests/test_gpu_locate_marginal.py (the device) share.  The data, grids, structures and priors are those of
tests/locate_cases.py; the reference of a cell is numpy's m + log(sum_k exp(l_k - m)) - log K over the oracle's volume
lr.ell_volume of every draw, and A, which the parity criterion is normalised by, the largest lr.abs_terms among the draws."""
import functools

import numpy as np

from tests import locate_cases as cases
from tests import locate_restatement as lr

KS = (1, 2, 7, 8, 9, 17, 33)             # straddle every power-of-two block of draws up to 32


def scale(which, n_sta):
    """wide: one draw dominates most cells (the running maximum, weights that underflow); tight: several draws carry weight,
    so that a dropped or a doubled draw shows -- the more stations, the closer the draws have to lie for that"""
    if which == "wide":
        return 1.0
    return 0.02 if n_sta < 64 else 5e-4


@functools.lru_cache(maxsize=None)
def draws(n_sta, seed, which, K):
    """K draws about cases.structure(n_sta, seed): t_corr [K][S], vs [K], a_corr [K][S], qs [K]"""
    s = scale(which, n_sta)
    tc, vs, ac, qs = cases.structure(n_sta, seed)
    rng = np.random.default_rng(3000 + seed)
    t = tc[None] + s * rng.normal(0.0, 0.05, (K, n_sta))
    v = vs * (1.0 + 0.03 * s * rng.normal(size=K))
    a = ac[None] + s * rng.normal(0.0, 0.02, (K, n_sta))
    q = qs * (1.0 + 0.1 * s * rng.normal(size=K))
    return t, v, a, q


def mixture(ell_k):
    """[K][...] -> log((1 / K) sum_k exp(l_k)): NaN where any draw is NaN, -inf where every draw is -inf"""
    ell_k = np.asarray(ell_k, dtype=np.float64)
    K = ell_k.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(ell_k, axis=0)
        ref = np.where(np.isfinite(m), m, 0.0)
        out = m + np.log(np.sum(np.exp(ell_k - ref[None]), axis=0)) - np.log(K)
    out = np.where(np.isneginf(m), -np.inf, out)
    return np.where(np.isnan(ell_k).any(axis=0), np.nan, out)


@functools.lru_cache(maxsize=None)
def _draw_volume(key, which, K, k):
    """(ell, abs) [E][nz][ny][nx] of draw k of K of a case"""
    c = _base(key)
    t, v, a, q = draws(c["n_sta"], c["seed"], which, K)
    ut, ua = c["use"]
    return (lr.ell_volume(c["sta"], c["obs"], ut, ua, t[k], v[k], a[k], q[k], c["grid"]),
            lr.abs_terms(c["sta"], c["obs"], ut, ua, t[k], v[k], a[k], q[k], c["grid"]))


@functools.lru_cache(maxsize=None)
def _base(key):
    if key == "excluded":
        c = dict(cases.excluded_case(), n_sta=6, seed=41)
    else:
        n_sta, n_events, grid_name, mode = key
        c = dict(cases.parity_case(n_sta, n_events, grid_name, mode), n_sta=n_sta, seed=7 * n_sta + n_events)
    pr = [lr.log_prior(c["grid"], p) for p in c["prior"]]
    c["log_prior"], c["log_prior_abs"] = np.stack([p[0] for p in pr]), np.stack([p[1] for p in pr])
    return c


def marginal_case(key, K, which):
    """key = (n_sta, n_events, grid_name, mode) of cases.parity_case, or "excluded": the case's data, grid and prior, the K
    draws of the set `which`, the per-draw volumes ell_k [K][E][nz][ny][nx], the reference ell and lp_prior, and abs,
    abs_prior: the largest sum of absolute terms among the draws"""
    c = dict(_base(key))
    vols = [_draw_volume(key, which, K, k) for k in range(K)]
    ell_k = np.stack([v[0] for v in vols])
    ab = np.max(np.stack([v[1] for v in vols]), axis=0)
    ell = mixture(ell_k)
    with np.errstate(invalid="ignore"):
        lp_prior = ell + c["log_prior"]
    c.update(draws=draws(c["n_sta"], c["seed"], which, K), ell_k=ell_k, ell=ell, abs=ab, lp_prior=lp_prior, abs_prior=ab + c["log_prior_abs"])
    return c


def weights(ell_k):
    """[K][...] normalised weights of the draws per cell"""
    with np.errstate(invalid="ignore"):
        w = np.exp(ell_k - np.max(ell_k, axis=0)[None])
    return w / w.sum(axis=0)[None]


# the cases whose preconditions tests/test_locate_marginal.py checks, K = 9
PRECONDITION_CASES = [(3, 1, "5x3x2", "both"), (3, 1, "5x3x2", "amp"), (65, 2, "67x3x5", "both"), (64, 1, "5x3x2", "time"), (64, 2, "5x3x2", "both")]


def write_calibration(d, names, n_ranks=2, n_rec=6, seed=5, vs=3.0, qs=250.0):
    """a calibration run's files in `d`: the two .stat files (medians vs, qs, zero corrections) and n_ranks x n_rec records of
    vs, qs, t_corr, a_corr that scatter about them; returns the stacked samples vs [n], qs [n], t_corr [n][S], a_corr [n][S]"""
    import os

    from hypotremormcmc_amd import run_files

    S = len(names)
    cases.write_structure(d, names, np.zeros(S), np.zeros(S), vs=vs, qs=qs)
    rng = np.random.default_rng(seed)
    out = {"vs": [], "qs": [], "t_corr": [], "a_corr": []}
    for r in range(n_ranks):
        its = 100 + 10 * np.arange(n_rec)
        smp = {"vs": vs * (1.0 + 0.01 * rng.normal(size=n_rec)), "qs": qs * (1.0 + 0.05 * rng.normal(size=n_rec)),
               "t_corr": rng.normal(0.0, 0.02, (n_rec, S)), "a_corr": rng.normal(0.0, 0.01, (n_rec, S))}
        for nm, v in smp.items():
            run_files.write_sample_file(os.path.join(d, "%s.%02d.out" % (nm, r)), its, v)
            out[nm].append(v)
    return tuple(np.concatenate(out[nm], axis=0) for nm in ("vs", "qs", "t_corr", "a_corr"))
