"""A plain numpy restatement of htm_forward_locate_draw_evidence (include/htm_hip.h) for the tests: the log
evidence of every draw from the per-draw volumes of tests/locate_marginal_cases.py, and the draws' effective number, largest
weight, heaviest draw and the mixture's log evidence from a log_z."""
import math

import numpy as np

from tests import locate_marginal_cases as mc
from tests import locate_restatement as lr

# (key of mc.marginal_case, K) of the parity tests, each with the sets `wide` and `tight`: every K on both sides of every block
# of draws on the 30-cell grid in every mode; 65 stations and two events; one cell; two tiles per layer, the second ragged, 16
# cells per thread; a row longer than a workgroup
PARITY = ([((3, 1, "5x3x2", mode), K) for mode in ("both", "time", "amp") for K in mc.KS]
          + [((65, 2, "67x3x5", "both"), K) for K in (8, 9)]
          + [((65, 1, "1x1x1", "time"), 33), ((3, 1, "1x1x1", "both"), 1), ((5, 1, "70x60x2", "both"), 9), ((4, 1, "300x3x1", "both"), 9)])


def log_z_ref(case, prior=True):
    """[K][E] from mc.marginal_case(...): per draw and event the logsumexp over the cells that are included under that draw of
    ell_k + log_prior (ell_k alone with prior=False), plus the log of the cell volume; -inf where no cell is included"""
    g = np.asarray(case["grid"], dtype=np.float64)
    log_cell = math.log(g[1] * g[4] * g[7])
    ell_k = case["ell_k"]
    K, E = ell_k.shape[:2]
    out = np.full((K, E), -np.inf)
    for k in range(K):
        for e in range(E):
            with np.errstate(invalid="ignore"):
                lp = (ell_k[k, e] + case["log_prior"][e]) if prior else ell_k[k, e]
            v = lp[lr.included(lp)]
            if v.size:
                m = v.max()
                out[k, e] = m + math.log(np.exp(v - m).sum()) + log_cell
    return out


def bound_scale(case, prior=True):
    """A of the parity criterion: the largest finite sum of absolute terms of a cell (abs_prior; abs with a flat prior)"""
    ab = case["abs_prior"] if prior else case["abs"]
    return float(np.max(ab[np.isfinite(ab)]))


def summarise(log_z):
    """log_z [E][K] -> dict of n_eff, w_max, log_evidence [E] and k_max [E] (int64): with w_k = exp(log_z_k - M) / S1, M the
    largest log_z of the window and S1 = sum_k exp(log_z_k - M): n_eff = S1^2 / sum_k exp(2 (log_z_k - M)), w_max = 1 / S1, k_max
    the lowest index of M, log_evidence = M + log S1 - log K.  A window whose log_z are all -inf: NaN and -1."""
    z = np.asarray(log_z, dtype=np.float64)
    E, K = z.shape
    out = {"n_eff": np.full(E, np.nan), "w_max": np.full(E, np.nan), "log_evidence": np.full(E, np.nan), "k_max": np.full(E, -1, dtype=np.int64)}
    for e in range(E):
        M = z[e].max()
        if M == -np.inf:
            continue
        d = z[e] - M
        S1, S2 = np.exp(d).sum(), np.exp(2.0 * d).sum()
        out["n_eff"][e], out["w_max"][e] = S1 * S1 / S2, 1.0 / S1
        out["k_max"][e] = int(np.argmax(z[e]))                     # the first of the largest
        out["log_evidence"][e] = M + (math.log(S1) - math.log(K))
    return out
