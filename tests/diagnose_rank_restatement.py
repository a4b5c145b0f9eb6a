"""Plain-numpy restatement of the rank-normalised diagnostics (Vehtari et al. 2021).  It shares no code with
the product; §3.6 (R-hat and ESS of a matrix) is tests/diagnose_restatement.diagnose.

Input: x [M*N][n_par], sequence m in rows m*N .. m*N + N - 1, R = M*N.  Per column:
  r_i = (#{x < x_i} + #{x <= x_i} + 1) / 2, the 1-based average rank among all R rows (-0.0 == +0.0 as numpy compares them;
        all rows rank, also the middle row of an odd N that the split then drops -- Stan drops it first);
  z_i = Phi^-1((r_i - 3/8) / (R + 1/4)), Phi^-1 = statistics.NormalDist().inv_cdf, evaluated once per distinct rank;
  folded: the same of y_i = |x_i - med|, med = 0.5 (x_((R+1)/2) + x_(R/2+1)) (1-based order statistics, integer division);
  tails: for p in {0.05, 0.95}: h = (R-1) p, k = floor(h), g = h - k, a = x_(k+1), b = x_(min(k+2, R)), q = a + g (b - a);
        I05 = [x <= q05], I95 = [x >= q95] as 0.0 / 1.0.
out [n_par][4] = rhat(z), rhat(zf), ess(z), min(ess(I05), ess(I95)) (NaN if either is)."""
import math
import statistics

import numpy as np

from tests import diagnose_restatement as dr

_INV = statistics.NormalDist().inv_cdf


def ranks(x):
    """[R][n_par] average ranks, exact half-integers"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    r = np.empty(x.shape)
    for p in range(x.shape[1]):
        s = np.sort(x[:, p])
        r[:, p] = (np.searchsorted(s, x[:, p], side="left") + np.searchsorted(s, x[:, p], side="right") + 1) / 2.0
    return r


def z_of_ranks(r):
    R = r.shape[0]
    u, inv = np.unique(r, return_inverse=True)
    zu = np.array([_INV((v - 0.375) / (R + 0.25)) for v in u])
    return zu[inv].reshape(r.shape)


def median(x):
    x = np.asarray(x, dtype=np.float64)
    s = np.sort(x, axis=0)
    R = x.shape[0]
    return 0.5 * (s[(R + 1) // 2 - 1] + s[R // 2 + 1 - 1])


def folded(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    return np.abs(x - median(x)[None, :])


def quantile(x, p):
    s = np.sort(np.asarray(x, dtype=np.float64), axis=0)
    R = s.shape[0]
    h = (R - 1) * p
    k = math.floor(h)
    g = h - k
    a, b = s[k], s[min(k + 2, R) - 1]
    return a + g * (b - a)


def indicators(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    return (x <= quantile(x, 0.05)[None, :]).astype(np.float64), (x >= quantile(x, 0.95)[None, :]).astype(np.float64)


def diagnose_rank(x, n_seq, max_lag=1000):
    """out [n_par][4]; parts = the four matrices z, zf, I05, I95; refs = tests/diagnose_restatement.diagnose of each"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    z = z_of_ranks(ranks(x))
    zf = z_of_ranks(ranks(folded(x)))
    i05, i95 = indicators(x)
    parts = (z, zf, i05, i95)
    refs = [dr.diagnose(m, n_seq, max_lag) for m in parts]
    out = np.empty((x.shape[1], 4))
    out[:, 0] = refs[0][0][:, 0]
    out[:, 1] = refs[1][0][:, 0]
    out[:, 2] = refs[0][0][:, 1]
    e05, e95 = refs[2][0][:, 1], refs[3][0][:, 1]
    out[:, 3] = np.where(np.isnan(e05) | np.isnan(e95), np.nan, np.minimum(e05, e95))
    return out, parts, refs
