"""A plain numpy restatement of htm_forward_locate_residuals (include/htm_hip.h) for the tests: from a given
volume of log posteriors, the stations' residuals, the offsets and chi2 at the best cell and as means over the posterior, in
the reference's TWO-PASS form (the weighted mean first, then the residuals about it: cls_forward.f90:125-132, :284, :295) --
the library takes one pass through shifted sums.  `dtype` numpy.float64 or numpy.longdouble: the second is what the first is
held against without a device (tests/test_locate_residuals.py).  It also gives the scales the bounds are stated in:

    X_dj(c)  = |syn_j| + |obs_j| + sum_k p_k (|syn_k| + |obs_k|) / sum_k p_k      the absolute terms of rho_dj(c)
    Xm_d(c)  = sum_k p_k (|syn_k| + |obs_k|) / sum_k p_k                           the absolute terms of m_d(c) (X's second part)
    S_d(c)   = sum_j p_j |rho_j(c)| X_j(c)                                         chi2's: d(rho^2) = 2 rho d(rho), and the header's
                                                                                   bound is stated without the 2
    Q(best) + sum_c (w / W) Q(c) for each of them: "bar", what a posterior mean about the best cell is made of

and, for the single-precision forward, the same three with tests/locate_fp32_restatement.py's scales (|d / vs| + |t_corr|;
|d pi f / (qs vs)| + |ln d| + |a_corr|) in the place of |syn| + |obs|, each taken U 2^-24 times: what one relative rounding of
every magnitude a synthetic passes through moves rho, m and chi2 by (chi2 in the fp64 bound's own form, without the 2).

The variance's fp32 widening is this file's own propagation, not a form the header states: with delta = U 2^-24 Fmbar the most that
u = m(c) - m(best) moves, the variance sum w u^2 / W - (sum w u / W)^2 moves by no more than 2 sd delta + delta^2."""
import math

import numpy as np

from tests import locate_restatement as lr

FREQ = lr.FREQ
EPS = np.finfo(np.float64).eps


def precisions(obs, e):
    """(p_t, p_a, constant_t, constant_a) of event e under init_forward's missing-data rule: precision 1, log stdv := 1.0"""
    ts, as_, lts, las = lr._precisions(obs[1][e], obs[3][e])
    return 1.0 / ts ** 2, 1.0 / as_ ** 2, float(np.sum(lr.LOG_2PI_HALF + lts)), float(np.sum(lr.LOG_2PI_HALF + las))


def synthetics(sta, xyz, t_corr, vs, a_corr, qs, dtype=np.float64):
    """t, a [cells][S] and their scales st, sa (module docstring), in dtype"""
    T = dtype
    sx, sy, sz = (np.asarray(v, dtype=T) for v in sta)
    ev = np.asarray(xyz, dtype=T).reshape(-1, 3)
    tc, ac = np.asarray(t_corr, dtype=T), np.asarray(a_corr, dtype=T)
    d = np.sqrt((ev[:, None, 0] - sx[None]) ** 2 + (ev[:, None, 1] - sy[None]) ** 2 + (ev[:, None, 2] - sz[None]) ** 2)
    k = T(math.pi) * T(FREQ) / (T(qs) * T(vs))
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.log(d)
        return d / T(vs) - tc[None], -d * k - ln - ac[None], np.abs(d / T(vs)) + np.abs(tc)[None], np.abs(d * k) + np.abs(ln) + np.abs(ac)[None]


def _about_best(q, best, w, inc, W):
    """q(best) + sum over the included cells of w (q - q(best)) / W, along axis 0: by selection"""
    return q[best] + ((w[inc].reshape((-1,) + (1,) * (q.ndim - 1))) * (q[inc] - q[best])).sum(axis=0) / W


def restate(sta, obs, use, structure, grid, vol, dtype=np.float64):
    """-> dict of [E]-leading arrays: res [E][S][4], fit [E][10] as the library lays them out (float64), index [E], and per data
    type d the scales Xbar [E][2][S], Xmbar [E][2], Sbest, Sbar [E][2], and the fp32 ones Fbar [E][2][S], Fmbar [E][2], FSbest,
    FSbar [E][2]; rho [E][2][cells][S] and chi2, m [E][2][cells] for the tests that look at single cells (NaN for a data type not in
    use, and for an event without an included cell where they are means)"""
    T = dtype
    tc, vs, ac, qs = structure
    xyz = lr.cell_xyz(grid).reshape(-1, 3)
    n_cells, S, E = xyz.shape[0], sta[0].size, obs[0].shape[0]
    syn_t, syn_a, sc_t, sc_a = synthetics(sta, xyz, tc, vs, ac, qs, T)
    out = {"res": np.full((E, S, 4), np.nan), "fit": np.full((E, 10), np.nan), "index": np.full(E, -1, dtype=np.int64),
           "rho": np.full((E, 2, n_cells, S), np.nan, dtype=T), "chi2": np.full((E, 2, n_cells), np.nan, dtype=T), "m": np.full((E, 2, n_cells), np.nan, dtype=T),
           "X": np.full((E, 2, n_cells, S), np.nan)}
    for nm in ("Xbar", "Fbar"):
        out[nm] = np.full((E, 2, S), np.nan)
    for nm in ("Xmbar", "Sbest", "Sbar", "Fmbar", "FSbest", "FSbar"):
        out[nm] = np.full((E, 2), np.nan)
    for e in range(E):
        p_t, p_a, _, _ = precisions(obs, e)
        lp = np.asarray(vol[e], dtype=np.float64).reshape(-1)
        inc = lr.included(lp)
        best = int(np.argmax(np.where(inc, lp, -np.inf))) if inc.any() else -1
        out["index"][e] = best
        if best >= 0:
            w = np.zeros(n_cells, dtype=T)
            w[inc] = np.exp(lp[inc].astype(T) - T(lp[best]))
            W = w[inc].sum()
        for d, (on, syn, ob, p, sc) in enumerate(((use[0], syn_t, obs[0][e], p_t, sc_t), (use[1], syn_a, obs[2][e], p_a, sc_a))):
            if not on:
                continue
            p, ob = np.asarray(p, dtype=T), np.asarray(ob, dtype=T)
            with np.errstate(invalid="ignore", over="ignore"):
                r = syn - ob[None]                                        # [cells][S]
                m = (p[None] * r).sum(axis=1) / p.sum()                   # first pass
                rho = m[:, None] - r                                      # second pass
                chi2 = (p[None] * rho * rho).sum(axis=1)
                A = np.abs(syn) + np.abs(ob)[None]
                Xm = (p[None] * A).sum(axis=1) / p.sum()
                X = A + Xm[:, None]
                Sx = (p[None] * np.abs(rho) * X).sum(axis=1)
                Fm = (p[None] * sc).sum(axis=1) / p.sum()
                F = sc + Fm[:, None]
                FS = (p[None] * np.abs(rho) * F).sum(axis=1)
            out["rho"][e, d], out["chi2"][e, d], out["m"][e, d], out["X"][e, d] = rho, chi2, m, X
            if best < 0:
                continue
            mean = lambda q: _about_best(q, best, w, inc, W)
            bar = lambda q: np.asarray(q[best] + (w[inc].reshape((-1,) + (1,) * (q.ndim - 1)) * q[inc]).sum(axis=0) / W, dtype=np.float64)
            out["res"][e, :, 2 * d], out["res"][e, :, 2 * d + 1] = rho[best], mean(rho)
            u = m - m[best]
            m1 = (w[inc] * u[inc]).sum() / W
            var = (w[inc] * u[inc] * u[inc]).sum() / W - m1 * m1
            out["fit"][e, 5 * d:5 * d + 5] = [m[best], m[best] + m1, np.sqrt(max(var, T(0.0))), chi2[best], mean(chi2)]
            out["Xbar"][e, d], out["Xmbar"][e, d], out["Sbest"][e, d], out["Sbar"][e, d] = bar(X), bar(Xm), Sx[best], bar(Sx)
            out["Fbar"][e, d], out["Fmbar"][e, d], out["FSbest"][e, d], out["FSbar"][e, d] = bar(F), bar(Fm), FS[best], bar(FS)
    return out


RTOL = 1e-12
U32 = 2.0 ** -24


def bounds(r, e, d, ulps=0):
    """the bounds of event e, data type d from restate's scales: (res [S], m, chi2_best, chi2_mean, var(sd, var) -> bound); ulps =
    U of tests/locate_fp32_restatement.py for the single-precision forward, 0 for fp64"""
    f = ulps * U32
    res = RTOL * r["Xbar"][e, d] + f * r["Fbar"][e, d]
    m = RTOL * r["Xmbar"][e, d] + f * r["Fmbar"][e, d]
    chi_b = RTOL * r["Sbest"][e, d] + f * r["FSbest"][e, d]
    chi_m = RTOL * r["Sbar"][e, d] + f * r["FSbar"][e, d]
    delta = f * r["Fmbar"][e, d]

    def var(sd, v):
        return RTOL * v + 8 * EPS * r["Xmbar"][e, d] * sd + 2.0 * sd * delta + delta * delta

    return res, m, chi_b, chi_m, var


def compare(got_res, got_fit, r, use, ulps=0, what=""):
    """got_res [E][S][4], got_fit [E][10] against restate's r: the NaN pattern exactly, every number within its bound; returns the
    worst ratio to the bound per kind"""
    worst = {"res": 0.0, "m": 0.0, "chi2": 0.0, "var": 0.0}
    E = got_res.shape[0]
    for e in range(E):
        for d in range(2):
            R, F = got_res[e, :, 2 * d:2 * d + 2], got_fit[e, 5 * d:5 * d + 5]
            if not use[d] or r["index"][e] < 0:
                assert np.isnan(R).all() and np.isnan(F).all(), (what, e, d)
                continue
            assert np.isfinite(R).all() and np.isfinite(F).all(), (what, e, d, R, F)
            b_res, b_m, b_cb, b_cm, b_var = bounds(r, e, d, ulps)
            want_R, want_F = r["res"][e, :, 2 * d:2 * d + 2], r["fit"][e, 5 * d:5 * d + 5]
            ratio = np.abs(R - want_R) / b_res[:, None]
            worst["res"] = max(worst["res"], float(ratio.max()))
            assert np.all(ratio <= 1.0), (what, e, d, "res", float(ratio.max()))
            for k in (0, 1):
                q = abs(F[k] - want_F[k]) / b_m
                worst["m"] = max(worst["m"], float(q))
                assert q <= 1.0, (what, e, d, "m", k, F[k], want_F[k])
            for k, b in ((3, b_cb), (4, b_cm)):
                q = abs(F[k] - want_F[k]) / b if b > 0 else float(F[k] != want_F[k])
                worst["chi2"] = max(worst["chi2"], float(q))
                assert q <= 1.0, (what, e, d, "chi2", k, F[k], want_F[k])
            sd = want_F[2]
            bv = b_var(sd, sd * sd)
            q = abs(F[2] ** 2 - sd * sd) / bv if bv > 0 else float(F[2] != sd)
            worst["var"] = max(worst["var"], float(q))
            assert q <= 1.0, (what, e, d, "var", F[2], sd)
    return worst
