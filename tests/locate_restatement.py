"""A plain numpy restatement of htm_forward_locate (include/htm_hip.h) for the tests.  The log-likelihood
term of a cell is NOT restated: it is oracle.Forward.calc_log_likelihood of a one-event forward at the cell centre.  What is
restated here is everything around it: cell centres, the log prior, the best cell, the log-sum-exp, the moments, the
marginals and their quantiles, the text of hypo_grid.stat, and `abs_terms`, the sum of the absolute values of a cell's
terms that the parity criterion is normalised by."""
import math

import numpy as np

from oracle import oracle

FREQ = 5.0
LOG_2PI_HALF = 0.5 * math.log(2.0 * math.acos(-1.0))


def counts(grid):
    g = np.asarray(grid, dtype=np.float64)
    return int(g[2]), int(g[5]), int(g[8])


def centres(grid, axis):
    """v0 + (i + 0.5) * dv: one multiplication, then one addition"""
    g = np.asarray(grid, dtype=np.float64)
    return g[3 * axis] + (np.arange(int(g[3 * axis + 2])) + 0.5) * g[3 * axis + 1]


def cell_xyz(grid):
    """[nz][ny][nx][3] cell centres"""
    x, y, z = (centres(grid, a) for a in range(3))
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([X, Y, Z], axis=-1)


def synthetics(sta, ev_xyz, t_corr, vs, a_corr, qs):
    """the forward model before the demeaning (cls_forward.f90:115-118, :201-204): t [E][S], a [E][S]"""
    sx, sy, sz = sta
    ev = np.asarray(ev_xyz, dtype=np.float64).reshape(-1, 3)
    d = np.sqrt((ev[:, None, 0] - sx[None]) ** 2 + (ev[:, None, 1] - sy[None]) ** 2 + (ev[:, None, 2] - sz[None]) ** 2)
    with np.errstate(divide="ignore"):
        return d / vs - t_corr[None], -d * math.pi * FREQ / (qs * vs) - np.log(d) - a_corr[None]


def _precisions(t_stdv, a_stdv):
    """init_forward's missing-data rule (cls_forward.f90:76-92): keyed on t_stdv alone, log-stdv := 1.0, stdv := 1"""
    ok = t_stdv > 1.0e-16
    ts, as_ = np.where(ok, t_stdv, 1.0), np.where(ok, a_stdv, 1.0)
    return ts, as_, np.where(ok, np.log(ts), 1.0), np.where(ok, np.log(as_), 1.0)


def abs_terms(sta, obs, use_time, use_amp, t_corr, vs, a_corr, qs, grid):
    """[E][nz][ny][nx]: the sum of the absolute values of the terms of a cell's log-likelihood term (per station and data type
    the misfit, log_2pi_half and the log standard deviation: cls_forward.f90:283-286, :294-297), the reference's two-pass form in
    plain fp64"""
    t_obs, t_stdv, a_obs, a_stdv = obs
    ts, as_, lts, las = _precisions(t_stdv, a_stdv)
    xyz = cell_xyz(grid).reshape(-1, 3)
    out = np.zeros((t_obs.shape[0], xyz.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        t_syn, a_syn = synthetics(sta, xyz, t_corr, vs, a_corr, qs)          # [cells][S]
        for e in range(t_obs.shape[0]):
            for use, syn, ob, sd, lsd in ((use_time, t_syn, t_obs[e], ts[e], lts[e]), (use_amp, a_syn, a_obs[e], as_[e], las[e])):
                if not use:
                    continue
                p = 1.0 / sd ** 2
                mean = np.sum(p[None] * (syn - ob[None]), axis=1) / np.sum(p)
                out[e] += np.sum((ob[None] - (syn - mean[:, None])) ** 2 / (2.0 * sd[None] ** 2), axis=1)
                out[e] += np.sum(np.abs(LOG_2PI_HALF) + np.abs(lsd))
    nx, ny, nz = counts(grid)
    return out.reshape(-1, nz, ny, nx)


def ell_volume(sta, obs, use_time, use_amp, t_corr, vs, a_corr, qs, grid):
    """[E][nz][ny][nx]: every event's term of the oracle's calc_log_likelihood at every cell centre (a one-event forward)"""
    t_obs, t_stdv, a_obs, a_stdv = obs
    xyz = cell_xyz(grid).reshape(-1, 3)
    out = np.empty((t_obs.shape[0], xyz.shape[0]))
    for e in range(t_obs.shape[0]):
        fw = oracle.Forward(sta[0], sta[1], sta[2], t_obs[e:e + 1], t_stdv[e:e + 1], a_obs[e:e + 1], a_stdv[e:e + 1], use_time, use_amp)
        for c in range(xyz.shape[0]):
            out[e, c] = fw.calc_log_likelihood(xyz[c], t_corr, vs, a_corr, qs)
    nx, ny, nz = counts(grid)
    return out.reshape(-1, nz, ny, nx)


def log_prior(grid, prior5):
    """([nz][ny][nx] log prior of one event, the sum of the absolute values of its terms): normalised Gaussians in x and y,
    the normalised depth prior of cls_model.f90:178-185; -inf at and below z0"""
    mu_x, mu_y, w_xy, z0, w_z = (float(v) for v in prior5)
    x, y, z = (centres(grid, a) for a in range(3))
    px = (-LOG_2PI_HALF - math.log(w_xy)) - (x - mu_x) ** 2 / (2.0 * w_xy * w_xy)
    py = (-LOG_2PI_HALF - math.log(w_xy)) - (y - mu_y) ** 2 / (2.0 * w_xy * w_xy)
    d = z - z0
    with np.errstate(divide="ignore", invalid="ignore"):
        pz = np.where(d > 0.0, (np.log(np.where(d > 0.0, d, 1.0)) - 2.0 * math.log(w_z)) - d * d / (2.0 * w_z * w_z), -np.inf)
        az = np.where(d > 0.0, np.abs(np.log(np.where(d > 0.0, d, 1.0))) + abs(2.0 * math.log(w_z)) + d * d / (2.0 * w_z * w_z), 0.0)
    ax = LOG_2PI_HALF + abs(math.log(w_xy)) + (x - mu_x) ** 2 / (2.0 * w_xy * w_xy)
    ay = LOG_2PI_HALF + abs(math.log(w_xy)) + (y - mu_y) ** 2 / (2.0 * w_xy * w_xy)
    lp = (px[None, None, :] + py[None, :, None]) + pz[:, None, None]
    return lp, (ax[None, None, :] + ay[None, :, None]) + az[:, None, None]


def included(lp):
    return ~np.isnan(lp) & (lp != -np.inf)


def summarise(lp, grid):
    """from one event's lp [nz][ny][nx]: index (the best cell, lowest index among ties; -1: none), best (its centre), lp,
    log_evidence = log(sum exp(lp) dx dy dz), mean [3], cov [3][3] and marg (x, y, z) under the weights exp(lp - lp_best) of
    the included cells, second (the largest lp of another cell, -inf if none)"""
    g = np.asarray(grid, dtype=np.float64)
    nx, ny, nz = counts(grid)
    lp = np.asarray(lp, dtype=np.float64).reshape(nz, ny, nx)
    inc = included(lp)
    nan3 = np.full(3, np.nan)
    if not inc.any():
        return {"index": -1, "best": nan3, "lp": np.nan, "log_evidence": np.nan, "mean": nan3, "cov": np.full((3, 3), np.nan),
                "marg": tuple(np.full(n, np.nan) for n in (nx, ny, nz)), "second": -np.inf}
    flat = np.where(inc, lp, -np.inf).reshape(-1)
    idx = int(np.argmax(flat))                                    # the first of the largest
    rest = np.delete(flat, idx)
    xyz = cell_xyz(grid)
    w = np.where(inc, np.exp(np.where(inc, lp, flat[idx]) - flat[idx]), 0.0)
    W = w.sum()
    p = w / W
    best = xyz.reshape(-1, 3)[idx]
    mean = np.array([best[a] + (p * (xyz[..., a] - best[a])).sum() for a in range(3)])      # (about the best cell: exact when all mass is there)
    d = xyz - mean
    cov = np.array([[(p * d[..., a] * d[..., b]).sum() for b in range(3)] for a in range(3)])
    return {"index": idx, "best": xyz.reshape(-1, 3)[idx], "lp": flat[idx], "log_evidence": flat[idx] + math.log(W) + math.log(g[1] * g[4] * g[7]),
            "mean": mean, "mean_abs": np.array([(p * np.abs(xyz[..., a])).sum() for a in range(3)]), "cov": cov, "marg": (p.sum(axis=(0, 1)), p.sum(axis=(0, 2)), p.sum(axis=(1, 2))),
            "second": rest.max() if rest.size else -np.inf}


def quantile(m, v0, dv, q):
    """the quantile q of one axis marginal m: in the first cell whose cumulative mass reaches q, linearly inside it"""
    c = 0.0
    for k, mk in enumerate(m):
        if c + mk >= q and mk > 0.0:
            return v0 + dv * (k + (q - c) / mk)
        c += mk
    k = max(i for i, mk in enumerate(m) if mk > 0.0)      # rounding left the total below q
    return v0 + dv * (k + 1.0)


def quantiles(marg, grid, levels=(0.025, 0.5, 0.975)):
    """[3][len(levels)] from marg = (mx, my, mz); NaN for a marginal of NaN"""
    g = np.asarray(grid, dtype=np.float64)
    return np.array([[np.nan if np.isnan(m).any() else quantile(m, g[3 * a], g[3 * a + 1], q) for q in levels] for a, m in enumerate(marg)])


def stat_text(win_id, quant):
    """hypo.stat's layout from quant [E][3][3] = 2.5 %, 50 %, 97.5 % per axis"""
    out = ["# window ID, x (50%), x (2.5%) x (97.5%), y (50%), y (2.5%), y (97.5%)z (50 %), z (2.5%), z (97.5%)"]
    for w, q in zip(win_id, quant):
        out.append("%9d" % w + "".join("%13s" % "NaN" if np.isnan(q[a][j]) else "%13.6f" % q[a][j] for a in range(3) for j in (1, 0, 2)))
    return "\n".join(out) + "\n"
