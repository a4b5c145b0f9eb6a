"""Location error ellipsoids of a step-5 run on the GPU: per window the 3 x 3 posterior covariance of (x, y, z), its
principal axes, and the depth-velocity trade-off, from the joint samples that step 6 summarises one axis at a time
(kernels in hypotremormcmc_amd/csrc/htm_ellipsoid.hpp).

    python -m hypotremormcmc_amd.ellipsoid <parameter file> [--level 0.68]

run in the directory of the step-5 outputs, writes `hypo_ellipsoid.stat` next to the `.stat` files of
`hypotremormcmc_amd.statistics`: one line per window of `selected_win.dat` with the mean location, the three semi-axes of
the ellipsoid that holds the fraction --level of the window's samples (each with its unit vector), the ratio of that
ellipsoid's scale to a Gaussian's (1 for a Gaussian cloud; far from 1 says the ellipsoid is a poor picture of the window),
the horizontal error ellipse and the correlation of depth with vs and with qs.  A window whose samples do not span three
dimensions, and the correlation with a parameter the job fixes, are written as NaN.  The sample distances are taken in
batches of windows under HTM_ELLIPSOID_MB MiB of device memory (default 1024).
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

from . import _lib
from .run_files import Step5Run, field
from .statistics import sample_matrix

N_OUT = 22
MAX_PIVOTS = 4
STAT_HEADER = ("# window, mean x y z, three times (semi-axis, unit vector x y z) of the ellipsoid holding the level's share of the samples, "
               "its scale over a Gaussian's, horizontal ellipse: semi-major, semi-minor, angle of the major axis from +x towards +y "
               "(degrees), corr(z, vs), corr(z, qs)")


def chi2_quantile(level: float, dof: int) -> float:
    """the `level` quantile of chi-square with 2 or 3 degrees of freedom: the squared radius of the disc / ball that holds
    that share of a standard normal cloud"""
    level = float(level)
    if not 0.0 <= level < 1.0:
        raise ValueError(f"level = {level}: need 0 <= level < 1")
    if dof == 2:
        return -2.0 * math.log1p(-level)
    if dof != 3:
        raise ValueError(f"dof = {dof}: 2 or 3")
    if level == 0.0:
        return 0.0
    cdf = lambda r: math.erf(r / math.sqrt(2.0)) - math.sqrt(2.0 / math.pi) * r * math.exp(-0.5 * r * r)
    lo, hi = 0.0, 1.0
    while cdf(hi) < level:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if cdf(mid) < level:
            lo = mid
        else:
            hi = mid
    r = 0.5 * (lo + hi)
    return r * r


def level_rank(level: float, n_mod: int) -> int:
    """the 1-based order statistic of the distances that the ellipsoid of `level` passes through"""
    level = float(level)
    if not 0.0 < level <= 1.0:
        raise ValueError(f"level = {level}: need 0 < level <= 1")
    return min(n_mod, max(1, math.ceil(level * n_mod)))


def ellipsoid(hypo, pivots=None, level: float = 0.68, device: int = 0):
    """hypo [n_mod][3 n_win] (window w in columns 3w .. 3w+2), pivots [n_mod][n_piv] or None, on the GPU.  Returns a dict:
    mean [n_win][3], cov [n_win][3][3], lam [n_win][3] (descending), axes [n_win][3][3] (column k = unit axis k), q [n_win]
    (the ellipsoid with semi-axes sqrt(q lam_k) holds `rank` = level_rank(level, n_mod) of the samples), piv_corr
    [n_win][3][n_piv], rank.  lam, axes and q of a window that does not span three dimensions are NaN."""
    x, _ = sample_matrix(hypo, "htm_hypo_ellipsoid takes", n_seq=None, name="hypo", layout="[n_mod][columns]")
    n_mod, n_col = x.shape
    if n_col < 3 or n_col % 3:
        raise ValueError(f"hypo has {n_col} columns: need x, y, z of every window")
    if n_mod < 4:
        raise ValueError(f"n_mod = {n_mod}: a covariance with its distances needs at least 4 samples")
    n_win = n_col // 3
    if pivots is None:
        p, n_piv = None, 0
    else:
        p, _ = sample_matrix(pivots, "htm_hypo_ellipsoid takes", n_seq=None, name="pivots", layout="[n_mod][columns]")
        n_piv = p.shape[1]
        if p.shape[0] != n_mod or not 1 <= n_piv <= MAX_PIVOTS:
            raise ValueError(f"pivots {p.shape}: need {n_mod} rows and 1..{MAX_PIVOTS} columns")
    rank = level_rank(level, n_mod)
    out = np.empty((n_win, N_OUT))
    corr = np.empty((n_win, 3, n_piv))
    _lib.check(_lib.load().htm_hypo_ellipsoid(device, _lib.ptr(x), _lib.ptr(p), n_mod, n_win, n_piv, rank, _lib.ptr(out),
                                              _lib.ptr(corr) if n_piv else None))
    return unpack(out, corr, rank)


def unpack(out, corr, rank):
    """the dict of `ellipsoid` from out [n_win][22] and piv_corr [n_win][3][n_piv] of htm_hypo_ellipsoid"""
    out = np.asarray(out)
    c = out[:, 3:9]
    cov = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)
    return {"mean": out[:, 0:3].copy(), "cov": cov, "lam": out[:, 9:12].copy(), "axes": out[:, 12:21].reshape(-1, 3, 3).copy(),
            "q": out[:, 21].copy(), "piv_corr": corr, "rank": rank}


def horizontal_ellipse(cov, level):
    """[n_win][3] = semi-major, semi-minor, angle (degrees in [0, 180) from +x towards +y) of the Gaussian error ellipse of the
    x-y block of cov [n_win][3][3]"""
    cov = np.asarray(cov, dtype=np.float64)
    a, b, c = cov[:, 0, 0], cov[:, 1, 1], cov[:, 0, 1]
    half = np.hypot(0.5 * (a - b), c)
    k = chi2_quantile(level, 2)
    major = np.sqrt(k * (0.5 * (a + b) + half))
    minor = np.sqrt(k * np.maximum(0.5 * (a + b) - half, 0.0))
    angle = np.degrees(0.5 * np.arctan2(2.0 * c, a - b)) % 180.0
    angle[angle >= 180.0] = 0.0          # -tiny % 180 rounds to 180
    return np.stack([major, minor, angle], axis=1)


def stat_rows(res, level, i_vs=0, i_qs=1):
    """[n_win][21]: the numbers of a line of hypo_ellipsoid.stat after the window id"""
    n_win = len(res["q"])
    semi = np.sqrt(res["q"][:, None] * res["lam"])
    rows = np.full((n_win, 21), np.nan)
    rows[:, 0:3] = res["mean"]
    for k in range(3):
        rows[:, 3 + 4 * k] = semi[:, k]
        rows[:, 4 + 4 * k:7 + 4 * k] = res["axes"][:, :, k]
    rows[:, 15] = res["q"] / chi2_quantile(level, 3)
    rows[:, 16:19] = horizontal_ellipse(res["cov"], level)
    corr = res["piv_corr"]
    if corr is not None and corr.shape[2] > max(i_vs, i_qs):
        rows[:, 19] = corr[:, 2, i_vs]
        rows[:, 20] = corr[:, 2, i_qs]
    return rows


# widths and decimals of the 21 numbers: lengths %14.6f, unit vectors, ratio and correlations %11.6f, the angle %10.3f
_FIELDS = [(14, 6)] * 3 + ([(14, 6)] + [(11, 6)] * 3) * 3 + [(11, 6)] + [(14, 6)] * 2 + [(10, 3)] + [(11, 6)] * 2


def stat_text(win_id, rows) -> str:
    """the text of hypo_ellipsoid.stat; NaN is written as NaN in the field's width"""
    lines = [STAT_HEADER]
    for w, row in zip(win_id, np.asarray(rows, dtype=np.float64)):
        lines.append("%8d" % w + "".join(field(v, wd, dc) for (wd, dc), v in zip(_FIELDS, row)))
    return "\n".join(lines) + "\n"


def summary_text(win_id, rows) -> str:
    rows = np.asarray(rows, dtype=np.float64)
    live = np.nonzero(~np.isnan(rows[:, 3]))[0]
    if not len(live):
        return "no window spans three dimensions: no ellipsoid\n"
    big = live[np.argmax(rows[live, 3])]
    odd = live[np.argmax(np.abs(rows[live, 15] - 1.0))]
    cz = np.abs(rows[:, 19])
    med = "NaN (vs is fixed)" if np.isnan(cz).all() else "%.6f" % np.nanmedian(cz)
    return (f"largest semi-axis  {rows[big, 3]:.6f}  (window {win_id[big]})\n"
            f"scale over a Gaussian's farthest from 1  {rows[odd, 15]:.6f}  (window {win_id[odd]})\n"
            f"median |corr(z, vs)|  {med}\n")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m hypotremormcmc_amd.ellipsoid", description=__doc__.split("\n\n")[0])
    ap.add_argument("parameter_file")
    ap.add_argument("--level", type=float, default=0.68, help="share of a window's samples inside its ellipsoid")
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if not 0.0 < args.level < 1.0:
        ap.error("--level must lie between 0 and 1")
    run = Step5Run.open(args.parameter_file)
    _, s = run.samples(("hypo", "vs", "qs"))
    res = ellipsoid(s["hypo"], np.hstack([s["vs"], s["qs"]]), level=args.level, device=run.device)
    rows = stat_rows(res, args.level)
    with open(os.path.join(run.work, "hypo_ellipsoid.stat"), "w") as fh:
        fh.write(stat_text(run.win_id, rows))
    sys.stdout.write(summary_text(run.win_id, rows))


if __name__ == "__main__":
    main()
