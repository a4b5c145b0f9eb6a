"""The single-precision forward of the three locate entry points (htm_forward_locate_set_precision, loc_station<.., F32> in
hypotremormcmc_amd/csrc/htm_locate.hpp) restated in plain numpy, on top of tests/fp32_restatement.py (the
float32 helpers, the nudges, the scales of D32) and tests/locate_restatement.py (cell centres, the prior, abs_terms): what the
mode computes (reference), how it computes it (emulate), the bound the two define, and the cases that the CPU tests
(tests/test_locate_fp32.py) and the GPU tests (tests/test_gpu_locate_fp32.py) share.

reference   the mode's DEFINITION in numpy.longdouble: the log-likelihood term of one event at every cell centre (the centres
            as the library forms them, in fp64), on the observations and precisions as they are -- this mode rounds neither to
            float -- and everything exact.  Per cell: ell, D32 and M (fp32_restatement.reference with round_inputs = False, the
            cells in the place of its events).  What is left between it and the library is arithmetic error alone.
emulate     the kernel's documented arithmetic: the three coordinate differences formed in fp64 and then rounded to float32,
            d = sqrt(fma(dz, dz, fma(dy, dy, dx dx))), log2 d, fma(d, (float)(1 / vs), -(float)t_corr), fma(-d, (float)katt,
            -fma(log2 d, ln2f, (float)a_corr)) in float32; each synthetic promoted to float64 before the observation is
            subtracted; the shifted one-pass sums of loc_station and loc_term in float64, the stations in their order (numpy's
            products and sums are not fused: that is inside the second term of the bound).  `nudge`: fp32_restatement's four
            settings -- every sqrt and log2 result left correctly rounded (0), moved by -1, 0 or +1 float32 ulp at random, or
            by +1 or by -1 ulp everywhere: the hardware's v_sqrt_f32 and v_log_f32 are "~1 ulp", not correctly rounded.  Two
            mutants for the CPU tests: f32_coords (the coordinates rounded before the difference) and next_corr (station j
            with the corrections of station j + 1).

The bound, for every included cell:

    |ell - ell_reference| <= U * 2^-24 * D32 + 1e-12 * abs_terms

D32 = sum over the stations and the data types in use of precision * |demeaned residual| * scale, scale = |d / vs| + |t_corr|
(travel time) and |d pi f / (qs vs)| + |ln d| + |a_corr| (amplitude): what one relative rounding (2^-24) of every magnitude a
synthetic passes through moves the term by, to first order.  The second term is tests/test_gpu_locate.py's own fp64 criterion
(RTOL_L of locate_restatement.abs_terms): what the fp64 part of the evaluation is held to without this mode.  With a prior,
abs_terms includes the prior's terms, as there.

U was MEASURED here, on emulate against reference alone (no device value entered it): the worst |ell_emulate - ell_reference| /
(2^-24 D32) over every included cell of every case of volume_cases() -- the cases of the GPU tests -- and the four nudges
(tests/test_locate_fp32.py prints the table; profiles/locate_fp32_tolerances.txt keeps it).  By group of cases:

    nudge            0       random  +1      -1
    2 stations       2.04    3.25    2.35    2.75
    6 stations       1.58    2.69    2.48    2.52
    64 stations      0.45    0.87    1.07    1.15
    65 stations      0.49    0.95    1.20    1.24
    missing fixture  0.78    1.48    1.07    1.45

(every grid, mode and both events of a row's cases.)  The worst is 3.25; U = 4 is the next power of two above it, the rule by which
fp32_restatement.ULPS32 = 4 was set, and equal to it: with two stations nothing averages, as there.  The documented arithmetic
spends at most 0.81 of the whole bound.  The mutants, in the same units, on the case shifted by 2^12 km (6 stations, 60 cells,
where the documented arithmetic stays within the bound under every nudge): f32_coords 0.22 .. 14.3, beyond the bound in 24
cells and 3.6 times the bound at the worst -- a cell's error is a signed sum over six stations and vanishes at some cells, so a
volume is what separates it --; next_corr 352 .. 9.4e4, beyond the bound in every cell."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import fp32_restatement as f32r
from tests import locate_cases as cases
from tests import locate_marginal_cases as mc
from tests import locate_restatement as lr
from tests.fp32_restatement import F32, LD, NUDGES, U32, _fma32, _move
from tests.test_forward_data_modes import restate_tables

U = 4
RTOL_L = 1e-12                  # tests/test_gpu_locate.py's criterion for the fp64 part, of abs_terms
LN2F = F32(0.69314718055994531)
SHIFT = 2.0 ** 12               # km: the mutants' case


def _one_event(sta, obs, e, n):
    """the stations and event e's observations, n times over: the cells take the place of fp32_restatement's events"""
    rep = lambda a: np.broadcast_to(a[e][None, :], (n, a.shape[1]))
    return SimpleNamespace(sta_x=sta[0], sta_y=sta[1], sta_z=sta[2], n_sta=sta[0].size, t_obs=rep(obs[0]), t_stdv=rep(obs[1]), a_obs=rep(obs[2]),
                           a_stdv=rep(obs[3]))


def reference(sta, obs, use, structure, grid):
    """-> (ell, D32, M), each [E][nz][ny][nx] in numpy.longdouble: the term of every event at every cell centre, NaN where the
    centre sits on a station and amplitudes are in use"""
    tc, vs, ac, qs = structure
    xyz = lr.cell_xyz(grid).reshape(-1, 3)
    nx, ny, nz = lr.counts(grid)
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for e in range(obs[0].shape[0]):
            r = f32r.reference(_one_event(sta, obs, e, xyz.shape[0]), use[0], use[1], xyz, tc, vs, ac, qs, round_inputs=False)
            out.append((r.L_ev, r.D32_ev, r.M_ev))
    return tuple(np.stack([o[k] for o in out]).reshape(-1, nz, ny, nx) for k in range(3))


def emulate(sta, obs, use, structure, grid, nudge=0, seed=0, f32_coords=False, next_corr=False):
    """-> ell [E][nz][ny][nx] in float64: loc_station<.., F32> and loc_term, term by term"""
    f64 = np.float64
    tc, vs, ac, qs = structure
    xyz = lr.cell_xyz(grid).reshape(-1, 3)
    nx, ny, nz = lr.counts(grid)
    S = sta[0].size
    rng = np.random.default_rng(seed)

    def moved(x):
        if isinstance(nudge, str):
            return _move(x, rng.integers(-1, 2, x.shape))
        return _move(x, int(nudge)) if nudge else x

    if f32_coords:      # MUTANT: the coordinates rounded before the difference
        dx, dy, dz = (xyz[:, None, a].astype(F32) - sta[a].astype(F32)[None, :] for a in range(3))
    else:
        dx, dy, dz = ((xyz[:, None, a] - sta[a].astype(f64)[None, :]).astype(F32) for a in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = moved(np.sqrt(_fma32(dz, dz, _fma32(dy, dy, dx * dx))))
        rbeta = f64(1.0) / f64(vs)
        katt = (f64(np.pi) * f64(5.0)) / (f64(qs) * f64(vs))
        tc32, ac32 = np.asarray(tc, dtype=f64).astype(F32), np.asarray(ac, dtype=f64).astype(F32)
        if next_corr:   # MUTANT: station j with the corrections of station j + 1
            tc32, ac32 = np.roll(tc32, -1), np.roll(ac32, -1)
        full = lambda v: np.broadcast_to(v, d.shape)
        ts = _fma32(d, full(F32(rbeta)), full(-tc32[None, :])).astype(f64)
        l2 = moved(np.log2(d.astype(LD)).astype(F32))
        am = _fma32(-d, full(F32(katt)), -_fma32(l2, full(LN2F), full(ac32[None, :]))).astype(f64)
        t64 = restate_tables(obs[1], obs[3], f64)
        log_2pi_half = 0.5 * np.log(2.0 * np.arccos(-1.0))
        out = np.zeros((obs[0].shape[0], xyz.shape[0]), f64)
        for e in range(obs[0].shape[0]):
            for on, k, syn, ob in ((use[0], "t", ts, obs[0][e]), (use[1], "a", am, obs[2][e])):
                if not on:
                    continue
                prec = t64[k + "_prec"][e]
                rps = 1.0 / np.sum(prec)
                const = np.sum(log_2pi_half + t64["log_" + k][e])
                r0 = syn[:, 0] - ob[0]
                s1, s2 = np.zeros(xyz.shape[0]), np.zeros(xyz.shape[0])
                for j in range(S):          # the stations in their order, the shifted sums
                    u = (syn[:, j] - ob[j]) - r0
                    pu = prec[j] * u
                    s1 = s1 + pu
                    s2 = s2 + pu * u
                out[e] -= 0.5 * (s2 - (s1 * s1) * rps) + const
    return out.reshape(-1, nz, ny, nx)


def bound(D32, ab, ulps=None):
    return (U if ulps is None else ulps) * U32 * np.asarray(D32, dtype=np.float64) + RTOL_L * np.asarray(ab, dtype=np.float64)


def units(err, D32):
    """|error| in 2^-24 D32, cell by cell (0 where D32 vanishes)"""
    err, D32 = np.abs(np.asarray(err, dtype=LD)), np.asarray(D32, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(D32 > 0, err / (LD(U32) * D32), 0.0).astype(np.float64)


# ---- the cases ------------------------------------------------------------------------------------------------------------
GRID_NAMES = ("1x1x1", "5x3x2", "67x3x5", "70x60x2", "300x3x1")
STATIONS = (2, 6, 64, 65)
MODE_NAMES = ("both", "time", "amp")
N_EVENTS = 2


def volume_cases():
    """the keys of the volume tests: (n_sta, n_events, grid, mode) of locate_cases.parity_case, and "missing" """
    return [(S, N_EVENTS, g, m) for g in GRID_NAMES for S in STATIONS for m in MODE_NAMES] + ["missing"]


def case_id(key):
    return key if isinstance(key, str) else "%dsta-%dev-%s-%s" % key


def group(key):
    """the row of the U table a case belongs to"""
    if key == "missing":
        return "missing fixture"
    return "%d stations" % key[0]


def case(key):
    return cases.missing_case() if key == "missing" else cases.parity_case(*key)


@functools.lru_cache(maxsize=None)
def references(key):
    """reference of a case -> namespace(ell, D32, M in longdouble; lp_prior = ell + the case's log prior); cached and shared: read-only"""
    c = case(key)
    ell, D32, M = reference(c["sta"], c["obs"], c["use"], c["structure"], c["grid"])
    pr = np.stack([lr.log_prior(c["grid"], p)[0] for p in c["prior"]])
    with np.errstate(invalid="ignore"):
        lp = ell + pr.astype(LD)
    for a in (ell, D32, M, lp):
        a.setflags(write=False)
    return SimpleNamespace(ell=ell, D32=D32, M=M, lp_prior=lp)


def check_volume(vol, ref, D32, ab, what, ulps=None):
    """the same NaN / -inf pattern as the reference, and every other cell within the bound; returns the worst |error| / bound"""
    vol = np.asarray(vol)
    assert vol.shape == ref.shape, what
    assert np.array_equal(np.isnan(vol), np.isnan(ref)), what
    assert np.array_equal(np.isneginf(vol), np.isneginf(ref)), what
    fin = np.isfinite(ref)
    assert np.isfinite(vol[fin]).all(), what
    err = np.abs(vol[fin].astype(LD) - ref[fin]).astype(np.float64)
    b = bound(D32[fin], ab[fin], ulps)
    worst = float(np.max(err / b)) if err.size else 0.0
    in_units = float(np.max(units(err, D32[fin]))) if err.size else 0.0
    print(f"{what}: {int(fin.sum())} cells, worst |ell - ell_ref| = {in_units:.3f} x 2^-24 D32 = {worst:.3f} of the bound")
    assert np.all(err <= b), (what, worst)
    return worst


@functools.lru_cache(maxsize=None)
def shifted_case():
    """parity_case(6, 2, "5x3x2", "both") moved by 2^12 km in x and y: stations, grid and prior together (the observations stay).
    Exact: the coordinates are first put on a 2^-16 km grid, so that neither the shift nor a difference of coordinates rounds in
    fp64 and the shifted term is the unshifted one; rounding a shifted coordinate to float32 leaves it to 2^-12 km."""
    c = dict(cases.parity_case(6, 2, "5x3x2", "both"))
    snap = lambda v: np.round(np.asarray(v, dtype=np.float64) / f32r.GRID) * f32r.GRID
    sx, sy, sz = (snap(v) for v in c["sta"])
    grid = c["grid"].copy()
    grid[0] += SHIFT
    grid[3] += SHIFT
    prior = c["prior"].copy()
    prior[:, 0] += SHIFT
    prior[:, 1] += SHIFT
    c.update(sta=(sx + SHIFT, sy + SHIFT, sz), grid=grid, prior=prior)
    tc, vs, ac, qs = c["structure"]
    c["abs"] = lr.abs_terms(c["sta"], c["obs"], True, True, tc, vs, ac, qs, grid)
    c["ref"] = reference(c["sta"], c["obs"], c["use"], c["structure"], grid)
    return c


# ---- the draws ------------------------------------------------------------------------------------------------------------
def marginal_reference(c):
    """from mc.marginal_case(...): (ell, b) -- the log-mean-exp over the draws of the per-draw reference terms, in longdouble, and
    the largest per-draw U 2^-24 D32 of every cell: a log-sum-exp moves by no more than its largest argument does"""
    tc, vs, ac, qs = c["draws"]
    K = len(vs)
    per = [reference(c["sta"], c["obs"], c["use"], (tc[k], vs[k], ac[k], qs[k]), c["grid"]) for k in range(K)]
    ell_k = np.stack([p[0] for p in per])
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(ell_k, axis=0)
        ell = m + np.log(np.sum(np.exp(ell_k - m[None]), axis=0)) - np.log(LD(K))
    return ell, np.max(np.stack([p[1] for p in per]), axis=0)
