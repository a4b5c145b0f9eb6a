"""The fp32-forward / fp64-accept mode (htm_forward_set_precision, csrc/htm_device.hpp event_misfit<.., F32>) restated in plain numpy, on
top of tests/test_forward_data_modes.py: what the mode computes (reference), how it computes it (emulate), the tolerance the two
define, and the cases the CPU tests (tests/test_fp32_restatement.py) and the GPU tests (tests/test_gpu_fp32_terms.py) share.

reference   the mode's DEFINITION in numpy.longdouble, on the inputs as the library stores them: observations and precisions
            rounded to float32 (the float copies of the four streams), the reciprocal precision sums from the fp64 precisions
            (ObsRegs::rpst, rpsa), everything else exact.  What is left between it and the library is arithmetic error alone.
emulate     the kernel's documented arithmetic in float32: coordinate differences formed in fp64 and then rounded, the fused sum of
            squares, sqrt, fma(d, (float)(1 / vs), -(float)t_corr), fma(log2 d, ln2f, (float)a_corr), fma(-d, (float)katt, -lg), fp64
            from there on.  The hardware's sqrt and log2 are "~1 ulp", not correctly rounded: `nudge` moves every sqrt and log2
            result by one float32 ulp -- "random" (seeded; -1, 0 or +1 each), +1 or -1 (one sign everywhere) -- and 0 leaves them
            correctly rounded.  Three mutants for the CPU tests: f32_coords, sqrt_bias, neighbour_corr.

Tolerance (T7 of tests/test_gpu_fp32.py), for every value L the mode gives:

    |L - L_reference| <= ULPS32 * 2^-24 * D32 + 16 * 2^-53 * M

D32 = sum of precision * |residual| * scale over the entries of the data types in use: what one relative rounding (u = 2^-24) of
every magnitude a synthetic passes through moves L by, to first order; scale = |d / vs| + |t_corr| (travel time) and
|d pi f / (qs vs)| + |ln d| + |a_corr| (amplitude).  M = the sum of the magnitudes of L's terms, for the fp64 sums (the bound of
tests/test_forward_data_modes.py, ULPS_L).  A difference of two values of one event (a partial update) is judged on the sum of the
one-event D32 and M of both positions.

ULPS32 was MEASURED here, on emulate against reference alone (no GPU value entered it): the worst |L_emulate - L_reference| /
(2^-24 D32) over every case of cases() -- pair probes, exact translations, ragged shapes, the single-type modes -- the four nudge
settings and five models each, full values and one-event differences (tests/test_fp32_restatement.py prints them):

    nudge          0       random  +1      -1
    pair probes    0.95    2.31    2.15    2.07
    translations   0.22    0.32    0.82    0.61
    ragged shapes  0.97    1.98    1.61    1.44
    single type    0.57    0.79    0.73    1.04

The worst is 2.31; ULPS32 = 4 is the next power of two (the rule ULPS_L was set by).  First order, per entry: the three rounded
differences, the fused sum of squares, the rounded sqrt and its ulp (up to 2 u), the converted factor and correction and the
rounding of the fma leave room for about 7 u of the scale; with two live stations nothing averages, hence 2.3 there and 1 at 64
stations and more.  The mutants, same units: f32_coords 45 .. 1.1e6 on every pair probe shifted by 2^12 / 2^20 km (the unshifted
arithmetic: the table); sqrt_bias 3.8 .. 7.5 on the time-only pair probes and 2.6 at 37 x 64, which therefore does not separate
it from a sqrt that is one ulp off (tests/test_fp32_restatement.py); neighbour_corr 7.5e4 .. 1.9e6 on the pair probes with a
live station 64."""
import functools
from types import SimpleNamespace

import numpy as np

from hypotremormcmc_amd import synth
from tests.helpers import with_missing
from tests.test_forward_data_modes import LD, MODES, ULPS_L, restate_log_likelihood, restate_tables

U32 = 2.0 ** -24
EPS = 2.0 ** -53
ULPS32 = 4
F32 = np.float32
GRID = 2.0 ** -16           # km: coordinates on this grid shift by a power of two up to 2^20 km without a rounding
SHIFTS = (2.0 ** 12, 2.0 ** 20)
STEP = 26214 * GRID         # the 0.4 km of a partial update, on the grid
NUDGES = (0, "random", 1, -1)


def _stored(data, round_inputs):
    """the observations, the entry precisions as weights, the variances of the misfit and the precision sums as the mode has them"""
    tab = restate_tables(data.t_stdv, data.a_stdv)
    if not round_inputs:
        return dict(tab, t_obs=data.t_obs.astype(LD), a_obs=data.a_obs.astype(LD), t_var=tab["t_sd"] ** 2, a_var=tab["a_sd"] ** 2,
                    t_psum=np.sum(tab["t_prec"], axis=1), a_psum=np.sum(tab["a_prec"], axis=1))
    t64 = restate_tables(data.t_stdv, data.a_stdv, np.float64)      # (1 / stdv^2 in fp64, as htm_forward_create forms it)
    out = dict(log_t=tab["log_t"], log_a=tab["log_a"])
    for k in "ta":
        out[k + "_obs"] = getattr(data, k + "_obs").astype(F32).astype(LD)
        out[k + "_prec"] = t64[k + "_prec"].astype(F32).astype(LD)
        out[k + "_var"] = LD(1.0) / out[k + "_prec"]
        out[k + "_psum"] = np.sum(t64[k + "_prec"].astype(LD), axis=1)
    return out


def reference(data, use_time, use_amp, hypo, t_corr, vs, a_corr, qs, round_inputs=True):
    """-> namespace(L, D32, M; L_ev, D32_ev, M_ev per event).  With round_inputs = False the same operations as
    tests/test_forward_data_modes.py restate_log_likelihood, in its order: L and M equal its values exactly."""
    st = _stored(data, round_inputs)
    h = np.asarray(hypo, dtype=LD).reshape(-1, 3)
    dx = h[:, None, 0] - data.sta_x.astype(LD)[None, :]
    dy = h[:, None, 1] - data.sta_y.astype(LD)[None, :]
    dz = h[:, None, 2] - data.sta_z.astype(LD)[None, :]
    d = np.sqrt(dx ** 2 + dy ** 2 + dz ** 2)
    beta, q, pi, freq = LD(vs), LD(qs), np.arccos(LD(-1.0)), LD(5.0)
    tc, ac = np.asarray(t_corr, dtype=LD)[None, :], np.asarray(a_corr, dtype=LD)[None, :]
    t = d / beta - tc
    a = -d * pi * freq / (q * beta) - np.log(d) - ac
    t_scale = np.abs(d / beta) + np.abs(tc)
    a_scale = np.abs(d * pi * freq / (q * beta)) + np.abs(np.log(d)) + np.abs(ac)
    log_2pi_half = LD(0.5) * np.log(LD(2.0) * np.arccos(LD(-1.0)))
    E = h.shape[0]
    L, mag, sens = LD(0.0), LD(0.0), LD(0.0)
    L_ev, mag_ev, sens_ev = np.zeros(E, LD), np.zeros(E, LD), np.zeros(E, LD)
    for use, k, raw, scale in ((use_time, "t", t, t_scale), (use_amp, "a", a, a_scale)):
        if use:
            obs, prec, var, lg = st[k + "_obs"], st[k + "_prec"], st[k + "_var"], st["log_" + k]
            mean = np.sum(prec * (raw - obs), axis=1) / st[k + "_psum"]
            syn = raw - mean[:, None]
            mis = (obs - syn) ** 2 / (LD(2.0) * var)
            L = L - np.sum(mis) - log_2pi_half * mis.size - np.sum(lg)
            mag = mag + np.sum(mis) + log_2pi_half * mis.size + np.sum(np.abs(lg))
            s = np.abs(obs - syn) / var * scale
            sens = sens + np.sum(s)
            L_ev = L_ev - np.sum(mis, axis=1) - log_2pi_half * mis.shape[1] - np.sum(lg, axis=1)
            mag_ev = mag_ev + np.sum(mis, axis=1) + log_2pi_half * mis.shape[1] + np.sum(np.abs(lg), axis=1)
            sens_ev = sens_ev + np.sum(s, axis=1)
    return SimpleNamespace(L=L, D32=sens, M=mag, L_ev=L_ev, D32_ev=sens_ev, M_ev=mag_ev)


def constants_sum(data, use_time, use_amp):
    """what is left of L where every misfit vanishes: -(log sqrt(2 pi) + log stdv) summed over the entries of the types in use"""
    tab = restate_tables(data.t_stdv, data.a_stdv)
    log_2pi_half = LD(0.5) * np.log(LD(2.0) * np.arccos(LD(-1.0)))
    return -sum((np.sum(tab[k]) + log_2pi_half * tab[k].size for k, use in (("log_t", use_time), ("log_a", use_amp)) if use), LD(0.0))


def _move(x, k):
    """float32 values moved by k ulps (k an integer or an integer array); zeros stay"""
    k = np.broadcast_to(np.asarray(k, dtype=np.int32), x.shape)
    bits = x.view(np.int32).copy()
    bits = np.where(x > 0, bits + k, np.where(x < 0, bits - k, bits)).astype(np.int32)
    return bits.view(F32)


def _fma32(a, b, c):
    """fmaf: the product of two float32 values is exact in longdouble; one rounding of the sum to float32"""
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(F32)


def emulate(data, use_time, use_amp, hypo, t_corr, vs, a_corr, qs, nudge=0, seed=0, f32_coords=False, sqrt_bias=False,
            neighbour_corr=False):
    """-> (L, L_ev): the value of a full evaluation and every event's share (a partial update gives L_old + L_ev_new[e] - L_ev_old[e]).
    csrc/htm_device.hpp event_misfit<.., F32> term by term; the fp64 part in numpy's float64 (its sums in numpy's order)."""
    f64 = np.float64
    h = np.asarray(hypo, dtype=f64).reshape(-1, 3)
    E, S = h.shape[0], data.n_sta
    rng = np.random.default_rng(seed)

    def moved(x):
        if isinstance(nudge, str):
            return _move(x, rng.integers(-1, 2, x.shape))
        return _move(x, int(nudge)) if nudge else x

    if f32_coords:      # MUTANT: the coordinates rounded before the difference
        dx = h[:, None, 0].astype(F32) - data.sta_x.astype(F32)[None, :]
        dy = h[:, None, 1].astype(F32) - data.sta_y.astype(F32)[None, :]
        dz = h[:, None, 2].astype(F32) - data.sta_z.astype(F32)[None, :]
    else:
        dx = (h[:, None, 0] - data.sta_x.astype(f64)[None, :]).astype(F32)
        dy = (h[:, None, 1] - data.sta_y.astype(f64)[None, :]).astype(F32)
        dz = (h[:, None, 2] - data.sta_z.astype(f64)[None, :]).astype(F32)
    d = moved(np.sqrt(_fma32(dz, dz, _fma32(dy, dy, dx * dx))))
    if sqrt_bias:       # MUTANT: a sqrt that is systematically 4 ulp high
        d = _move(d, 4)
    rbeta = f64(1.0) / f64(vs)
    katt = (f64(np.pi) * f64(5.0)) / (f64(qs) * f64(vs))
    tc32, ac32 = np.asarray(t_corr, dtype=f64).astype(F32), np.asarray(a_corr, dtype=f64).astype(F32)
    if neighbour_corr:  # MUTANT: station j with the corrections of station j - 1
        tc32, ac32 = np.roll(tc32, 1), np.roll(ac32, 1)
    ts = _fma32(d, np.broadcast_to(F32(rbeta), d.shape), np.broadcast_to(-tc32[None, :], d.shape)).astype(f64)
    l2 = moved(np.log2(d.astype(LD)).astype(F32))
    lg = _fma32(l2, np.broadcast_to(F32(0.69314718055994531), d.shape), np.broadcast_to(ac32[None, :], d.shape))
    am = _fma32(-d, np.broadcast_to(F32(katt), d.shape), -lg).astype(f64)
    t64 = restate_tables(data.t_stdv, data.a_stdv, f64)
    log_2pi_half = 0.5 * np.log(2.0 * np.arccos(-1.0))
    L_ev = np.zeros(E, f64)
    for use, k, syn in ((use_time, "t", ts), (use_amp, "a", am)):
        if use:
            obs = getattr(data, k + "_obs").astype(F32).astype(f64)
            prec = t64[k + "_prec"].astype(F32).astype(f64)
            rps = 1.0 / np.sum(t64[k + "_prec"], axis=1)
            mean = np.sum(prec * (syn - obs), axis=1) * rps
            r = obs - (syn - mean[:, None])
            L_ev = L_ev - 0.5 * np.sum(r * r * prec, axis=1) - np.sum(log_2pi_half + t64["log_" + k], axis=1)
    return float(np.sum(L_ev)), L_ev


def bound(D32, M, ulps=None):
    return (ULPS32 if ulps is None else ulps) * U32 * float(D32) + ULPS_L * EPS * float(M)


def units(err, D32):
    """|error| in 2^-24 D32 (0 where D32 vanishes -- one station: the fp64 share of the bound is what is left)"""
    return float(abs(err)) / (U32 * float(D32)) if float(D32) > 0.0 else 0.0


# ---- the cases ------------------------------------------------------------------------------------------------------------
PAIR_S = (2, 64, 65, 127, 128)
LIVE_SD, MUTE_SD = 2.0 ** -6, 2.0 ** 20
RAGGED = [(E, S) for S in (1, 2, 3, 63, 64, 65, 100, 127, 128) for E in (1, 5, 37)] + [(1001, 64), (4099, 70)]
N_MODELS = 5


def T1_is_meetable(data, use_time, use_amp, *m):
    """tests/test_gpu_fp32.py T1 measures the error in |L|, and L can cancel: with amplitudes only the misfits' sum stands against
    the constants' (-log stdv - log sqrt(2 pi) > 0 per entry), and one model of 37 x 5 drawn here had |L| = 0.007 M, where the
    correctly rounded float32 arithmetic sits at 1.7e-5 |L| -- no kernel can meet T1 there.  The ragged cases are held to T1 as
    well as to T7, so a model of theirs is drawn again until the documented arithmetic itself (emulate, sqrt and log2 correctly
    rounded) is within half of T1's 3e-6 |L| of the fp64 restatement.  A property of the reference's numbers alone."""
    L64 = restate_log_likelihood(data, use_time, use_amp, *m)[0]
    return float(abs(LD(emulate(data, use_time, use_amp, *m)[0]) - L64)) <= 1.5e-6 * float(abs(L64))


def live_stations(S):
    return sorted({j for j in (0, 63, 64, S - 1) if j < S})


def live_pairs(S, E=3):
    """event i -> its two live stations: neighbours in live_stations, so that every one of them is live somewhere"""
    live = live_stations(S)
    return [(live[i % len(live)], live[(i + 1) % len(live)]) for i in range(E)]


def cases():
    """(kind, E, S, mode, shift) of sections C and D: what ULPS32 was measured over, what the GPU tests run"""
    out = [("pair", 3, S, mode, 0.0) for S in PAIR_S for mode in MODES]
    out += [("grid", E, S, "both", K) for (E, S) in ((5, 63), (3, 128)) for K in (0.0,) + SHIFTS]
    out += [("ragged", E, S, "both", 0.0) for (E, S) in RAGGED]
    out += [("ragged", 37, S, mode, 0.0) for S in (5, 65, 127) for mode in MODES if mode != "both" or (37, S) not in RAGGED]
    return out


def case_id(c):
    kind, E, S, mode, K = c
    return "%s-%dx%d-%s%s" % (kind, E, S, mode.replace(" ", "-"), "-shift2^%d" % int(np.log2(K)) if K else "")


def _snap(x):
    return np.round(np.asarray(x, dtype=np.float64) / GRID) * GRID


@functools.lru_cache(maxsize=None)
def build(c):
    """-> namespace(data, H, TC, VS, AC, QS: N_MODELS stacked models, moves: per model (event id, component, step) of its partial
    update).  Cached and shared: treat as read-only."""
    kind, E, S, mode, K = c
    data = synth.make_synthetic(E, S, seed=900 + 7 * E + S)
    rng = np.random.default_rng(E * 1000 + S + len(mode) + (11 if kind == "pair" else 0))
    on_grid = kind == "grid" or K != 0.0
    if kind == "ragged":
        data = with_missing(data)
    if kind == "pair":
        for k in ("t_stdv", "a_stdv"):
            sd = np.full((E, S), MUTE_SD)
            for i, pair in enumerate(live_pairs(S, E)):
                sd[i, list(pair)] = LIVE_SD
            setattr(data, k, sd)
        data.t_obs, data.a_obs = data.t_obs.astype(F32).astype(np.float64), data.a_obs.astype(F32).astype(np.float64)
    if on_grid:
        data.sta_x, data.sta_y, data.sta_z, data.ev_xyz = _snap(data.sta_x), _snap(data.sta_y), _snap(data.sta_z), _snap(data.ev_xyz)
    n = N_MODELS
    H, TC, AC, VS, QS = np.empty((n, E, 3)), np.empty((n, S)), np.empty((n, S)), np.empty(n), np.empty(n)
    for k in range(n):
        for _ in range(50):
            H[k] = data.ev_xyz + rng.normal(0, 1.0, data.ev_xyz.shape)
            H[k, :, 2] = np.abs(H[k, :, 2]) + 0.5
            TC[k], AC[k], VS[k], QS[k] = rng.normal(0, 0.2, S), rng.normal(0, 0.02, S), 3 + rng.normal(0, 0.2), 250 + rng.normal(0, 30)
            if kind != "ragged" or T1_is_meetable(data, *MODES[mode], H[k].reshape(-1), TC[k], VS[k], AC[k], QS[k]):
                break
        else:
            raise AssertionError("no model of %s with a log-likelihood that does not cancel" % (c,))
    moves = [((k % E) + 1, k % 3, STEP if on_grid else 0.4) for k in range(n)]
    if kind == "pair":
        # model 1: the first event 1 m from its first live station (small d, large |ln d|); its partial update starts there
        j = live_pairs(S, E)[0][0]
        H[1, 0] = np.array([data.sta_x[j], data.sta_y[j], data.sta_z[j]]) + np.array([6e-4, -6e-4, 5e-4])
        moves[1] = (1, 0, 0.4)
        # model 2: corrections of +-5 s and +-1, so that their conversions to float carry weight
        TC[2] = 5.0 * rng.choice([-1.0, 1.0], S); AC[2] = rng.choice([-1.0, 1.0], S)
    if on_grid:
        H = _snap(H)
    if K:
        data.sta_x, data.sta_y = data.sta_x + K, data.sta_y + K
        data.ev_xyz = data.ev_xyz + np.array([K, K, 0.0])
        H = H + np.array([K, K, 0.0])
    for a in (data.sta_x, data.sta_y, data.sta_z, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv, H, TC, VS, AC, QS):
        a.setflags(write=False)
    return SimpleNamespace(data=data, H=H.reshape(n, -1), TC=TC, VS=VS, AC=AC, QS=QS, moves=moves, mode=MODES[mode])


def moved_model(cs, k):
    """(event id, hypocentres after the partial update of model k)"""
    evt, cmp_, step = cs.moves[k]
    h2 = cs.H[k].copy()
    h2[3 * (evt - 1) + cmp_] += step
    return evt, h2


@functools.lru_cache(maxsize=None)
def references(c):
    """per model of build(c): (reference at the model, reference at its moved model); cached, shared by the tests"""
    cs = build(c)
    ut, ua = cs.mode
    out = []
    for k in range(N_MODELS):
        evt, h2 = moved_model(cs, k)
        out.append((reference(cs.data, ut, ua, cs.H[k], cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k]),
                    reference(cs.data, ut, ua, h2, cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k])))
    return out


def partial_reference(c, k):
    """the one-event difference L_new - L_old of model k's partial update and the D32 and M it is judged on (both positions)"""
    evt, _ = moved_model(build(c), k)
    r0, r1 = references(c)[k]
    e = evt - 1
    return r1.L_ev[e] - r0.L_ev[e], r0.D32_ev[e] + r1.D32_ev[e], r0.M_ev[e] + r1.M_ev[e]
