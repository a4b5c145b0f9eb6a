"""GPU: the fp32-forward / fp64-accept mode term by term (T7), under exact translations (T8), at ragged shapes (T9) and through its
switch, at call level: calc_log_likelihood, calc_log_likelihood_batch and partially_update_log_likelihood of handles with
forward_precision = fp32 against tests/fp32_restatement.py -- `reference`, the mode's definition in numpy.longdouble on the inputs as
the library stores them -- at

    |L_gpu - L_ref| <= ULPS32 * 2^-24 * D32 + 16 * 2^-53 * M        (T7; ULPS32, D32, M: tests/fp32_restatement.py)

The cases are that module's cases(), the ones ULPS32 was measured over on the CPU: pair probes (an event's weight on two stations,
so that L resolves single synthetics; live stations at 0, 63, 64 and S - 1 of S = 2, 64, 65, 127, 128; a model 1 m from a live
station, one with corrections of +-5 s and +-1), coordinates on a 2^-16 km grid shifted by 2^12 and 2^20 km, every chunk shape of
n_sta <= 128 with 1, 5 and 37 events (a last event tile with three idle waves), 1001 x 64 and 4099 x 70 (two events per wave), and
the single-type modes with missing entries.  A one-event difference is judged on the one-event D32 and M of both positions, plus the
rounding of the old value it is added to (16 * 2^-53 * M of the full value).  Every case appends its worst ratio
|L_gpu - L_ref| / (2^-24 D32) to the file of measured tolerances that tests/test_gpu_fp32.py keeps (its _note)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import fp32_restatement as R
from tests.test_forward_data_modes import LD
from tests.test_gpu_fast_master import RTOL_FP32
from tests.test_gpu_forward import RTOL_L
from tests.test_gpu_fp32 import _note

pytestmark = pytest.mark.gpu


def _handle(cs, prec):
    from hypotremormcmc_amd.forward import Forward
    from hypotremormcmc_amd.obs_data import ObsData

    d = cs.data
    obs = ObsData.from_arrays(d.sta_x, d.sta_y, d.t_obs, d.t_stdv, d.a_obs, d.a_stdv)
    f = Forward(n_sta=d.n_sta, n_events=d.n_events, sta_x=d.sta_x, sta_y=d.sta_y, sta_z=d.sta_z, obs=obs, use_time=cs.mode[0],
                use_amp=cs.mode[1], forward_precision=prec)
    assert f.forward_precision == prec
    return f


def _evaluate(f, cs, L_old):
    """every value the three entry points give on the case's five models: (full one by one, partial updates); the stacked calls
    (n = 2, 5) must give the bits of the calls one by one"""
    n = R.N_MODELS
    full = np.array([f.calc_log_likelihood(cs.H[k], cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k]) for k in range(n)])
    for m in (2, n):
        Lb = f.calc_log_likelihood_batch(cs.H[:m], cs.TC[:m], cs.VS[:m], cs.AC[:m], cs.QS[:m])
        assert np.array_equal(Lb, full[:m]), "stacked models differ from one by one"
    part = np.empty(n)
    for k in range(n):
        evt, h2 = R.moved_model(cs, k)
        part[k] = f.partially_update_log_likelihood(evt, cs.H[k], L_old[k], h2, cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k])
    assert np.all(np.isfinite(full)) and np.all(np.isfinite(part))
    return full, part


def _old_values(c):
    return np.array([float(r0.L) for r0, _ in R.references(c)])


@pytest.mark.parametrize("c", R.cases(), ids=R.case_id)
def test_fp32_values_against_the_longdouble_reference(c):
    """T7 on every case; T9: the ragged shapes also at T1 against the fp64 oracle; one station: the misfit vanishes"""
    kind, E, S, mode, K = c
    cs = R.build(c)
    refs, L_old = R.references(c), _old_values(c)
    f = _handle(cs, "fp32")
    full, part = _evaluate(f, cs, L_old)
    assert f.obs_pack_bytes() == 0
    worst_f = worst_p = worst_m = 0.0
    for k in range(R.N_MODELS):
        r0, _ = refs[k]
        err = float(abs(LD(full[k]) - r0.L))
        worst_f, worst_m = max(worst_f, R.units(err, r0.D32)), max(worst_m, err / (R.EPS * float(r0.M)))
        assert err <= R.bound(r0.D32, r0.M), "full, model %d: %.3f in 2^-24 D32" % (k, R.units(err, r0.D32))
        dref, D, M = R.partial_reference(c, k)
        err = float(abs(LD(part[k]) - LD(L_old[k]) - dref))
        worst_p = max(worst_p, R.units(err, D))
        assert err <= R.bound(D, M) + R.bound(0, r0.M), "partial, model %d: %.3f in 2^-24 D32" % (k, R.units(err, D))
    if S == 1:
        # the one entry's weighted mean is the entry: no residual, L is the constants' sum
        _note("T7 %s: one station, |L_gpu - L_ref| / (2^-53 M) = %.2f" % (R.case_id(c), worst_m))
        const = R.constants_sum(cs.data, *cs.mode)
        for k in range(R.N_MODELS):
            assert float(abs(LD(full[k]) - const)) <= R.bound(0, refs[k][0].M), (full[k], float(const))
    else:
        _note("T7 %s: |L_gpu - L_ref| / (2^-24 D32) = %.3f (full) %.3f (one-event difference)" % (R.case_id(c), worst_f, worst_p))
    if kind == "ragged":
        from oracle import oracle

        d = cs.data
        orc = oracle.Forward(d.sta_x, d.sta_y, d.sta_z, d.t_obs, d.t_stdv, d.a_obs, d.a_stdv, *cs.mode)
        for k in range(R.N_MODELS):
            Lo = orc.calc_log_likelihood(cs.H[k], cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k])
            assert abs(full[k] - Lo) <= RTOL_FP32 * abs(Lo)
            evt, h2 = R.moved_model(cs, k)
            Po = orc.partially_update_log_likelihood(evt, cs.H[k], L_old[k], h2, cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k])
            assert abs(part[k] - Po) <= RTOL_FP32 * abs(Po)
    f.close()


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", [(5, 63), (3, 128)])
def test_exact_translations_leave_every_bit(shape, prec):
    """T8: stations and hypocentres on a 2^-16 km grid, x and y of all of them shifted by 2^12 and 2^20 km: the fp64 coordinate
    differences are the same numbers, and nothing else of a coordinate may reach the result -- in either precision"""
    E, S = shape
    base = ("grid", E, S, "both", 0.0)
    L_old = _old_values(base)
    cs0 = R.build(base)
    f0 = _handle(cs0, prec)
    want = _evaluate(f0, cs0, L_old)
    f0.close()
    for K in R.SHIFTS:
        cs = R.build(base[:4] + (K,))
        assert np.array_equal(cs.data.sta_x - K, cs0.data.sta_x) and np.array_equal(cs.H.reshape(-1, 3)[:, 1] - K, cs0.H.reshape(-1, 3)[:, 1])
        f = _handle(cs, prec)
        got = _evaluate(f, cs, L_old)
        f.close()
        assert np.array_equal(got[0], want[0]), "full evaluations, shift %g km" % K
        assert np.array_equal(got[1], want[1]), "partial updates, shift %g km" % K
    _note("T8 %dx%d %s: full, stacked and partial values bit-equal under shifts of 2^12 and 2^20 km" % (E, S, prec))


def test_fp32_is_refused_above_128_stations_and_the_handle_stays_usable():
    from hypotremormcmc_amd import synth
    from hypotremormcmc_amd._lib import HtmError
    from oracle import oracle

    from tests.test_forward_data_modes import model

    d = synth.make_synthetic(3, 129, seed=129)
    cs = SimpleNamespace(data=d, mode=(True, True))
    f = _handle(cs, "fp64")
    orc = oracle.Forward(d.sta_x, d.sta_y, d.sta_z, d.t_obs, d.t_stdv, d.a_obs, d.a_stdv, True, True)
    m = model(d, np.random.default_rng(129))
    Lo = orc.calc_log_likelihood(*m)
    assert abs(f.calc_log_likelihood(*m) - Lo) <= RTOL_L * abs(Lo)
    with pytest.raises(HtmError, match="128"):
        f.set_precision("fp32")
    assert f.forward_precision == "fp64" and f.obs_pack_bytes() == 0
    assert abs(f.calc_log_likelihood(*m) - Lo) <= RTOL_L * abs(Lo)
    h2 = m[0].copy(); h2[4] += 0.4
    Po = orc.partially_update_log_likelihood(2, m[0], Lo, h2, *m[1:])
    assert abs(f.partially_update_log_likelihood(2, m[0], Lo, h2, *m[1:]) - Po) <= RTOL_L * abs(Po)
    f.close()


def test_switching_fp32_fp64_fp32_gives_the_bits_of_a_fresh_handle():
    c = ("ragged", 5, 65, "both", 0.0)
    cs, L_old = R.build(c), _old_values(c)
    fresh = {}
    for prec in ("fp32", "fp64"):
        f = _handle(cs, prec)
        fresh[prec] = _evaluate(f, cs, L_old)
        assert f.obs_pack_bytes() == 0
        f.close()
    assert not np.array_equal(fresh["fp32"][0], fresh["fp64"][0])
    f = _handle(cs, "fp32")
    for prec in ("fp32", "fp64", "fp32", "fp64"):
        f.set_precision(prec)
        assert f.forward_precision == prec and f.obs_pack_bytes() == 0
        got = _evaluate(f, cs, L_old)
        assert np.array_equal(got[0], fresh[prec][0]) and np.array_equal(got[1], fresh[prec][1]), "after switching to " + prec
    f.close()
