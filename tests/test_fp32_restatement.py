"""CPU: the restatement of the fp32-forward mode (tests/fp32_restatement.py) against itself -- the definition equals the fp64
restatement where nothing is rounded, the documented arithmetic meets the tolerance on every case the GPU tests run, and the
tolerance bites: three kernels that are subtly wrong exceed it.  No GPU value enters here; ULPS32 comes from these numbers."""
import numpy as np
import pytest

from hypotremormcmc_amd import synth
from tests import fp32_restatement as R
from tests.helpers import with_missing
from tests.test_forward_data_modes import LD, MODES, model, restate_log_likelihood


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(9, 70), (5, 3)])
def test_reference_without_rounding_is_the_fp64_restatement(shape, mode):
    """uneven standard deviations (0.07, 0.13 and the generator's), missing entries: L and M bit for bit"""
    E, S = shape
    ut, ua = MODES[mode]
    data = synth.make_synthetic(E, S, seed=41 + S)
    data.t_stdv[:, ::2] = 0.07; data.a_stdv[:, 1::3] = 0.13; data.t_stdv[0, :] = 0.13
    data = with_missing(data)
    rng = np.random.default_rng(S)
    for _ in range(3):
        m = model(data, rng)
        L, mag, _ = restate_log_likelihood(data, ut, ua, *m)
        ref = R.reference(data, ut, ua, *m, round_inputs=False)
        assert ref.L == L and ref.M == mag
        assert float(abs(np.sum(ref.L_ev) - L)) <= 4 * 2.0 ** -64 * float(mag) and float(ref.D32) > 0
        # rounding the stored inputs moves L by about u = 2^-24 of its terms, and not by more
        rounded = R.reference(data, ut, ua, *m)
        assert 0 < float(abs(rounded.L - L)) <= 8 * R.U32 * float(mag + ref.D32)


def _worst(c, **kw):
    """emulate against reference over the five models of a case, full values and one-event differences: the worst error beyond the
    fp64 share 16 eps M, in 2^-24 D32"""
    cs = R.build(c)
    ut, ua = cs.mode
    w = 0.0
    for k in range(R.N_MODELS):
        r0, _ = R.references(c)[k]
        L, L_ev = R.emulate(cs.data, ut, ua, cs.H[k], cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k], **dict(kw, seed=k))
        evt, h2 = R.moved_model(cs, k)
        _, L_ev2 = R.emulate(cs.data, ut, ua, h2, cs.TC[k], cs.VS[k], cs.AC[k], cs.QS[k], **dict(kw, seed=100 + k))
        w = max(w, R.units(max(0.0, float(abs(LD(L) - r0.L)) - R.bound(0, r0.M)), r0.D32))
        dref, D, M = R.partial_reference(c, k)
        w = max(w, R.units(max(0.0, float(abs(LD(L_ev2[evt - 1]) - LD(L_ev[evt - 1]) - dref)) - R.bound(0, M)), D))
    return w


@pytest.mark.parametrize("c", R.cases(), ids=R.case_id)
def test_documented_arithmetic_meets_the_tolerance(c):
    """the condition that the reference alone meets T7: float32 arithmetic as htm_device.hpp documents it, its sqrt and log2 correctly
    rounded or moved by an ulp (seeded, or one sign everywhere), stays within ULPS32.  These are the numbers ULPS32 was set from
    (the module's docstring)."""
    w = {n: _worst(c, nudge=n) for n in R.NUDGES}
    print(R.case_id(c), " ".join("%s: %.3f" % kv for kv in w.items()))
    assert max(w.values()) <= R.ULPS32


def _pairs(with_station_64=False, modes=MODES):
    return [c for c in R.cases() if c[0] == "pair" and c[3] in modes and (not with_station_64 or 64 in R.live_stations(c[2]))]


def test_coordinates_rounded_before_the_difference_exceed_the_bound():
    """`coordinate differences stay fp64` (htm_device.hpp event_misfit): a kernel that rounds the coordinates first is caught on
    EVERY pair probe at both offsets of the translation tests (real station coordinates are projected kilometres)"""
    for c in _pairs():
        for K in R.SHIFTS:
            shifted = c[:4] + (K,)
            assert _worst(shifted) <= R.ULPS32, "the clean arithmetic does not see the offset"
            w = _worst(shifted, f32_coords=True)
            print(R.case_id(shifted), "f32_coords: %.1f" % w)
            assert w > R.ULPS32


def test_a_square_root_four_ulp_high_exceeds_the_bound():
    """a systematic 4 ulp: caught where the travel times carry the weight of two stations -- on most time-only pair probes (5.2,
    5.7, 7.5, 4.1 at S = 2, 64, 65, 127; 3.8 at 128) and some with both types (6.3, 5.4 at S = 64, 65).  At 37 x 64 with both
    types it reaches 2.6: 64 stations' demeaning absorbs what is common to them, and a sqrt that is 1 ulp off with one sign
    (which the hardware's may be) reaches 1.6 at the ragged shapes -- the probes separate the two, 37 x 64 does not."""
    w37 = _worst(("ragged", 37, 64, "both", 0.0), sqrt_bias=True)
    print("ragged-37x64-both sqrt_bias: %.2f" % w37)
    assert w37 > 2.0
    caught = 0
    for c in _pairs(modes=("time only",)):
        w = _worst(c, sqrt_bias=True)
        print(R.case_id(c), "sqrt_bias: %.2f" % w)
        caught += w > R.ULPS32
    assert caught >= 3


def test_a_neighbours_correction_exceeds_the_bound():
    """station j with the corrections of station j - 1 (an off-by-one in the second chunk's loads): on every probe whose live
    stations include j = 64, in each data mode"""
    probes = _pairs(with_station_64=True)
    assert len(probes) == 9
    for c in probes:
        w = _worst(c, neighbour_corr=True)
        print(R.case_id(c), "neighbour_corr: %.0f" % w)
        assert w > 100 * R.ULPS32


def test_T1_passes_coordinates_rounded_to_float():
    """why the u * D32 scale exists: tests/test_gpu_fp32.py T1, |L32 - L64| <= 3e-6 |L64|, passes the f32_coords mutant at 37 x 64
    with every coordinate offset by 500 km -- |L| is not what the error scales with.  Five models 1 km from the truth: the mutant
    sits at 3.3e-7 .. 1.2e-6 |L| in four of them (the clean arithmetic: 7e-8 .. 9e-7) and at 3.6e-6 in one; other data sets of
    the generator give the same picture (one or two models in five between 3e-6 and 5.5e-6, the rest below).  So T1 lets the
    mutant through for most models and stops it for some by the luck of the draw.  With 64 stations sharing the weight it stays
    below this module's bound too (0.7); the pair probes, shifted as real coordinates are, see it at 45 and more (above)."""
    data = synth.make_synthetic(37, 64, seed=101)
    rng = np.random.default_rng(37064)
    data.sta_x, data.sta_y = data.sta_x + 500.0, data.sta_y + 500.0
    data.ev_xyz = data.ev_xyz + np.array([500.0, 500.0, 0.0])
    t1, t7 = [], []
    for _ in range(5):
        m = model(data, rng)
        L64, _, _ = restate_log_likelihood(data, True, True, *m)
        ref = R.reference(data, True, True, *m)
        Lm, _ = R.emulate(data, True, True, *m, f32_coords=True)
        Lc, _ = R.emulate(data, True, True, *m)
        t1.append(float(abs(LD(Lm) - L64) / abs(L64)))
        t7.append(R.units(float(abs(LD(Lm) - ref.L)), ref.D32))
        assert float(abs(LD(Lc) - ref.L)) <= R.bound(ref.D32, ref.M) and float(abs(LD(Lc) - L64)) <= 3e-6 * float(abs(L64))
    print("f32_coords at 37 x 64, 500 km: |L| units (T1: 3e-6)", " ".join("%.2e" % v for v in t1), "; 2^-24 D32:", " ".join("%.2f" % v for v in t7))
    assert sum(v <= 3e-6 for v in t1) >= 4, "T1 passes the mutant for four models in five"
