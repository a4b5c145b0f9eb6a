"""Steps 2 and 3 (hypotremormcmc_amd.correlate / .measure) without a GPU: the numpy restatement of the reference
(tests/xcorr_restatement.py) against a direct sum, the file formats of src/cls_correlator.f90:246-251 and
src/hypo_tremor_correlate.f90:71-86, the parameter rules of src/cls_param.f90:117-122 and the detection rule of
src/cls_measurer.f90:238-271."""
import math
import os

import numpy as np
import pytest

from hypotremormcmc_amd import correlate as corr, measure, synth
from hypotremormcmc_amd.obs_data import ObsData
from hypotremormcmc_amd.param import Param, ParamError
from hypotremormcmc_amd.select import read_detected_win

from . import helpers, xcorr_restatement as rs


def test_restatement_fft_equals_direct_sum():
    rng = np.random.default_rng(1)
    for n in (2, 10, 64, 300):
        a, b = rs.prep_correlate(rng.random(n)), rs.prep_correlate(rng.random(n))
        np.testing.assert_allclose(rs.circ_fft(a, b), rs.circ_direct(a, b), rtol=0, atol=1e-13)


def test_taper_formula():
    x = np.ones(300)
    y = rs.taper(x)
    nleng = 15
    for i in range(1, nleng + 1):
        f = 0.5 * (1 - math.cos((i - 1) * math.pi / nleng))
        assert y[i - 1] == f and y[300 - i] == f
    assert np.all(y[nleng:300 - nleng] == 1.0)
    assert y[0] == 0.0 and y[-1] == 0.0
    assert np.array_equal(rs.taper(np.arange(10.0)), np.arange(10.0))    # nleng = int(0.5) = 0: no taper


@pytest.mark.parametrize("n_smp,n,n_step,want", [(50, 100, 30, 0), (99, 100, 1, 0), (1000, 100, 50, 18),
                                                 (1000, 100, 100, 9), (1000, 100, 150, 6), (100, 100, 7, 0),
                                                 (101, 100, 1, 1)])
def test_window_count(n_smp, n, n_step, want):
    assert corr.window_count(n_smp, n, n_step) == want


def test_nint_rounds_half_away_from_zero():
    assert corr.nint(2.5) == 3 and corr.nint(-2.5) == -3 and corr.nint(0.49) == 0 and corr.nint(299.9999) == 300


def _write_env(path, times, amps, extra=None):
    rec = np.empty((times.size, 2))
    rec[:, 0], rec[:, 1] = times, amps
    v = rec.ravel()
    if extra is not None:
        v = np.append(v, extra)
    v.astype("<f8").tofile(path)


def test_env_reader_dt_rules_and_odd_tail(tmp_path):
    t = np.array([0.0, 1.0, 2.0, 3.5])
    p = str(tmp_path / "A.merged.env")
    _write_env(p, t, np.arange(4.0), extra=99.0)
    tt, aa = corr.read_env(p)
    assert np.array_equal(tt, t) and np.array_equal(aa, np.arange(4.0))
    assert corr.env_dt(tt) == 1.5                   # step 2: the last two times
    assert measure.envelope_dt(p) == 1.0             # step 3: record 3 - record 1 (times 1 and 2)
    _write_env(p, np.array([4.0]), np.array([1.0]))
    assert corr.env_dt(corr.read_env(p)[0]) == 4.0   # one sample: t - 0


def test_corr_writers_layout_and_roundtrip(tmp_path):
    n, n_win, dt, t_step, t_win = 6, 3, 0.5, 1.25, 3.0
    cc = np.arange(n_win * n, dtype=np.float64).reshape(n_win, n) / 7.0
    p, q = str(tmp_path / "A.B.corr"), str(tmp_path / "A.B.max_corr")
    corr.write_corr(p, cc, n, dt, t_step, t_win)
    corr.write_max_corr(q, cc.max(axis=1), t_step, t_win)
    assert os.path.getsize(p) == 24 * n * n_win and os.path.getsize(q) == 16 * n_win
    v = corr.read_corr(p)
    for i in range(1, n_win + 1):
        for j in range(1, n + 1):
            row = v[(i - 1) * n + j - 1]
            assert row[0] == (i - 1) * t_step + 0.5 * t_win
            assert row[1] == (j - n // 2 - 1) * dt
            assert row[2] == cc[i - 1, j - 1]
    m = corr.read_max_corr(q)
    assert np.array_equal(m[:, 1], cc.max(axis=1)) and m[0, 0] == 0.5 * t_win


def _param(tmp_path, **kv):
    (tmp_path / "sta.list").write_text("A 0 0 0 1 1\nB 1 0 0 1 1\nC 0 1 0 1 1\n")
    p = tmp_path / "p.in"
    p.write_text("".join(f"{k} = {v}\n" for k, v in dict(station_file="sta.list", **kv).items()))
    return str(p)


def test_required_keys(tmp_path):
    with pytest.raises(ParamError, match="t_step_corr"):
        Param(_param(tmp_path, n_procs=1, t_win_corr=300), from_where="correlate")
    Param(_param(tmp_path, n_procs=1, t_win_corr=300, t_step_corr=150), from_where="correlate")
    with pytest.raises(ParamError, match="n_pair_thred"):
        Param(_param(tmp_path, n_procs=1, alpha=0.9), from_where="measure")
    para = Param(_param(tmp_path, n_procs=1, alpha=0.9, n_pair_thred=3), from_where="measure")
    with pytest.raises(ParamError, match="t_win_corr"):
        para.require("t_win_corr", "t_step_corr")
    Param(_param(tmp_path, n_procs=1), from_where="select_is_not_checked_here")      # unknown programs: no list


def test_threshold_rank_refuses_zero():
    assert measure.threshold_rank(300, 10, 0.5) == 1500
    with pytest.raises(SystemExit, match="rank"):
        measure.threshold_rank(300, 10, 1.0 / 3001.0)
    v = np.random.default_rng(0).random(3000)
    assert rs.threshold(v, 0.99) == np.sort(v)[measure.threshold_rank(300, 10, 0.99) - 1]


def test_detection_is_strictly_more_than_n_pair_thred():
    cc_max = np.array([[0.9, 0.9, 0.1], [0.9, 0.9, 0.9], [0.5, 0.49, 0.5]])
    thred = np.array([0.5, 0.5, 0.5])
    assert measure.detect(cc_max, thred, 2) == [2]            # windows 1 and 3: exactly 2 detecting pairs
    assert measure.detect(cc_max, thred, 1) == [1, 2, 3]      # cc_max == threshold detects (window 3)
    assert measure.detect(cc_max, thred, 3) == []


def test_outputs_readable_by_steps_4_and_5(tmp_path):
    os.chdir(tmp_path)
    measure.write_detected_win([3, 7], 150.0, 300.0)
    ids, times = read_detected_win()
    assert ids == [3, 7] and times == [450.0, 1050.0]
    t = np.array([[0.5, -0.25, -0.25]]); ts = np.array([[1.0, 2.0, 3.0]])
    a = np.array([[0.1, 0.2, -0.3]]); asd = np.array([[0.01, 0.02, 0.03]])
    sx, sy, sz = np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.zeros(3)
    measure.write_opt_data([7], sx, sy, sz, t, ts, a, asd)
    obs = ObsData([7], 3, sx, sy)
    assert np.array_equal(obs.get_t_obs(), t) and np.array_equal(obs.get_t_stdv(), ts)
    assert np.array_equal(obs.get_a_obs(), a) and np.array_equal(obs.get_a_stdv(), asd)
    measure.write_cc_thred([("A", "B")], [0.25])
    assert open("cc_thred.dat").read().split() == ["A", "B", "0.25"]


def test_synthetic_envelopes_files(tmp_path):
    env = synth.make_tremor_envelopes(4, 12, 100, 50, [3, 8], [0, 2, -1, 3], [0.0, 0.5, -0.5, 0.2])
    pf = synth.write_envelopes(str(tmp_path), env, t_step_corr=50.0)
    para = Param(pf, from_where="correlate")
    assert para.stations == env.stations
    t, a = corr.read_env(os.path.join(str(tmp_path), env.stations[1] + ".merged.env"))
    assert np.array_equal(a, env.amps[1]) and corr.env_dt(t) == 1.0
    n, n_step, n_win = corr.geometry(para.values["t_win_corr"], para.values["t_step_corr"], 1.0, a.size)
    assert (n, n_step, n_win) == (100, 50, 12)
    # noise-free: station 1's burst is station 0's shifted by 2 samples and scaled by e^0.5
    c = (3 - 1) * 50 + 50
    assert env.amps[1][c + 2] - 1.0 == pytest.approx(10.0 * math.exp(0.5))
    assert np.argmax(env.amps[3][c - 20:c + 20]) == 20 + 3


# ---- pinned to the compiled reference (tests/golden/xcorr_*.npz, written by the unmodified steps 2 and 3 linked with
# the FFT stand-in oracle/ref_dft.c; make_golden.py)

@pytest.mark.parametrize("n", [1, 2, 3, 10, 31, 64, 300])
def test_reference_fft_stand_in_equals_numpy(n):
    from oracle import oracle

    x = np.random.default_rng(n).standard_normal(n)
    X = oracle.ref_dft_r2c(x)
    np.testing.assert_allclose(X, np.fft.rfft(x), rtol=0, atol=1e-13 * max(1, n))
    # c2r: unnormalised, the imaginary parts of bin 0 and (n even) bin n/2 ignored
    c = np.fft.rfft(np.random.default_rng(n + 1).standard_normal(n))
    c[0] += 5j
    if n % 2 == 0:
        c[-1] += 7j
    y = oracle.ref_dft_c2r(c, n)
    want = np.fft.irfft(np.where(np.arange(c.size) == 0, c.real, c) if n % 2 else
                        np.where((np.arange(c.size) == 0) | (np.arange(c.size) == n // 2), c.real, c), n) * n
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-13 * max(1, n))
    np.testing.assert_allclose(oracle.ref_dft_c2r(oracle.ref_dft_r2c(x), n), n * x, rtol=0, atol=1e-13 * n)


@pytest.mark.parametrize("case", helpers.XCORR_CASES)
def test_restatement_correlograms_equal_reference(case):
    fx, env, g = helpers.load_xcorr_case(case)
    n, n_step, n_win = g["n"], g["n_step"], g["n_win"]
    cc, cc_max = rs.correlate(env.amps, n, n_step, n_win)
    np.testing.assert_allclose(cc, fx["cc"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(cc_max, fx["cc_max"], rtol=0, atol=1e-13)
    assert np.array_equal(fx["cc_max"], fx["cc"].max(axis=2))


@pytest.mark.parametrize("case", helpers.XCORR_CASES)
def test_threshold_rank_and_detection_equal_reference(case):
    fx, env, g = helpers.load_xcorr_case(case)
    n, n_win, alpha = g["n"], g["n_win"], float(fx["alpha"])
    assert measure.threshold_rank(n, n_win, alpha) == int(fx["thred_rank"])
    # the threshold is the element of that rank among the reference's own .corr values, as cc_thred.dat prints it
    ref_cc = fx["cc"]
    for p in range(ref_cc.shape[1]):
        assert rs.threshold(ref_cc[:, p], alpha) == fx["thred"][p]
        assert np.sort(ref_cc[:, p].ravel())[measure.threshold_rank(n, n_win, alpha) - 1] == fx["thred"][p]
    assert np.all(np.abs(fx["thred_text"] - fx["thred"]) <= 2 * np.spacing(fx["thred"]))
    # detection on the reference's own cc_max and thresholds, then on the restatement's
    det = fx["detected"].tolist()
    assert measure.detect(fx["cc_max"], fx["thred"], int(fx["n_pair_thred"])) == det
    cc, cc_max = rs.correlate(env.amps, n, g["n_step"], n_win)
    thr = [rs.threshold(cc[:, p], alpha) for p in range(cc.shape[1])]
    np.testing.assert_allclose(thr, fx["thred"], rtol=0, atol=1e-13)
    assert measure.detect(cc_max, thr, int(fx["n_pair_thred"])) == det
    t_win, t_step = n * g["dt"], g["n_step"] * g["dt"]
    assert [(w - 1) * t_step + 0.5 * t_win for w in det] == fx["detected_time"].tolist()


@pytest.mark.parametrize("case", helpers.XCORR_CASES)
def test_restatement_measurements_equal_reference(case):
    fx, env, g = helpers.load_xcorr_case(case)
    det = fx["detected"].tolist()
    x = measure.gather_windows(list(env.amps), det, g["n"], g["n_step"])
    S = g["n_sta"]
    n_tied = 0
    for d in range(len(det)):
        rt, rts, ra, rasd, lag, gap = rs.measure(x[d], g["dt"])
        if np.any(np.triu(gap < 1e-12, 1)):          # a near-tied pair may pick another lag: counted, not compared
            n_tied += 1
            continue
        opt = fx["opt"][d]
        assert np.array_equal(opt[:, 3], rt), d
        assert np.array_equal(opt[:, 4], rts), d
        np.testing.assert_allclose(opt[:, 5], ra, rtol=1e-12, atol=0)
        np.testing.assert_allclose(opt[:, 6], rasd, rtol=1e-12, atol=0)
    assert n_tied == 0
    assert fx["opt"].shape == (len(det), S, 7)


@pytest.mark.parametrize("case", helpers.XCORR_CASES)
def test_corr_writers_reproduce_reference_files(case, tmp_path):
    """the .corr / .max_corr streams of the first pair, written from the reference's own values, are its bytes"""
    import hashlib

    fx, env, g = helpers.load_xcorr_case(case)
    n, dt = g["n"], g["dt"]
    p, q = str(tmp_path / "a.corr"), str(tmp_path / "a.max_corr")
    corr.write_corr(p, fx["cc"][:, 0], n, dt, g["n_step"] * dt, n * dt)
    corr.write_max_corr(q, fx["cc_max"][:, 0], g["n_step"] * dt, n * dt)
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == str(fx["corr0_sha256"])
    assert hashlib.sha256(open(q, "rb").read()).hexdigest() == str(fx["max_corr0_sha256"])


# ---- limits: ranks and launches that would wrap a 32-bit integer are refused, not wrapped

def test_threshold_rank_refuses_more_values_than_int_max():
    assert measure.threshold_rank(4096, 524287, 0.5) == 4096 * 524287 // 2          # 2^31 - 4096 values: fine
    with pytest.raises(SystemExit, match="exceed"):
        measure.threshold_rank(4096, 524288, 0.5)                                   # 2^31 values
    with pytest.raises(SystemExit, match="exceed"):
        measure.threshold_rank(4096, 60 * 24 * 366, 0.999)                          # a year of windows every 60 s
    with pytest.raises(ValueError, match="rank"):
        measure._thresholds_dev(None, 2 ** 32 + 7, 1, 2 ** 32 + 7, -1)


def test_batch_pairs_stays_below_one_launch():
    assert corr.xc_threads(2) == 64 and corr.xc_threads(66) == 128 and corr.xc_threads(4096) == 1024
    for n_win, n, mb in ((4000, 300, 512), (100000, 4096, 1e9), (2 ** 21, 4096, 1e12), (10, 2, 1e12)):
        b = corr.batch_pairs(n_win, n, mb)
        assert b >= 1
        assert b == 1 or n_win * b * corr.xc_threads(n) <= corr.MAX_WORK_ITEMS, (n_win, n, mb, b)
    assert corr.batch_pairs(2 ** 20, 4096, 1e12) == 3 and corr.batch_pairs(4000, 300, 512) == 512 * 2 ** 20 // (8 * 4000 * 301)


def test_c_abi_refuses_launches_and_selects_beyond_32_bits():
    """The guards answer HTM_EINVAL before any device call (device -1: without them the call would fail in the device
    selection, never in a launch with undersized buffers)."""
    import ctypes as C

    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    rk = (C.c_int * 3)(1, 2, 3)
    assert lib.htm_quantiles_dev(-1, p, 2 ** 31, 1, 1, rk, p, None) == -1
    assert b"n_mod" in lib.htm_last_error()
    q = buf.ctypes.data_as(_lib.dp)
    assert lib.htm_quantiles(-1, q, 2 ** 31, 1, rk, q) == -1
    assert b"n_mod" in lib.htm_last_error()
    # k_xcorr: 2^22 windows of 4096 samples (1024 work-items each) for one pair is 2^32 work-items: refused
    n, n_win = 4096, 2 ** 22
    n_smp = n_win - 1 + n
    assert lib.htm_xcorr_dev(-1, p, n_smp, n_smp, 2, n, 1, n_win, 0, 1, p, 1, p, None) == -1
    assert b"work-items" in lib.htm_last_error()
    # one window fewer fits in a launch: past the guard, the call fails at device -1
    lib.htm_xcorr_dev(-1, p, n_smp, n_smp, 2, n, 1, n_win - 1, 0, 1, p, 1, p, None)
    assert b"work-items" not in lib.htm_last_error() and b"device" in lib.htm_last_error().lower()
    # n = 66 runs 128 work-items per workgroup: 2^25 workgroups of it are 2^32
    n, n_win = 66, 2 ** 24
    n_smp = n_win - 1 + n
    assert lib.htm_xcorr_dev(-1, p, n_smp, n_smp, 3, n, 1, n_win, 0, 2, p, 2, p, None) == -1
    assert b"work-items" in lib.htm_last_error()
