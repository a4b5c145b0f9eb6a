"""Steps 2 and 3 on the GPU (`htm_xcorr`, `htm_measure_windows`, python -m hypotremormcmc_amd.correlate / .measure)
against the numpy restatement of the reference in tests/xcorr_restatement.py, and on synthetic tremor with known
delays and amplitudes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hypotremormcmc_amd import _lib, measure, synth
from hypotremormcmc_amd._lib import check, dp
from hypotremormcmc_amd.select import read_detected_win

from . import xcorr_restatement as rs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(dp)


def xcorr(amps, n, n_step, n_win, pair0=0, n_pairs=None):
    n_sta, n_smp = amps.shape
    n_pairs = n_sta * (n_sta - 1) // 2 - pair0 if n_pairs is None else n_pairs
    amps = np.ascontiguousarray(amps)
    cc = np.empty((n_win * n, n_pairs)); mx = np.empty((n_win, n_pairs))
    check(_lib.load().htm_xcorr(0, _p(amps), n_smp, n_sta, n, n_step, n_win, pair0, n_pairs, _p(cc), _p(mx)))
    return cc.reshape(n_win, n, n_pairs).transpose(0, 2, 1), mx


@pytest.mark.parametrize("n_sta,n,n_step,n_win", [(3, 10, 3, 7), (17, 300, 150, 4), (17, 300, 300, 3),
                                                  (64, 300, 100, 2), (3, 4096, 1000, 3), (5, 4096, 4096, 2)])
def test_correlograms_equal_restatement(n_sta, n, n_step, n_win):
    rng = np.random.default_rng(n_sta * 7 + n)
    amps = 1.0 + rng.random((n_sta, (n_win - 1) * n_step + n + 5))
    amps[n_sta - 1, :n] = 0.0                     # window 0 of the last station has zero energy: zeros
    cc, mx = xcorr(amps, n, n_step, n_win)
    ref, ref_mx = rs.correlate(amps, n, n_step, n_win)
    np.testing.assert_allclose(cc, ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(mx, ref_mx, rtol=0, atol=1e-12)
    p_last = [p for p, (i, j) in enumerate((i, j) for i in range(n_sta - 1) for j in range(i + 1, n_sta)) if j == n_sta - 1]
    assert np.all(cc[0, p_last] == 0.0) and np.all(mx[0, p_last] == 0.0)


def test_pair_ranges_and_negative_lags_first():
    n, d = 300, 7
    rng = np.random.default_rng(3)
    a = rng.random(n + 50)
    amps = np.stack([a, np.roll(a, d), rng.random(n + 50), rng.random(n + 50)])
    cc, mx = xcorr(amps, n, 50, 2)
    w = rs.prep_correlate(a[:n]); v = rs.prep_correlate(np.roll(a, d)[:n])
    assert int(np.argmax(rs.reference_order(rs.circ_direct(w, v)))) == int(np.argmax(cc[0, 0]))
    b = np.r_[np.zeros(100), np.hanning(40), np.zeros(160)]
    amps2 = np.stack([b, np.roll(b, d), np.roll(b, -d)])
    cc2, _ = xcorr(amps2, n, n, 1)
    assert int(np.argmax(cc2[0, 0])) == n // 2 + d       # pair (1,2): station 2 later by d -> lag +d
    assert int(np.argmax(cc2[0, 1])) == n // 2 - d       # pair (1,3): station 3 earlier by d -> lag -d
    # a sub-range of pairs gives the same columns as the full set
    sub, submx = xcorr(amps, n, 50, 2, pair0=2, n_pairs=3)
    assert np.array_equal(sub, cc[:, 2:5]) and np.array_equal(submx, mx[:, 2:5])


def test_xcorr_refuses_bad_shapes():
    lib = _lib.load()
    amps = np.ones((3, 100)); cc = np.empty(10000); mx = np.empty(100)
    assert lib.htm_xcorr(0, _p(amps), 100, 3, 11, 5, 2, 0, 3, _p(cc), _p(mx)) == -1      # odd n
    assert b"even" in lib.htm_last_error()
    big = np.ones((3, 5000)); cc2 = np.empty(3 * 4098); mx2 = np.empty(3)
    assert lib.htm_xcorr(0, _p(big), 5000, 3, 4098, 1, 1, 0, 3, _p(cc2), _p(mx2)) == -1   # n > 4096
    assert lib.htm_xcorr(0, _p(amps), 100, 3, 50, 30, 3, 0, 3, _p(cc), _p(mx)) == -1      # windows past the end
    assert lib.htm_xcorr(0, _p(amps), 100, 3, 50, 30, 2, 1, 3, _p(cc), _p(mx)) == -1      # pairs past the last


def _measure_vs_restatement(x, dt):
    t, ts, a, asd = measure.measure_windows(x, dt)
    n_pairs = n_tied = 0
    for d in range(x.shape[0]):
        rt, rts, ra, rasd, lag, gap = rs.measure(x[d], dt)
        S = x.shape[1]
        n_pairs += S * (S - 1) // 2
        # windows with a near-tied pair may pick another lag under other rounding: counted, not compared
        tied = np.argwhere(np.triu(gap < 1e-12, 1))
        n_tied += len(tied)
        if len(tied) == 0:
            assert np.array_equal(t[d], rt), d
            assert np.array_equal(ts[d], rts), d
            np.testing.assert_allclose(a[d], ra, rtol=1e-10, atol=1e-300)
            np.testing.assert_allclose(asd[d], rasd, rtol=1e-10, atol=1e-14)
    assert n_tied < 1e-3 * n_pairs, (n_tied, n_pairs)
    return t, ts, a, asd


@pytest.mark.parametrize("n_sta,n", [(3, 10), (17, 300), (64, 300), (5, 4096)])
def test_measure_windows_equal_restatement(n_sta, n):
    rng = np.random.default_rng(n_sta + n)
    x = 1.0 + rng.random((6, n_sta, n))
    m = np.arange(n)
    for d in range(x.shape[0]):
        for s in range(n_sta):
            x[d, s] += 5.0 * np.exp(-0.5 * ((m - n / 2 - rng.integers(-n // 10, n // 10 + 1)) / (n / 40 + 1)) ** 2)
    _measure_vs_restatement(x, 0.5)


def test_measure_negative_sxy_and_zero_energy_station():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 5, 300))         # zero-mean noise: some sxy < 0
    x[1] = 1.0 + np.abs(x[1])
    x[1, 2] = 0.0                                # zero-energy station: lag 0 with everyone
    t, ts, a, asd = measure.measure_windows(x, 1.0)
    rt, rts, ra, rasd, lag, gap = rs.measure(x[0], 1.0)
    assert np.all(ra == 0.0) and np.all(rasd == 0.0)
    assert np.all(a[0] == 0.0) and np.all(asd[0] == 0.0)
    rt1, rts1, _, _, lag1, _ = rs.measure(x[1], 1.0)
    assert np.all(lag1[2] == 0.0) and np.all(lag1[:, 2] == 0.0)
    assert np.array_equal(t[1], rt1) and np.array_equal(ts[1], rts1)


def test_measure_half_sample_shift_rounds_away_from_zero():
    # 4 stations, delays 0, 0, 0, 2 samples: lags (i, 3) = 2 -> t(3) = 2 - 0.5 = 1.5 ... t(0) = -0.5: nint -> -1, not 0
    n = 300
    m = np.arange(n)
    pulse = lambda c: 1.0 + 10.0 * np.exp(-0.5 * ((m - c) / 4.0) ** 2)
    x = np.stack([pulse(150), pulse(150), pulse(150), pulse(152)])[None]
    t, ts, a, asd = _measure_vs_restatement(x, 1.0)
    assert t[0, 0] == -0.5 and t[0, 3] == 1.5
    # with nint(-0.5) = -1 stations 0..2 are shifted one sample, station 3 two: all aligned but station 3 by one
    ra = rs.optimize_amp(x[0], t[0], 1.0)[0]
    np.testing.assert_allclose(a[0], ra, rtol=1e-10)
    # what rint (half to even) would give instead: every station aligned, a different amplitude of station 3
    t_rint = t[0].copy(); t_rint[:3] = 0.0                # rint(-0.5) = 0: the same shifts as t = 0
    assert abs(rs.optimize_amp(x[0], t_rint, 1.0)[0][3] - a[0, 3]) > 1e-3


def test_synthetic_recovery_noise_free_and_noisy():
    S, n = 6, 300
    delay = np.array([0, 3, -2, 5, 1, -1])           # mean 1: whole-sample alignment
    la = np.array([0.0, 0.4, -0.3, 0.2, -0.5, 0.1])
    env = synth.make_tremor_envelopes(S, 4, n, n, [2, 4], delay, la, noise=0.0, width=6.0, level=0.0)
    x = measure.gather_windows(list(env.amps), [2, 4], n, n)
    t, ts, a, asd = measure.measure_windows(x, env.dt)
    rt = rs.optimize_cc(x[0], env.dt)[0]
    for d in range(2):
        np.testing.assert_allclose(t[d], delay - delay.mean(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(a[d], la - la.mean(), rtol=0, atol=1e-10)
    assert np.array_equal(t[0], rt)
    noisy = synth.make_tremor_envelopes(S, 4, n, n, [2, 4], delay, la, noise=0.3, width=6.0, level=0.0, seed=4)
    xn = measure.gather_windows(list(noisy.amps), [2, 4], n, n)
    tn, _, an, _ = measure.measure_windows(xn, noisy.dt)
    # stated tolerance with noise 0.3 against bursts of 10 x e^la: one sample in t, 0.1 in log-amplitude
    assert np.all(np.abs(tn - (delay - delay.mean())) <= 1.0)
    assert np.all(np.abs(an - (la - la.mean())) <= 0.1)


def _run(args, cwd, env=None, timeout=300):
    e = dict(os.environ, PYTHONPATH=ROOT, **(env or {}))
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def _outputs(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith((".dat",)):
            out[f] = open(os.path.join(d, f), "rb").read()
    return out


def test_pipeline_end_to_end(tmp_path):
    S, n, n_win = 6, 100, 40
    delay = np.array([0, 2, -1, 3, 1, -5])
    la = np.array([0.0, 0.3, -0.2, 0.1, -0.4, 0.2])
    bursts = [5, 17, 30]
    env = synth.make_tremor_envelopes(S, n_win, n, n, bursts, delay, la, noise=0.2, width=3.0, seed=9)
    a, b, c = tmp_path / "files", tmp_path / "dev", tmp_path / "dev_small"
    params = dict(t_win_corr=100.0, t_step_corr=100.0, alpha=0.998, n_pair_thred=10)
    for d in (a, b, c):
        synth.write_envelopes(str(d), env, **params)
    _run(["hypotremormcmc_amd.correlate", "tremor.in"], a)
    assert os.path.getsize(a / "E001.E002.corr") == 24 * n * n_win
    _run(["hypotremormcmc_amd.measure", "tremor.in"], a)
    ids, times = read_detected_win(str(a / "detected_win.dat"))
    assert ids == bursts and times == [(w - 1) * 100.0 + 50.0 for w in bursts]
    # the restatement pipeline: thresholds, detections, measurements
    ref_cc, ref_mx = rs.correlate(env.amps, n, n, n_win)
    thr = [rs.threshold(ref_cc[:, p, :], 0.998) for p in range(ref_cc.shape[1])]
    assert measure.detect(ref_mx, thr, 10) == bursts
    got_thr = [float(l.split()[2]) for l in open(a / "cc_thred.dat")]
    np.testing.assert_allclose(got_thr, thr, rtol=0, atol=1e-12)
    x = measure.gather_windows(list(env.amps), bursts, n, n)
    for d, w in enumerate(bursts):
        rt, rts, ra, rasd, _, gap = rs.measure(x[d], 1.0)
        rows = np.loadtxt(a / ("opt_data.%06d.dat" % w))
        assert np.array_equal(rows[:, 3], rt) and np.array_equal(rows[:, 4], rts)
        np.testing.assert_allclose(rows[:, 5], ra, rtol=1e-10)
    _run(["hypotremormcmc_amd.select", "tremor.in"], a)
    assert os.path.exists(a / "selected_win.dat")
    # no .corr file, same bits; and many small batches, same bits
    _run(["hypotremormcmc_amd.measure", "tremor.in", "--from-envelopes"], b)
    _run(["hypotremormcmc_amd.measure", "tremor.in", "--from-envelopes"], c, env={"HTM_XCORR_MB": "0.01"})
    assert not any(f.endswith(".corr") for f in os.listdir(b))
    ref = _outputs(a)
    ref.pop("regress.dat"); ref.pop("selected_win.dat")
    assert _outputs(b) == ref and _outputs(c) == ref
    # and correlate itself in many batches writes the same files
    _run(["hypotremormcmc_amd.correlate", "tremor.in"], c, env={"HTM_XCORR_MB": "0.01"})
    for f in os.listdir(a):
        if f.endswith((".corr", ".max_corr")):
            assert open(a / f, "rb").read() == open(c / f, "rb").read(), f
