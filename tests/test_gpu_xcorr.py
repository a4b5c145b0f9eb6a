"""Steps 2 and 3 on the GPU (`htm_xcorr`, `htm_measure_windows`, python -m hypotremormcmc_amd.correlate / .measure)
against the compiled reference (tests/golden/xcorr_*.npz), against the numpy restatement of the reference in
tests/xcorr_restatement.py and its long-double direct sums at edge shapes, and on synthetic tremor with known delays
and amplitudes."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hypotremormcmc_amd import _lib, correlate as corr, measure, synth
from hypotremormcmc_amd._lib import check, dp
from hypotremormcmc_amd.select import read_detected_win

from . import helpers, xcorr_restatement as rs

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


def _select_files(d, param_file):
    """regress.dat and selected_win.dat that `select` wrote in d, against oracle.select_regress and select() on the
    opt_data files there: 1e-10 relative, NaN in place, the same windows.  -> (regress rows, the opt_data inputs)"""
    from oracle import oracle

    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.param import Param
    from hypotremormcmc_amd.select import select

    para = Param(str(d / param_file), from_where="select")
    g = para.values
    ids, times = read_detected_win(str(d / "detected_win.dat"))
    obs = ObsData(ids, para.n_stations, para.sta_x, para.sta_y, directory=str(d))
    ref = oracle.select_regress(para.sta_x, para.sta_y, para.sta_z, g["z_guess"], obs.t_obs, obs.t_stdv, obs.a_obs,
                                obs.a_stdv)
    reg = np.array([float(x) for x in open(d / "regress.dat").read().split()]).reshape(-1, 7)
    assert reg[:, 0].astype(int).tolist() == ids
    assert np.array_equal(np.isnan(reg[:, 1:]), np.isnan(ref))
    np.testing.assert_allclose(reg[:, 1:], ref, rtol=1e-10, atol=0)
    keep = select(ref, g["vs_min"], g["vs_max"], g["b_min"], g["b_max"])
    rows = [ln.split() for ln in open(d / "selected_win.dat") if ln.strip()]
    assert [int(r[0]) for r in rows] == [i for i, k in zip(ids, keep) if k]
    assert [float(r[1]) for r in rows] == [tm for tm, k in zip(times, keep) if k]
    return reg, obs


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
    # every station at depth z_guess = 0: log(0) at the nearest station, so the amplitude columns are NaN; the lags of
    # these bursts are consistent, t_stdv = 0 gives weights of inf and the time columns are NaN too
    reg, _ = _select_files(a, "tremor.in")
    assert np.all(np.isnan(reg[:, [2, 4, 6]]))
    # with the source below the stations the amplitude regression is finite
    (a / "deeper.in").write_text(open(a / "tremor.in").read().replace("z_guess = 0.0", "z_guess = 2.5"))
    _run(["hypotremormcmc_amd.select", "deeper.in"], a)
    reg, _ = _select_files(a, "deeper.in")
    assert np.all(np.isfinite(reg[:, [2, 4, 6]]))
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


def test_pipeline_select_keeps_some_windows(tmp_path):
    """noisier, wider bursts: the lags are not all consistent, every t_stdv > 0 and both regressions are finite; the vs
    window keeps two of the three detections (vs of about -4.6, -5.0 and -5.3 in the restatement)"""
    S, n, n_win = 6, 100, 40
    delay = np.array([0, 2, -1, 3, 1, -5])
    la = np.array([0.0, 0.3, -0.2, 0.1, -0.4, 0.2])
    bursts = [5, 17, 30]
    env = synth.make_tremor_envelopes(S, n_win, n, n, bursts, delay, la, noise=1.0, width=6.0, seed=9)
    synth.write_envelopes(str(tmp_path), env, t_win_corr=100.0, t_step_corr=100.0, alpha=0.998, n_pair_thred=10,
                          z_guess=2.5, vs_min=-5.15, vs_max=0.0)
    _run(["hypotremormcmc_amd.measure", "tremor.in", "--from-envelopes"], tmp_path)
    ids, _ = read_detected_win(str(tmp_path / "detected_win.dat"))
    assert ids == bursts
    _run(["hypotremormcmc_amd.select", "tremor.in"], tmp_path)
    reg, obs = _select_files(tmp_path, "tremor.in")
    assert np.all(obs.t_stdv > 0) and np.all(np.isfinite(reg))
    assert [int(ln.split()[0]) for ln in open(tmp_path / "selected_win.dat") if ln.strip()] == [5, 17]


def test_pipeline_dead_first_station(tmp_path):
    """station 1 records nothing: step 3 gives every amplitude of a window NaN (0/0), step 4's maxloc
    then has no candidate and takes station 1.  select must run, regress on the times from station 1,
    write NaN amplitude columns, and keep none of those windows."""
    from hypotremormcmc_amd.obs_data import maxloc

    S, n, n_win = 6, 100, 40
    delay = np.array([0, 2, -1, 3, 1, -5])
    la = np.array([0.0, 0.3, -0.2, 0.1, -0.4, 0.2])
    bursts = [5, 17, 30]
    env = synth.make_tremor_envelopes(S, n_win, n, n, bursts, delay, la, noise=0.2, width=3.0, seed=9)
    env.amps[0] = 0.0
    # the five pairs with station 1 have zero correlograms; the ten live pairs detect the bursts
    synth.write_envelopes(str(tmp_path), env, t_win_corr=100.0, t_step_corr=100.0, alpha=0.998, n_pair_thred=8,
                          z_guess=2.5, vs_min=-1.0e9)
    _run(["hypotremormcmc_amd.measure", "tremor.in", "--from-envelopes"], tmp_path)
    ids, _ = read_detected_win(str(tmp_path / "detected_win.dat"))
    assert ids == bursts
    _run(["hypotremormcmc_amd.select", "tremor.in"], tmp_path)
    reg, obs = _select_files(tmp_path, "tremor.in")
    assert np.all(np.isnan(obs.a_obs)) and np.all(maxloc(obs.a_obs) == 0)
    assert np.all(np.isfinite(obs.t_obs)) and np.all(np.isfinite(obs.t_stdv)) and np.all(obs.t_stdv > 0)
    assert np.all(np.isnan(reg[:, [2, 4, 6]])) and np.all(np.isfinite(reg[:, [1, 3, 5]]))
    # the time columns are those of station 1 as the nearest: not those of any other station
    from oracle import oracle

    for k in range(1, S):
        a_k = np.full_like(obs.a_obs, -1.0)
        a_k[:, k] = 0.0
        other = oracle.select_regress(obs.sta_x, obs.sta_y, np.zeros(S), 2.5, obs.t_obs, obs.t_stdv, a_k, obs.a_stdv)
        assert not np.allclose(other[:, [0, 2, 4]], reg[:, [1, 3, 5]], rtol=1e-10, atol=0)
    assert open(tmp_path / "selected_win.dat").read().strip() == ""


# ---- steps 2 and 3 against the compiled reference (tests/golden/xcorr_*.npz, make_golden.py) ---------------------------

def _fixture_dir(tmp_path, case):
    fx, env, g = helpers.load_xcorr_case(case)
    synth.write_envelopes(str(tmp_path), env, t_win_corr=repr(g["n"] * g["dt"]), t_step_corr=repr(g["n_step"] * g["dt"]),
                          alpha=repr(float(fx["alpha"])), n_pair_thred=int(fx["n_pair_thred"]))
    return fx, env, g


def _check_step3_files(d, fx, env, g):
    S = g["n_sta"]
    prs = corr.pairs(env.stations)
    tok = open(d / "cc_thred.dat").read().split()
    assert tok[0::3] == [a for a, _ in prs] and tok[1::3] == [b for _, b in prs]
    np.testing.assert_allclose([float(v) for v in tok[2::3]], fx["thred"], rtol=0, atol=1e-12)
    ids, times = read_detected_win(str(d / "detected_win.dat"))
    assert ids == fx["detected"].tolist() and times == fx["detected_time"].tolist()
    for k, w in enumerate(ids):
        rows = np.array([float(v) for v in open(d / ("opt_data.%06d.dat" % w)).read().split()]).reshape(S, 7)
        ref = fx["opt"][k]
        assert np.array_equal(rows[:, :5], ref[:, :5]), w               # x y z, t, t_stdv
        np.testing.assert_allclose(rows[:, 5:], ref[:, 5:], rtol=1e-10, atol=0)


@pytest.mark.parametrize("case", helpers.XCORR_CASES)
def test_programs_equal_compiled_reference(case, tmp_path, monkeypatch):
    fx, env, g = _fixture_dir(tmp_path / "files", case)
    _fixture_dir(tmp_path / "dev", case)
    n, n_win = g["n"], g["n_win"]
    monkeypatch.chdir(tmp_path / "files")
    corr.main(["tremor.in"])
    for p, (a, b) in enumerate(corr.pairs(env.stations)):
        v = corr.read_corr(f"{a}.{b}.corr").reshape(n_win, n, 3)
        np.testing.assert_allclose(v[:, :, 2], fx["cc"][:, p], rtol=0, atol=1e-12)
        np.testing.assert_allclose(corr.read_max_corr(f"{a}.{b}.max_corr")[:, 1], fx["cc_max"][:, p], rtol=0, atol=1e-12)
    measure.main(["tremor.in"])
    _check_step3_files(tmp_path / "files", fx, env, g)
    monkeypatch.chdir(tmp_path / "dev")
    measure.main(["tremor.in", "--from-envelopes"])
    _check_step3_files(tmp_path / "dev", fx, env, g)


# ---- k_xcorr at the shapes and edges where it could go wrong, against a long-double direct sum -------------------------

def _prep_exact(w):
    """src/cls_correlator.f90:207-212 in long double (the taper factors in double, as the kernel takes them)"""
    n = w.size
    nleng = int(n * 0.05)
    f = np.ones(n)
    for q in range(nleng):
        f[q] = f[n - 1 - q] = 0.5 * (1.0 - math.cos(q * math.pi / nleng))
    x = np.asarray(w, dtype=np.longdouble) * np.asarray(f, dtype=np.longdouble)
    x = x - np.sum(x) / n
    return x / np.sqrt(np.sum(x * x))


def _xcorr_exact(amps, n, n_step, n_win, prs):
    """-> cc (n_win, len(prs), n) in the reference's lag order from long-double sums"""
    out = np.empty((n_win, len(prs), n))
    for w in range(n_win):
        r = {s: _prep_exact(amps[s, w * n_step:w * n_step + n]) for s in {s for pr in prs for s in pr}}
        for p, (i, j) in enumerate(prs):
            out[w, p] = rs.reference_order(rs.circ_exact(r[i], r[j]))
    return out


def _envelopes(rng, n_sta, n_smp, n):
    """positive envelopes: a level, noise, and a burst of n/8 samples somewhere in every row"""
    m = np.arange(n_smp)
    a = 1.0 + rng.random((n_sta, n_smp))
    for s in range(n_sta):
        c = rng.integers(0, n_smp)
        a[s] += 8.0 * np.exp(-0.5 * ((m - c) / (n / 8.0 + 0.5)) ** 2)
    return a


def _bound(n):
    return 2.0 * n * 2.0 ** -53


XC_SIZES = [2, 20, 22, 62, 64, 66, 130, 1022, 1024, 1026, 2050, 3000, 4094]


@pytest.mark.parametrize("k,n", list(enumerate(XC_SIZES)))
def test_xcorr_shapes_against_exact_sums(k, n):
    # n_step below, at and above n in turn; 3 stations up to 1026 samples, 2 above (one pair, n_sta = 2)
    n_step = (n // 2 + 1, n, n + 3)[k % 3]
    n_sta, n_win = (3, 3) if n <= 1026 else (2, 2)
    rng = np.random.default_rng(100 + n)
    amps = _envelopes(rng, n_sta, (n_win - 1) * n_step + n + 1, n)
    cc, mx = xcorr(amps, n, n_step, n_win)
    prs = [(i, j) for i in range(n_sta - 1) for j in range(i + 1, n_sta)]
    ex = _xcorr_exact(amps, n, n_step, n_win, prs)
    assert np.max(np.abs(cc - ex)) <= _bound(n), np.max(np.abs(cc - ex))
    assert np.array_equal(mx, cc.max(axis=2))
    assert np.max(np.abs(mx - ex.max(axis=2))) <= _bound(n)


@pytest.mark.parametrize("n_sta,n,n_step,n_win,pair0,n_pairs,pad_env,pad_cc", [
    (5, 300, 100, 4, 2, 6, 37, 5),            # a middle range of pairs
    (100, 66, 70, 3, 4949, 1, 11, 3),         # the last pair of 100 stations
    (2, 1026, 500, 2, 0, 1, 1, 7),            # two stations
    (4, 3000, 3000, 2, 0, 6, 64, 2),          # several lags per thread
])
def test_xcorr_dev_strides_leave_padding_alone(n_sta, n, n_step, n_win, pair0, n_pairs, pad_env, pad_cc):
    """htm_xcorr_dev on a torch buffer with row stride ld_env > n_smp and ld_cc > n_pairs: NaN in every padding element
    of the input must not reach a result, and NaN in the padding columns of cc and cc_max must stay untouched."""
    import torch

    rng = np.random.default_rng(n_sta + n)
    n_smp = (n_win - 1) * n_step + n
    host = np.full((n_sta, n_smp + pad_env), np.nan)
    host[:, :n_smp] = _envelopes(rng, n_sta, n_smp, n)
    dev = torch.device("cuda", 0)
    d_env = torch.from_numpy(host).to(dev)
    ld_cc = n_pairs + pad_cc
    d_cc = torch.full((n_win * n, ld_cc), float("nan"), dtype=torch.float64, device=dev)
    d_mx = torch.full((n_win, ld_cc), float("nan"), dtype=torch.float64, device=dev)
    check(_lib.load().htm_xcorr_dev(0, C.c_void_p(d_env.data_ptr()), n_smp + pad_env, n_smp, n_sta, n, n_step, n_win,
                                    pair0, n_pairs, C.c_void_p(d_cc.data_ptr()), ld_cc, C.c_void_p(d_mx.data_ptr()), None))
    torch.cuda.synchronize()
    cc, mx = d_cc.cpu().numpy(), d_mx.cpu().numpy()
    assert np.all(np.isnan(cc[:, n_pairs:])) and np.all(np.isnan(mx[:, n_pairs:]))
    all_prs = [(i, j) for i in range(n_sta - 1) for j in range(i + 1, n_sta)]
    ex = _xcorr_exact(host[:, :n_smp], n, n_step, n_win, all_prs[pair0:pair0 + n_pairs])
    got = cc[:, :n_pairs].reshape(n_win, n, n_pairs).transpose(0, 2, 1)
    assert np.max(np.abs(got - ex)) <= _bound(n)
    assert np.array_equal(mx[:, :n_pairs], got.max(axis=2))


def test_thresholds_of_correlograms_take_the_slab_path_exactly():
    """k_xcorr output of 2000 windows x 60 pairs at n = 300 (n_mod * n_par = 36 M: the slab select) in a buffer of
    row stride 64 > 60, through htm_quantiles_dev: every selected element equals np.sort's"""
    import torch

    n, n_step, n_win, n_sta, pair0, n_pairs, ld = 300, 150, 2000, 12, 3, 60, 64
    rng = np.random.default_rng(77)
    amps = _envelopes(rng, n_sta, (n_win - 1) * n_step + n, n)
    env = corr.Envelopes(amps, device=0)
    d_cc = torch.full((n_win * n, ld), float("nan"), dtype=torch.float64, device=env.dev)
    d_mx = torch.full((n_win, ld), float("nan"), dtype=torch.float64, device=env.dev)
    env.correlate(n, n_step, n_win, pair0, n_pairs, d_cc, d_mx)
    n_mod = n * n_win
    r = measure.threshold_rank(n, n_win, 0.995)
    thr = measure._thresholds_dev(d_cc, n_mod, n_pairs, r, 0)
    ranks = (1, r, n_mod)
    out = torch.empty((n_pairs, 3), dtype=torch.float64, device=env.dev)
    check(_lib.load().htm_quantiles_dev(0, C.c_void_p(d_cc.data_ptr()), n_mod, n_pairs, ld, (C.c_int * 3)(*ranks),
                                        C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    srt = np.sort(d_cc.cpu().numpy()[:, :n_pairs], axis=0)
    assert not np.any(np.isnan(srt))
    assert np.array_equal(thr, srt[r - 1])
    assert np.array_equal(out.cpu().numpy(), srt[[q - 1 for q in ranks]].T)
    assert np.all(np.isnan(d_mx.cpu().numpy()[:, n_pairs:]))


# ---- k_measure at the shapes and edges where it could go wrong ---------------------------------------------------------

def _pulses(rng, n_det, n_sta, n, width=None):
    m = np.arange(n)
    x = 0.5 + 0.2 * rng.random((n_det, n_sta, n))
    w = width or (n / 40 + 1)
    for d in range(n_det):
        for s in range(n_sta):
            c = n / 2 + rng.integers(-n // 6, n // 6 + 1)
            x[d, s] += 6.0 * np.exp(-0.5 * ((m - c) / w) ** 2)
    return x


def _measure_vs_exact(x, dt):
    """measure_windows against the restatement with long-double direct correlations; near-tied pairs (top two within
    1e-12) are counted, not compared.  NaN and inf results (zero-energy stations) must match in place."""
    t, ts, a, asd = measure.measure_windows(x, dt)
    n_pairs = n_tied = 0
    S = x.shape[1]
    for d in range(x.shape[0]):
        with np.errstate(divide="ignore", invalid="ignore"):
            rt, rts, ra, rasd, lag, gap = rs.measure(x[d], dt, circ=rs.circ_exact)
        n_pairs += S * (S - 1) // 2
        tied = int(np.count_nonzero(np.triu(gap < 1e-12, 1)))
        n_tied += tied
        if tied:
            continue
        assert np.array_equal(t[d], rt), d
        assert np.array_equal(ts[d], rts), d
        np.testing.assert_allclose(a[d], ra, rtol=1e-10, atol=1e-13, equal_nan=True)
        np.testing.assert_allclose(asd[d], rasd, rtol=1e-10, atol=1e-13, equal_nan=True)
    assert n_tied <= 1e-3 * n_pairs, (n_tied, n_pairs)
    return t, ts, a, asd


@pytest.mark.parametrize("n_sta,n", [(5, 301), (4, 1025), (5, 20), (5, 66), (4, 1026), (3, 3000), (3, 20), (130, 64)])
def test_measure_shapes_against_exact_sums(n_sta, n):
    # odd n; the taper inside one wave; several samples per thread; stations outnumbering the threads (130 > 64)
    rng = np.random.default_rng(7 * n + n_sta)
    x = _pulses(rng, 2 if n_sta < 100 else 1, n_sta, n)
    _measure_vs_exact(x, 0.25)


@pytest.mark.parametrize("n", [64, 300, 1026])
def test_measure_maximum_at_half_window_and_shifts_off_both_ends(n):
    """pair (0, 1) peaks at natural lag n/2 exactly, where the sign convention switches (lag -n/2 dt: idx < n/2 gives
    idx dt, else (idx - n) dt); the large lags then shift stations by more than n/4 samples in both directions"""
    m = np.arange(n)
    pulse = lambda c: 0.05 + 10.0 * np.exp(-0.5 * ((m - c) / 2.0) ** 2)
    q = n // 4
    x = np.stack([pulse(q), pulse(q + n // 2), pulse(q + 1), pulse(q + n // 2 - 2), pulse(2 * q)])[None]
    t, ts, a, asd = _measure_vs_exact(x, 0.5)
    lag = rs.optimize_cc(x[0], 0.5, rs.circ_exact)[2]
    assert lag[0, 1] == -(n // 2) * 0.5                  # the maximum at index n/2 exactly
    it = [corr.nint(v / 0.5) for v in t[0]]
    assert max(it) > n // 8 and min(it) < -n // 8        # samples pushed off both ends
    assert np.all(np.isfinite(a))


def test_measure_zero_energy_station_nan_and_inf_in_place():
    rng = np.random.default_rng(31)
    x = _pulses(rng, 3, 5, 300)
    x[0, 0] = 0.0               # the first station: 0/0 in every rel(0, j)
    x[1, 3] = 0.0               # a later one: log(0 / sxx(i)) = -inf
    x[2, 4] = 0.0               # the last one
    t, ts, a, asd = _measure_vs_exact(x, 1.0)
    assert np.any(np.isnan(a)) and np.any(np.isinf(a[1:]) | np.isnan(a[1:]))


def test_measure_windows_split_over_launches_same_bits(monkeypatch):
    """HTM_MEASURE_MB: one window per launch, 7 per launch (7 + 7 + 6), all in one launch -- identical bits"""
    rng = np.random.default_rng(41)
    n_det, S, n = 20, 6, 300
    x = _pulses(rng, n_det, S, n)
    x[5, 2] = 0.0               # NaN / inf results travel through the chunk copies too
    per_win = (S * n + S * S + 5 * S) * 8
    runs = []
    for mb in (None, 1e-9, 7.5 * per_win / 2 ** 20):
        if mb is None:
            monkeypatch.delenv("HTM_MEASURE_MB", raising=False)
        else:
            monkeypatch.setenv("HTM_MEASURE_MB", repr(mb))
        runs.append(measure.measure_windows(x, 0.5))
    for r in runs[1:]:
        for u, v in zip(runs[0], r):
            assert u.tobytes() == v.tobytes()
    monkeypatch.delenv("HTM_MEASURE_MB", raising=False)
    _measure_vs_exact(x[:5], 0.5)
