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

from . import xcorr_restatement as rs


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
