"""CPU: the one reader and writer of a step-5 run's files (hypotremormcmc_amd/run_files.py) -- the window list, the record
layout of the sample files, the per-rank gather with its agreement checks, the device selection and the number-or-NaN field --
and statistics' hypo.stat row rule."""
import struct

import numpy as np
import pytest

from hypotremormcmc_amd import run_files as rf
from hypotremormcmc_amd import synth
from tests.helpers import write_fake_samples, write_run_dir

N_STA, WIN_ID = 3, [4, 9]


def _run(tmp_path, monkeypatch, **params):
    """a run directory of 2 ranks, 2 windows and 3 stations, opened; the sample files are the test's to write"""
    monkeypatch.delenv("HTM_SAMPLE_ENDIAN", raising=False)
    monkeypatch.delenv("HTM_DEVICE", raising=False)
    data = synth.make_synthetic(len(WIN_ID), N_STA, 0)
    param_file, _ = write_run_dir(tmp_path, data, dict(synth.DEFAULT_PARAMS, n_procs=2, **params), WIN_ID)
    return param_file, rf.Step5Run.open(param_file)


def _values(rng, n_rec, names):
    width = {"vs": 1, "qs": 1, "t_corr": N_STA, "a_corr": N_STA, "hypo": 3 * len(WIN_ID)}
    return {nm: rng.normal(size=(n_rec, width[nm])) for nm in names}


# ---- the window list -------------------------------------------------------------------------------------------------
def test_read_window_ids(tmp_path):
    p = tmp_path / "win.dat"
    for text, want in (("3 0.0\n12 150.0\n", [3, 12]), ("3\n12\n", [3, 12]), ("\n3 0.0\n   \n\n12 150.0\n\n", [3, 12]),
                       ("# id, start\n3 0.0\n  # 7 1.0\n12 150.0 # the last\n", [3, 12]), ("", [])):
        p.write_text(text)
        assert rf.read_window_ids(str(p)) == want, text


def test_the_driver_keeps_its_exit_for_a_missing_window_list(tmp_path):
    from hypotremormcmc_amd import driver

    with pytest.raises(SystemExit, match="cannot open selected_win.dat"):
        driver.read_selected_win(str(tmp_path / "selected_win.dat"))
    (tmp_path / "selected_win.dat").write_text("# ids\n5 0.0\n6\n")
    assert driver.read_selected_win(str(tmp_path / "selected_win.dat")) == [5, 6]


# ---- the record layout -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_val", [1, 6])
@pytest.mark.parametrize("endian,bo", [("little", "<"), ("big", ">")])
def test_sample_file_round_trip_and_bytes(endian, bo, n_val, tmp_path, monkeypatch):
    """write -> read gives the records back, and the bytes are the packed records [int32][n_val float64] that one
    struct.pack per record gives: 4 + 8 n_val bytes each, no padding"""
    monkeypatch.delenv("HTM_SAMPLE_ENDIAN", raising=False)
    rng = np.random.default_rng(3)
    iters = np.array([10, 20, 20, 2 ** 31 - 1, -5])
    values = rng.normal(size=(5, n_val))
    values[1, 0], values[2, -1], values[3, 0] = np.nan, -0.0, 1e300
    path = str(tmp_path / "x.out")
    rf.write_sample_file(path, iters, values[:, 0] if n_val == 1 else values, endian=endian)
    raw = open(path, "rb").read()
    assert raw == b"".join(struct.pack(bo + "i%dd" % n_val, int(i), *v) for i, v in zip(iters, values))
    assert len(raw) == 5 * (4 + 8 * n_val) and rf.record_dtype(n_val, endian).itemsize == 4 + 8 * n_val
    it, v = rf.read_sample_file(path, n_val, endian=endian)
    assert it.dtype == np.int32 and v.dtype == np.float64 and v.shape == (5, n_val)
    assert np.array_equal(it, iters) and np.array_equal(v, values, equal_nan=True) and np.signbit(v[2, -1])
    monkeypatch.setenv("HTM_SAMPLE_ENDIAN", endian)                     # the variable picks the order where none is given
    rf.write_sample_file(path, iters, values)
    assert open(path, "rb").read() == raw
    assert np.array_equal(rf.read_sample_file(path, n_val)[1], values, equal_nan=True)


def test_a_file_without_records(tmp_path):
    path = str(tmp_path / "x.out")
    rf.write_sample_file(path, np.zeros(0, dtype=np.int64), np.zeros(0))
    assert open(path, "rb").read() == b""
    it, v = rf.read_sample_file(path, 1)
    assert it.shape == (0,) and v.shape == (0, 1)


# ---- the per-rank gather ---------------------------------------------------------------------------------------------
def test_samples_stack_two_ranks_in_rank_order(tmp_path, monkeypatch):
    _, run = _run(tmp_path, monkeypatch)
    assert (run.work, run.win_id, run.n_procs, run.n_sta, run.n_events, run.device) == (str(tmp_path), WIN_ID, 2, N_STA, 2, 0)
    rng = np.random.default_rng(4)
    names = ("vs", "qs", "t_corr", "a_corr", "hypo")
    its = [np.array([10, 10, 20]), np.array([10, 20, 20, 30])]           # the ranks need not record the same number
    parts = [_values(rng, len(it), names) for it in its]
    for r in range(2):
        write_fake_samples(tmp_path, r, its[r], parts[r])
    iters, s = run.samples(names)
    assert list(s) == list(names) and np.array_equal(iters, np.concatenate(its))
    for nm in names:
        assert np.array_equal(s[nm], np.concatenate([parts[0][nm], parts[1][nm]])), nm
    iters, s = run.samples(("hypo",))
    assert list(s) == ["hypo"] and s["hypo"].shape == (7, 6) and len(iters) == 7


def test_reader_refuses_mismatched_iteration_columns(tmp_path, monkeypatch):
    _, run = _run(tmp_path, monkeypatch)
    rng = np.random.default_rng(2)
    it = np.arange(10, 60, 10)
    parts = {}
    for r in range(2):
        v = _values(rng, len(it), ("hypo", "vs", "qs"))
        write_fake_samples(tmp_path, r, it + r, v)
        parts.update({(nm, r): v[nm] for nm in v})
    _, s = run.samples(("hypo", "vs", "qs"))
    hypo, piv = s["hypo"], np.hstack([s["vs"], s["qs"]])
    assert np.array_equal(hypo, np.concatenate([parts["hypo", 0], parts["hypo", 1]]))
    assert np.array_equal(piv, np.concatenate([np.hstack([parts["vs", 0], parts["qs", 0]]), np.hstack([parts["vs", 1], parts["qs", 1]])]))
    write_fake_samples(tmp_path, 1, it + 2, {"qs": parts["qs", 1]})
    with pytest.raises(ValueError, match=r"qs\.01\.out records other iterations than hypo\.01\.out"):
        run.samples(("hypo", "vs", "qs"))


def test_likelihood_trace_is_cut_at_the_burn_in(tmp_path, monkeypatch):
    _, run = _run(tmp_path, monkeypatch, n_burn=20)
    rng = np.random.default_rng(5)
    trace_it = np.repeat(np.arange(10, 51, 10), 2)                        # 10 10 20 20 | 30 30 40 40 50 50
    traces, parts = [], []
    for r in range(2):
        traces.append(rng.normal(size=len(trace_it)))
        parts.append(_values(rng, 6, ("vs", "hypo")))
        write_fake_samples(tmp_path, r, trace_it[4:], parts[r])
        rf.write_sample_file(str(tmp_path / ("likelihood%02d.out" % r)), trace_it, traces[r])
    iters, s = run.samples(("vs", "hypo"), likelihood=True)
    assert list(s) == ["vs", "hypo", "likelihood"] and np.array_equal(iters, np.tile(trace_it[4:], 2))
    assert np.array_equal(s["likelihood"], np.concatenate([traces[0][4:], traces[1][4:]])[:, None])
    assert np.array_equal(s["vs"], np.concatenate([parts[0]["vs"], parts[1]["vs"]]))
    assert "likelihood" not in run.samples(("vs", "hypo"))[1]
    rf.write_sample_file(str(tmp_path / "likelihood01.out"), trace_it + 10, traces[1])        # 20 20 | 30 30 40 40 50 50 60 60
    with pytest.raises(ValueError, match=r"likelihood01\.out records other iterations after the burn-in than vs\.01\.out"):
        run.samples(("vs", "hypo"), likelihood=True)


def test_statistics_refuses_a_mismatched_file(tmp_path, monkeypatch):
    """step 6 reads its five files through the same gather: it stops at the file before any device call"""
    from hypotremormcmc_amd import statistics

    param_file, _ = _run(tmp_path, monkeypatch, n_iter=2000, n_burn=1000, n_interval=10)          # n_mod = 200
    rng = np.random.default_rng(6)
    it = np.arange(1010, 2001, 10)
    for r in range(2):
        write_fake_samples(tmp_path, r, it, _values(rng, len(it), ("vs", "qs", "t_corr", "a_corr", "hypo")))
    write_fake_samples(tmp_path, 1, it + 1, _values(rng, len(it), ("a_corr",)))
    with pytest.raises(ValueError, match=r"a_corr\.01\.out records other iterations than vs\.01\.out"):
        statistics.main([param_file])
    assert not (tmp_path / "uniform_structure.stat").exists()


# ---- the device, the field, hypo.stat's rows -------------------------------------------------------------------------
def test_device_from_env(tmp_path, monkeypatch):
    monkeypatch.delenv("HTM_DEVICE", raising=False)
    assert rf.device_from_env() == 0
    monkeypatch.setenv("HTM_DEVICE", "3")
    assert rf.device_from_env() == 3
    data = synth.make_synthetic(len(WIN_ID), N_STA, 0)
    param_file, _ = write_run_dir(tmp_path, data, synth.DEFAULT_PARAMS, WIN_ID)
    assert rf.Step5Run.open(param_file).device == 3


def test_field():
    assert rf.field(float("nan"), 13) == "          NaN" and rf.field(np.nan, 15) == " " * 12 + "NaN" and rf.field(np.nan, 10, 3) == "       NaN"
    assert rf.field(-4.5, 13) == "    -4.500000" and rf.field(-4.5, 15) == "      -4.500000" and rf.field(-4.5, 10, 3) == "    -4.500"
    assert rf.field(1.23456789, 13) == "%13.6f" % 1.23456789 == "     1.234568" and rf.field(179.9996, 10, 3) == "   180.000"
    assert rf.field(-1234567.5, 13) == "-1234567.500000"                  # wider than the field: nothing is cut
    assert rf.field(7.0, 7, 0) == "      7" and rf.field(-1.0, 7, 0) == "     -1"


def test_hypo_rows_and_as_printed():
    from hypotremormcmc_amd.statistics import as_printed, hypo_rows

    h = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0],                    # window 0: (lo, med, hi) of x, y, z
                  [-0.5, 0.12345649, 0.5], [10.0, 20.00000051, 30.0], [1e-9, 2e-7, 123456.7890125]])
    rows = hypo_rows(h)
    assert rows[0] == [2.0, 1.0, 3.0, 5.0, 4.0, 6.0, 8.0, 7.0, 9.0]
    assert rows[1] == [0.12345649, -0.5, 0.5, 20.00000051, 10.0, 30.0, 2e-7, 1e-9, 123456.7890125] and len(rows) == 2
    p = as_printed(rows)
    assert p[0] == rows[0]
    assert p[1] == [0.123456, -0.5, 0.5, 20.000001, 10.0, 30.0, 0.0, 0.0, float("%13.6f" % 123456.7890125)]
    assert hypo_rows(np.zeros((0, 3))) == []
