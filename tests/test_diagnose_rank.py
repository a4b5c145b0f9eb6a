"""Rank-normalised diagnostics, CPU part: the numpy restatement on inputs whose answer is known -- the two
cases the un-normalised diagnostics are blind to, iid draws, a monotone transform, ties -- and the host logic of
hypotremormcmc_amd.diagnose (refusals before any device call, the text of convergence_rank.stat).  The device against the
restatement: tests/test_gpu_diagnose_rank.py."""
import ctypes as C

import numpy as np
import pytest

from tests import diagnose_rank_restatement as rr
from tests import diagnose_restatement as dr


def _blind_case(kind):
    rng = np.random.default_rng(7)
    if kind == "scale":
        x = rng.normal(size=(4, 1000))
        x[0] *= 3.0
    else:
        x = rng.standard_cauchy(size=(4, 1000))
        x[0] *= 4.0
    return x.reshape(4000, 1)


@pytest.mark.parametrize("kind", ["scale", "cauchy"])
def test_restatement_sees_what_the_plain_numbers_miss(kind):
    """4 x 1000 draws, one sequence wider than the others: the plain split R-hat calls it converged, the folded one does not,
    and the tails of the scale case are worth a few dozen draws"""
    x = _blind_case(kind)
    plain = dr.diagnose(x, 4)[0][0]
    out = rr.diagnose_rank(x, 4)[0][0]
    print("%s: plain rhat %.4f ess %.0f; rhat_bulk %.4f rhat_folded %.4f ess_bulk %.0f ess_tail %.1f" % ((kind, plain[0], plain[1]) + tuple(out)))
    assert plain[0] < 1.01
    assert out[1] > 1.05
    if kind == "scale":
        assert out[3] < 100


def test_restatement_on_iid_normals():
    """the band tests/test_diagnose.py uses for its iid (rho = 0) check: R-hat < 1.05, ESS within 0.7 .. 1.4 of the draws"""
    rng = np.random.default_rng(20211)
    x = rng.normal(size=(8000, 16))
    out = rr.diagnose_rank(x, 4, max_lag=200)[0]
    print("iid: rhat_bulk <= %.4f, rhat_folded <= %.4f, ess_bulk/tot %.3f..%.3f, ess_tail/tot %.3f..%.3f" % (
        out[:, 0].max(), out[:, 1].max(), out[:, 2].min() / 8000, out[:, 2].max() / 8000, out[:, 3].min() / 8000, out[:, 3].max() / 8000))
    assert np.all(out[:, :2] < 1.05)
    assert np.all((out[:, 2:] / 8000 >= 0.7) & (out[:, 2:] / 8000 <= 1.4))


def test_restatement_is_invariant_under_a_monotone_transform():
    rng = np.random.default_rng(11)
    x = rng.normal(size=(2000, 3))
    a, b = rr.diagnose_rank(x, 4)[0], rr.diagnose_rank(np.exp(x), 4)[0]
    assert np.array_equal(a[:, [0, 2]], b[:, [0, 2]])
    assert not np.array_equal(a[:, 1], b[:, 1]), "the folded form is not invariant: exp moves the median's neighbours apart"


def test_restatement_ranks_of_ties():
    rng = np.random.default_rng(3)
    x = np.round(2.0 * rng.normal(size=1001))
    x[::7] = -0.0
    x[3::7] = 0.0
    r = rr.ranks(x)[:, 0]
    assert np.array_equal(2 * r, np.round(2 * r)) and r.min() >= 1 and r.max() <= 1001
    assert r.sum() == 1001 * 1002 / 2
    assert len(np.unique(r[x == 0])) == 1, "-0.0 and +0.0 share a rank"
    assert len(np.unique(r)) == len(np.unique(x))
    z = rr.z_of_ranks(r[:, None])[:, 0]
    assert np.array_equal(np.argsort(r, kind="stable"), np.argsort(z, kind="stable"))


def test_restatement_quantile_and_median():
    x = np.array([[5.0], [1.0], [4.0], [2.0], [3.0], [6.0]])
    assert rr.median(x)[0] == 3.5 and rr.median(x[:5])[0] == 3.0
    h = 5 * 0.05
    assert rr.quantile(x, 0.05)[0] == 1.0 + h * (2.0 - 1.0)
    assert rr.quantile(x, 0.95)[0] == 5.0 + (5 * 0.95 - 4) * (6.0 - 5.0)
    i05, i95 = rr.indicators(x)
    assert i05[:, 0].tolist() == [0, 1, 0, 0, 0, 0] and i95[:, 0].tolist() == [0, 0, 0, 0, 0, 1]


def test_rank_entry_points_refuse_before_any_device_call():
    """device -1 would fail in the library; these fail before it is loaded"""
    from hypotremormcmc_amd.diagnose import diagnose_rank, rank_normalize

    with pytest.raises(ValueError, match="at least 4 draws"):
        diagnose_rank(np.zeros((6, 2)), 2, device=-1)
    x = np.arange(16.0).reshape(8, 2)
    for bad in (np.nan, np.inf, -np.inf):
        x[5, 1] = bad
        with pytest.raises(ValueError, match="NaN or inf"):
            diagnose_rank(x, 1, device=-1)
        with pytest.raises(ValueError, match="NaN or inf"):
            rank_normalize(x, device=-1)
    big = np.broadcast_to(np.zeros((1, 1)), (2 ** 31, 1))
    with pytest.raises(ValueError, match="exceeds"):
        diagnose_rank(big, 2 ** 11, device=-1)
    with pytest.raises(ValueError, match="exceeds"):
        rank_normalize(big, device=-1)
    with pytest.raises(ValueError, match="equal length"):
        diagnose_rank(np.zeros((9, 1)), 2, device=-1)
    with pytest.raises(ValueError, match="max_lag"):
        diagnose_rank(np.zeros((8, 1)), 2, max_lag=0, device=-1)
    with pytest.raises(ValueError, match="at least 2 rows"):
        rank_normalize(np.zeros((1, 3)), device=-1)
    with pytest.raises(ValueError, match="rows..n_par"):
        rank_normalize(np.zeros((2, 2, 2)), device=-1)


def test_c_entry_points_refuse_bad_arguments_without_a_device(monkeypatch):
    """HTM_EINVAL (-1) comes before any device call, so it is the same with and without a GPU; a good shape then gives
    HTM_ENODEVICE (-2) where there is none"""
    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    for n_seq, n_draws, n_par, ld, max_lag in ((1, 3, 1, 1, 10), (0, 8, 1, 1, 10), (1, 8, 0, 1, 10), (1, 8, 1, 1, 0),
                                               (1, 8, 2, 1, 10), (2 ** 11, 2 ** 20, 1, 1, 10), (2, 2 ** 62, 1, 1, 10)):
        assert lib.htm_diagnose_rank_dev(-1, p, n_seq, n_draws, n_par, ld, max_lag, p, None) == -1, (n_seq, n_draws)
        assert b"" != lib.htm_last_error()
        if ld >= n_par:
            assert lib.htm_diagnose_rank(-1, buf, n_seq, n_draws, n_par, max_lag, buf) == -1, (n_seq, n_draws)
    assert lib.htm_diagnose_rank_dev(-1, None, 1, 8, 1, 1, 10, p, None) == -1 and lib.htm_last_error() == b"NULL argument"
    assert lib.htm_diagnose_rank_dev(-1, p, 1, 8, 1, 1, 10, None, None) == -1
    assert lib.htm_diagnose_rank(-1, None, 1, 8, 1, 10, buf) == -1 and lib.htm_diagnose_rank(-1, buf, 1, 8, 1, 10, None) == -1
    # (n_rows, n_par, ld, ld_z)
    for n_rows, n_par, ld, ld_z in ((1, 1, 1, 1), (0, 1, 1, 1), (8, 0, 1, 1), (8, 2, 1, 2), (8, 2, 2, 1), (2 ** 31, 1, 1, 1)):
        assert lib.htm_rank_normalize_dev(-1, p, n_rows, n_par, ld, 0, p, ld_z, None, None) == -1, (n_rows, n_par, ld, ld_z)
        if ld >= n_par and ld_z >= n_par:
            assert lib.htm_rank_normalize(-1, buf, n_rows, n_par, 1, buf, None) == -1, (n_rows, n_par)
    assert lib.htm_rank_normalize_dev(-1, None, 8, 1, 1, 0, p, 1, None, None) == -1 and lib.htm_last_error() == b"NULL argument"
    assert lib.htm_rank_normalize_dev(-1, p, 8, 1, 1, 0, None, 1, None, None) == -1
    assert lib.htm_rank_normalize(-1, None, 8, 1, 0, buf, None) == -1 and lib.htm_rank_normalize(-1, buf, 8, 1, 0, None, None) == -1
    # a launch beyond 2^32 - 1 work-items: 2^24 column groups x 64 split sequences x 256 threads (k_diag_mean's) ...
    assert lib.htm_diagnose_rank_dev(-1, p, 32, 8, 2 ** 30, 2 ** 30, 10, p, None) == -1
    assert b"work-items" in lib.htm_last_error()
    # ... and the key transpose of one column of 2^31 - 1 rows: 2^25 row tiles x 256 threads
    assert lib.htm_rank_normalize_dev(-1, p, 2 ** 31 - 1, 1, 1, 0, p, 1, None, None) == -1
    assert b"work-items" in lib.htm_last_error()
    monkeypatch.setenv("HTM_RANK_MB", "0")
    assert lib.htm_rank_normalize_dev(-1, p, 8, 1, 1, 0, p, 1, None, None) == -1 and b"HTM_RANK_MB" in lib.htm_last_error()
    monkeypatch.delenv("HTM_RANK_MB")
    n = C.c_int(-1)
    if lib.htm_device_count(C.byref(n)) == 0 and n.value > 0:
        return                                    # with a GPU the good shapes run: tests/test_gpu_diagnose_rank.py
    assert lib.htm_rank_normalize_dev(0, p, 8, 2, 2, 1, p, 2, None, None) == -2 and b"no HIP device" in lib.htm_last_error()
    assert lib.htm_rank_normalize(0, buf, 8, 2, 0, buf, buf) == -2
    assert lib.htm_diagnose_rank_dev(0, p, 1, 8, 2, 2, 10, p, None) == -2
    assert lib.htm_diagnose_rank(0, buf, 1, 8, 2, 10, buf) == -2


def test_convergence_rank_stat_text():
    from hypotremormcmc_amd.diagnose import rank_stat_text, rank_summary_text

    names = ["vs", "t_corr N.AAA", "log_likelihood", "x 7"]
    out = np.array([[np.nan] * 4, [1.0123456789, 1.2, 1234.5, 31.25], [2.5, 1.5, 40.0, np.nan], [1.001, np.nan, 900.0, 800.0]])
    lines = rank_stat_text(names, out).split("\n")
    assert lines[0].startswith("#") and lines[5] == "" and len(lines) == 6
    assert lines[1] == "vs" + " " * 22 + (" " * 10 + "NaN") * 5
    assert lines[2] == "t_corr N.AAA" + " " * 12 + "     1.200000     1.012346     1.200000  1234.500000    31.250000"
    assert lines[3] == "log_likelihood" + " " * 10 + "     2.500000     2.500000     1.500000    40.000000          NaN"
    assert lines[4] == "x 7" + " " * 21 + "     1.001000     1.001000          NaN   900.000000   800.000000"
    s = rank_summary_text(names, out, 1.01).split("\n")
    assert len(s) == 4 and s[3] == ""
    assert s[0] == "largest rank-normalised R-hat  2.500000  (log_likelihood)"
    assert s[1] == "smallest bulk-ESS  40.0  (log_likelihood), smallest tail-ESS  31.2  (t_corr N.AAA)"
    assert s[2] == "rank-normalised R-hat > 1.01: 2 parameters"
    assert "no parameter varies" in rank_summary_text(names[:1], out[:1], 1.01)
