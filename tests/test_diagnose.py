"""Convergence diagnostics (split R-hat, ESS), CPU part: the numpy restatement on series whose answer is known, the
host logic of hypotremormcmc_amd.diagnose (sequences from sample records, refusals before any device call, the text of
convergence.stat).  The device against the restatement: tests/test_gpu_diagnose.py."""
import numpy as np
import pytest

from tests import diagnose_restatement as dr


def _ar1(rng, rho, n_rows, n_par):
    """stationary AR(1) columns of unit variance"""
    e = rng.normal(size=(n_rows, n_par))
    x = np.empty_like(e)
    x[0] = e[0]
    s = np.sqrt(1.0 - rho * rho)
    for i in range(1, n_rows):
        x[i] = rho * x[i - 1] + s * e[i]
    return x


@pytest.mark.parametrize("N,M", [(2000, 4), (4000, 2), (20000, 4)])
@pytest.mark.parametrize("rho", [0.0, 0.5, 0.9])
def test_restatement_on_ar1(rho, N, M):
    """R-hat near 1 and ESS near tot (1 - rho) / (1 + rho).  The band is the statistical scatter of the estimator plus
    headroom (observed 0.85-1.12, R-hat <= 1.017), not a rounding tolerance.  max_lag 200 is beyond the lag at which
    every one of these columns terminates, so it gives what 1000 gives."""
    rng = np.random.default_rng(20211)
    x = np.concatenate([_ar1(rng, rho, N, 16) for _ in range(M)], axis=0)
    out, acov, _, _ = dr.diagnose(x, M, max_lag=200)
    assert np.all(out[:, 3] >= 0), "every column terminates before max_lag"
    assert np.all(out[:, 0] < 1.05), out[:, 0].max()
    ratio = out[:, 1] / (N // 2 * 2 * M * (1 - rho) / (1 + rho))
    print("rho %.1f N %d M %d: ESS ratio %.3f..%.3f, R-hat <= %.4f" % (rho, N, M, ratio.min(), ratio.max(), out[:, 0].max()))
    assert np.all((ratio >= 0.7) & (ratio <= 1.4)), (ratio.min(), ratio.max())


def test_restatement_on_a_shifted_sequence():
    """two sequences, one shifted by 3 sigma: W = 1, the four split means are 0, 0, 3, 3, so R-hat is 2, and
    rho stays near 3/4 at every lag, so the pair sums never go negative"""
    rng = np.random.default_rng(5)
    x = rng.normal(size=(4000, 3))
    x[2000:] += 3.0
    out, _, _, _ = dr.diagnose(x, 2, max_lag=1000)
    print("shifted: R-hat", out[:, 0])
    assert np.all(out[:, 0] > 1.5)
    assert np.all(out[:, 3] == -1)


def test_restatement_splits_and_drops_the_middle_draw():
    x = np.arange(10.0).reshape(10, 1)                      # two sequences of 5
    s = dr.split_sequences(x, 2)[:, :, 0]
    assert s.tolist() == [[0, 1], [3, 4], [5, 6], [8, 9]]


def test_sequences_by_iteration():
    from hypotremormcmc_amd.diagnose import sequences_by_iteration

    # k = 3 records per iteration; rank 0 holds 2, 1, 3 of them at iterations 11, 21, 31, rank 1 the others
    it0, it1 = np.array([11, 11, 21, 31, 31, 31], np.int32), np.array([11, 21, 21], np.int32)
    v0 = np.array([[1.0, 10], [2, 20], [4, 40], [7, 70], [8, 80], [9, 90]])
    v1 = np.array([[3.0, 30], [5, 50], [6, 60]])
    x = sequences_by_iteration(np.concatenate([it0, it1]), np.concatenate([v0, v1]), 3)
    # sequence j = the j-th record of every iteration, rank 0's records before rank 1's
    assert x[:, 0].tolist() == [1, 4, 7, 2, 5, 8, 3, 6, 9]
    assert np.array_equal(x[:, 1], 10 * x[:, 0])
    with pytest.raises(ValueError, match="iteration 21"):
        sequences_by_iteration(np.concatenate([it0, it1[:2]]), np.concatenate([v0, v1[:2]]), 3)
    with pytest.raises(ValueError, match="iteration 11"):
        sequences_by_iteration(np.concatenate([it0, it1]), np.concatenate([v0, v1]), 2)


def test_diagnose_refuses_before_any_device_call():
    """device -1 would fail in the library; these fail before it is loaded"""
    from hypotremormcmc_amd.diagnose import diagnose

    with pytest.raises(ValueError, match="at least 4 draws"):
        diagnose(np.zeros((6, 2)), 2, device=-1)                                   # N = 3
    x = np.arange(16.0).reshape(8, 2)
    x[5, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or inf"):
        diagnose(x, 1, device=-1)
    x[5, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or inf"):
        diagnose(x, 1, device=-1)
    big = np.broadcast_to(np.zeros((1, 1)), (2 ** 31, 1))                          # no memory behind it
    with pytest.raises(ValueError, match="exceeds"):
        diagnose(big, 2 ** 11, device=-1)                                          # n_seq * n_draws = 2^31
    with pytest.raises(ValueError, match="equal length"):
        diagnose(np.zeros((9, 1)), 2, device=-1)


def test_c_entry_points_refuse_bad_shapes_without_a_device():
    """HTM_EINVAL (-1) comes before any device call, so it is the same with and without a GPU"""
    import ctypes as C

    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    for n_seq, n_draws, n_par, ld, max_lag in ((1, 3, 1, 1, 10), (0, 8, 1, 1, 10), (1, 8, 0, 1, 10), (1, 8, 1, 1, 0),
                                               (1, 8, 2, 1, 10), (2 ** 11, 2 ** 20, 1, 1, 10), (2, 2 ** 62, 1, 1, 10)):
        assert lib.htm_diagnose_dev(-1, p, n_seq, n_draws, n_par, ld, max_lag, p, None, None) == -1, (n_seq, n_draws)
        assert b"" != lib.htm_last_error()
        if ld >= n_par:
            assert lib.htm_diagnose(-1, buf, n_seq, n_draws, n_par, max_lag, buf, None) == -1, (n_seq, n_draws)
    # a launch beyond 2^32 - 1 work-items: 2^24 column groups x 64 split sequences x 256 threads
    assert lib.htm_diagnose_dev(-1, p, 32, 8, 2 ** 30, 2 ** 30, 10, p, None, None) == -1
    assert b"work-items" in lib.htm_last_error()


def test_convergence_stat_text():
    from hypotremormcmc_amd.diagnose import parameter_names, stat_text, summary_text

    names = parameter_names(["N.AAA ", "N.BBB"], [7, 12])
    assert names == ["vs", "qs", "t_corr N.AAA", "t_corr N.BBB", "a_corr N.AAA", "a_corr N.BBB",
                     "x 7", "y 7", "z 7", "x 12", "y 12", "z 12", "log_likelihood"]
    out = np.array([[np.nan] * 4, [1.0123456789, 1234.5, 3.25, 14], [2.5, 40.0, 100.0, -1]])
    text = stat_text(["vs", "t_corr N.AAA", "log_likelihood"], out)
    lines = text.split("\n")
    assert lines[0].startswith("#") and lines[4] == "" and len(lines) == 5
    assert lines[1] == "vs" + " " * 22 + " " * 10 + "NaN" + " " * 10 + "NaN" + " " * 10 + "NaN" + "    NaN"
    assert lines[2] == "t_corr N.AAA" + " " * 12 + "     1.012346  1234.500000     3.250000     14"
    assert lines[3] == "log_likelihood" + " " * 10 + "     2.500000    40.000000   100.000000     -1"
    s = summary_text(["vs", "t_corr N.AAA", "log_likelihood"], out, 1.01)
    assert "2 parameters (1 constant)" in s
    assert "largest R-hat  2.500000  (log_likelihood)" in s and "smallest ESS   40.0  (log_likelihood)" in s
    assert "R-hat > 1.01: 2 parameters" in s and "upper bound): 1 parameters" in s
