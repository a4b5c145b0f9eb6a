"""CPU: the host side of `locate --draws` (hypotremormcmc_amd/locate.py: read_structure_draws, the argument handling), what
htm_forward_locate_marginal refuses without a device, and the reference's side of the preconditions of
tests/test_gpu_locate_marginal.py (tests/locate_marginal_cases.py)."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import run_files
from tests import locate_marginal_cases as mc


# ---- the preconditions of the GPU tests, on the reference alone ----------------------------------------------------------
@pytest.mark.parametrize("key", mc.PRECONDITION_CASES)
def test_tight_draws_share_the_weight(key):
    """K = 9, tight: at 90 % of the cells or more, three or more draws have a normalised weight above 1e-3 -- a draw that is
    dropped or counted twice moves those cells by far more than the parity bound"""
    c = mc.marginal_case(key, 9, "tight")
    w = mc.weights(c["ell_k"])
    share = ((w > 1e-3).sum(axis=0) >= 3).mean()
    print(f"{key}: share of cells with >= 3 draws above 1e-3 = {share:.2f}")
    assert share >= 0.9, (key, share)


@pytest.mark.parametrize("key", mc.PRECONDITION_CASES)
def test_wide_mixture_is_no_single_draw(key):
    """K = 9, wide: at every cell the mixture differs from every single draw's term by more than 1e-9 A, a thousand times the
    parity bound -- returning the largest draw, or any one draw, fails the parity test everywhere"""
    c = mc.marginal_case(key, 9, "wide")
    gap = np.min(np.abs(c["ell"][None] - c["ell_k"]) / c["abs"][None])
    print(f"{key}: smallest |mixture - draw| / A = {gap:.2e}")
    assert gap > 1e-9, (key, gap)


def test_reference_mixture_rules():
    """one draw is itself; equal draws are one draw; NaN in any draw is NaN; a draw of -inf has no weight; all -inf is -inf"""
    a = np.array([-3.0, -700.0, 2.5])
    assert np.array_equal(mc.mixture(a[None]), a)
    assert np.allclose(mc.mixture(np.stack([a] * 5)), a, rtol=0, atol=1e-15 * 700)
    got = mc.mixture(np.array([[-1.0, np.nan, -np.inf, -np.inf], [-1.0, 0.0, -2.0, -np.inf]]))
    assert got[0] == -1.0 and np.isnan(got[1]) and abs(got[2] - (-2.0 - np.log(2.0))) < 1e-15 and np.isneginf(got[3])
    # against the plain sum where nothing underflows
    rng = np.random.default_rng(1)
    x = rng.normal(-5.0, 2.0, (7, 11))
    assert np.allclose(mc.mixture(x), np.log(np.exp(x).mean(axis=0)), rtol=1e-14, atol=0)


# ---- read_structure_draws ------------------------------------------------------------------------------------------------
NAMES = ["S001", "S002", "S003"]


def test_even_thinning_picks_the_stated_records():
    assert lc.draw_records(12, 6) == [1, 3, 5, 7, 9, 11] and lc.draw_records(12, 12) == list(range(12))
    assert lc.draw_records(12, 1) == [6] and lc.draw_records(12, 5) == [1, 3, 6, 8, 10] and lc.draw_records(7, 2) == [1, 5]


def test_read_structure_draws_across_two_ranks(tmp_path):
    d = str(tmp_path)
    vs, qs, tc, ac = mc.write_calibration(d, NAMES, n_ranks=2, n_rec=6)
    assert vs.shape == (12,) and tc.shape == (12, 3)
    for K, keep in ((5, [1, 3, 6, 8, 10]), (12, list(range(12))), (1, [6])):      # (records 6.. are rank 01's)
        got = lc.read_structure_draws(d, ["S001", "S002 ", "S003"], 3, K)
        assert all(isinstance(g, np.ndarray) for g in got) and got[0].shape == (K,) and got[2].shape == (K, 3)
        for g, full in zip(got, (vs, qs, tc, ac)):
            assert np.array_equal(g, full[keep]), K
    # a third rank's file that does not follow 00, 01 is not read
    run_files.write_sample_file(os.path.join(d, "vs.03.out"), [1], [9.0])
    assert np.array_equal(lc.read_structure_draws(d, NAMES, 3, 12)[0], vs)


def test_read_structure_draws_errors(tmp_path):
    d = str(tmp_path)
    with pytest.raises(FileNotFoundError, match="vs.00.out is missing"):
        lc.read_structure_draws(d, NAMES, 3, 2)
    mc.write_calibration(d, NAMES, n_ranks=2, n_rec=6)
    with pytest.raises(ValueError, match="13 draws asked for.*12 records in 2 rank"):
        lc.read_structure_draws(d, NAMES, 3, 13)
    with pytest.raises(ValueError, match="need at least one"):
        lc.read_structure_draws(d, NAMES, 3, 0)
    # the names of station_corrections.stat must be the station file's, in its order
    for names in (["S002", "S001", "S003"], ["S001", "S002"], ["S001", "S002", "S003", "S004"], ["S001", "S002", "S009"]):
        with pytest.raises(ValueError, match="must be the same, in the same order"):
            lc.read_structure_draws(d, names, len(names), 2)
    # a rank whose files record other iterations (Step5Run.samples)
    v = np.zeros(6)
    run_files.write_sample_file(os.path.join(d, "qs.01.out"), 7 + np.arange(6), v + 250.0)
    with pytest.raises(ValueError, match="qs.01.out records other iterations"):
        lc.read_structure_draws(d, NAMES, 3, 2)
    os.remove(os.path.join(d, "station_corrections.stat"))
    with pytest.raises(FileNotFoundError, match="station_corrections.stat is missing"):
        lc.read_structure_draws(d, NAMES, 3, 2)


def test_names_are_compared_by_their_first_twelve_characters(tmp_path):
    d = str(tmp_path)
    long_names = ["STATION_NUMBER_1", "STATION_NUMBER_2"]
    mc.write_calibration(d, [n[:12] for n in long_names], n_ranks=1, n_rec=3)
    with pytest.raises(ValueError, match="must be the same"):      # (both names are STATION_NUMB there: the order cannot be told, equal lists pass)
        lc.read_structure_draws(d, ["OTHER", "STATION_NUMBER_2"], 2, 2)
    assert lc.read_structure_draws(d, long_names, 2, 3)[2].shape == (3, 2)


# ---- what needs no device ---------------------------------------------------------------------------------------------------
def test_null_handle_needs_no_device():
    lib = lc._lib.load()
    v, g = np.zeros(16), np.array([0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2])
    p = lc._lib.ptr
    assert lib.htm_forward_locate_marginal(None, 2, p(v), p(v), p(v), p(v), p(g), None, p(v), None, None) == -1
    assert lib.htm_last_error().decode() == "NULL handle"


@pytest.mark.parametrize("k", ["0", "-3"])
def test_program_refuses_draws_below_one(k, capsys):
    """before the parameter file is opened: the one named here does not exist"""
    with pytest.raises(SystemExit) as e:
        lc.main(["no_such_file.in", "--cell", "5", "--draws", k])
    assert e.value.code == 2 and f"--draws {k}: need at least one draw" in capsys.readouterr().err


def test_summary_names_the_draws():
    res = {"index": np.array([5, -1])}
    grid = [0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 4]
    assert lc.summary_text(res, grid, 64).split("\n")[0] == "2 windows located on 4 x 3 x 4 cells, the structure marginalised over 64 draws"
    assert lc.summary_text(res, grid).split("\n")[0] == "2 windows located on 4 x 3 x 4 cells"
