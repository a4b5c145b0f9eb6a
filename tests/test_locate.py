"""CPU: the host side of `locate` (hypotremormcmc_amd/locate.py) and the numpy restatement the GPU tests compare with
(tests/locate_restatement.py): the restatement against closed forms, marginal_quantiles on hand-made marginals,
read_structure on written files, the text of both output files, what htm_forward_locate refuses before any device call, the
noise-free recovery of truths on cell centres, and the restatement's side of the preconditions of tests/test_gpu_locate.py."""
import math
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from tests import locate_cases as cases
from tests import locate_restatement as lr


# ---- the restatement against closed forms ------------------------------------------------------------------------------
def test_restatement_summary_of_a_gaussian_volume():
    """lp = a separable Gaussian log density on a fine wide grid: evidence 1, mean, covariance and quantiles of the Gaussian
    (a midpoint rule on a smooth integrand over +-8 sigma: errors far below 1e-6)"""
    mu, sd = np.array([1.0, -2.0, 3.0]), np.array([1.5, 0.7, 1.1])
    n = 161
    grid = np.concatenate([[mu[a] - 8 * sd[a], 16 * sd[a] / n, n] for a in range(3)])
    xyz = lr.cell_xyz(grid)
    lp = sum(-0.5 * ((xyz[..., a] - mu[a]) / sd[a]) ** 2 - math.log(sd[a]) - lr.LOG_2PI_HALF for a in range(3))
    s = lr.summarise(lp, grid)
    assert abs(s["log_evidence"]) < 1e-6
    assert np.allclose(s["mean"], mu, atol=1e-6) and np.allclose(s["cov"], np.diag(sd ** 2), atol=1e-6)
    assert all(abs(m.sum() - 1.0) < 1e-13 for m in s["marg"])
    q = lr.quantiles(s["marg"], grid)
    assert np.allclose(q[:, 1], mu, atol=1e-3) and np.allclose(q[:, 2] - q[:, 0], 2 * 1.959964 * sd, rtol=2e-3)
    c = (n // 2) * (1 + n + n * n)
    assert s["index"] == c and np.allclose(s["best"], mu, atol=1e-12) and s["second"] < s["lp"]


def test_restatement_prior_is_normalised_and_excludes_at_and_below_z0():
    grid = np.array([-100.0, 2.0, 100, -90.0, 2.0, 100, -4.0, 0.5, 160])
    lp, ab = lr.log_prior(grid, [3.0, 7.0, 12.0, 1.25, 9.0])
    z = lr.centres(grid, 2)
    assert np.all(np.isneginf(lp[z <= 1.25])) and np.all(np.isfinite(lp[z > 1.25])) and (z == 1.25).any()
    assert abs(np.exp(lp).sum() * 2.0 * 2.0 * 0.5 - 1.0) < 1e-3       # the depth prior is cut at 76 km = 8 widths; midpoint rule
    fin = np.isfinite(lp)
    assert np.all(ab[fin] >= np.abs(lp[fin]))


def test_restatement_terms_add_up():
    """the two data types' terms add to the term of both, abs_terms bounds the term, and at the truth of noise-free data the
    misfit vanishes: the term is minus the constants"""
    both, time, amp = (cases.parity_case(3, 5, "5x3x2", m) for m in ("both", "time", "amp"))
    assert np.allclose(time["ell"] + amp["ell"], both["ell"], rtol=1e-13, atol=0)
    assert np.all(both["abs"] >= np.abs(both["ell"]) * (1 - 1e-14))
    rec = cases.recovery_case()
    n = lr.counts(rec["grid"])
    ell = lr.ell_volume(rec["sta"], tuple(o[:1] for o in rec["obs"]), True, True, *rec["structure"], rec["grid"]).reshape(-1)
    const = 12 * (2 * lr.LOG_2PI_HALF + math.log(0.1) + math.log(0.05))
    assert abs(ell[rec["index"][0]] + const) < 1e-9 and n[0] * n[1] * n[2] == ell.size


def test_noise_free_recovery_restatement():
    """truths exactly on cell centres, observations from the restatement's forward there, flat prior: the best cell is the
    truth's, for every window"""
    rec = cases.recovery_case()
    ell = lr.ell_volume(rec["sta"], rec["obs"], True, True, *rec["structure"], rec["grid"])
    got = [lr.summarise(v, rec["grid"]) for v in ell]
    assert [s["index"] for s in got] == list(rec["index"])
    assert np.array_equal(np.array([s["best"] for s in got]), rec["truth"])


# ---- the preconditions of the GPU tests, on the restatement ---------------------------------------------------------------
def test_parity_cases_have_a_clear_best_cell():
    """the best index of the device is compared with the restatement's own only where its two best cells differ by more than
    1e-9: with the chosen seeds that leaves out no window"""
    todo = [(n_sta, n_events, grid, mode) for n_sta in (3, 64, 65) for n_events in (1, 5) for grid in ("1x1x1", "5x3x2", "67x3x5")
            for mode in ("both", "time", "amp")] + [(5, 1, "70x60x2", "both"), (4, 1, "300x3x1", "both"), (3, 1, "70x60x2", "time")]
    for args in todo:
        c = cases.parity_case(*args)
        for key in ("ell", "lp_prior"):
            for v in c[key]:
                s = lr.summarise(v, c["grid"])
                assert s["lp"] - s["second"] > 1e-9, (args, key)
    c = cases.missing_case()
    assert all(lr.summarise(v, c["grid"])["lp"] - lr.summarise(v, c["grid"])["second"] > 1e-9 for key in ("ell", "lp_prior") for v in c[key])


def test_excluded_case_has_the_patterns_it_is_meant_to():
    c = cases.excluded_case()
    assert np.isnan(c["ell"][:, 0, 1, 1]).all() and np.isfinite(np.delete(c["ell"].reshape(3, -1), 6, axis=1)).all()
    assert np.isneginf(c["lp_prior"][0, 0]).sum() == 14 and np.isnan(c["lp_prior"][0, 0, 1, 1])
    assert np.isfinite(c["lp_prior"][1]).sum() == 15 and np.isneginf(c["lp_prior"][1, 0]).sum() == 14 and not lr.included(c["lp_prior"][2]).any()


def test_end_to_end_reference_covers_the_truth():
    """the restatement's 95 % interval of every window of the end-to-end job holds the truth on at least two of three axes"""
    ref = cases.e2e_reference()
    inside = (ref["quant"][:, :, 0] <= ref["truth"]) & (ref["truth"] <= ref["quant"][:, :, 2])
    assert np.all(inside.sum(axis=1) >= 2), inside


# ---- marginal_quantiles -----------------------------------------------------------------------------------------------
def test_marginal_quantiles_on_hand_made_marginals():
    grid = [10.0, 2.0, 4, -5.0, 0.5, 3, 0.0, 1.0, 5]
    mx = [0.0, 1.0, 0.0, 0.0]                       # all mass in one cell: the quantile q lies at the share q of that cell
    my = [0.0, 0.0, 1.0]                            # ... in the last cell
    mz = [0.2] * 5                                  # uniform: the quantile q lies at the share q of the axis
    q = lc.marginal_quantiles(np.array(mx + my + mz), grid, levels=(0.025, 0.5, 0.975, 0.2))
    assert np.allclose(q[0], [12.0 + 2.0 * v for v in (0.025, 0.5, 0.975, 0.2)], rtol=0, atol=1e-15)
    assert np.allclose(q[1], [-4.0 + 0.5 * v for v in (0.025, 0.5, 0.975, 0.2)], rtol=0, atol=1e-15)
    assert np.allclose(q[2], [5.0 * v for v in (0.025, 0.5, 0.975, 0.2)], rtol=0, atol=1e-15)
    # a step in the middle of a cell: 0.3 | 0.7 -> the median lies 2/7 into the second cell
    q = lc.marginal_quantiles(np.array([0.3, 0.7, 0.0, 0.0] + my + mz), grid, levels=(0.5,))
    assert abs(q[0, 0] - (10.0 + 2.0 * (1 + 0.2 / 0.7))) < 1e-14
    # rows: one NaN marginal gives NaN on every axis of that row only; and the restatement agrees on random marginals
    rng = np.random.default_rng(3)
    m = rng.random((4, 12))
    for lo, hi in ((0, 4), (4, 7), (7, 12)):
        m[:, lo:hi] /= m[:, lo:hi].sum(axis=1, keepdims=True)
    m[2] = np.nan
    q = lc.marginal_quantiles(m, grid)
    assert q.shape == (4, 3, 3) and np.isnan(q[2]).all() and not np.isnan(np.delete(q, 2, axis=0)).any()
    for e in (0, 1, 3):
        assert np.allclose(q[e], lr.quantiles((m[e, :4], m[e, 4:7], m[e, 7:]), grid), rtol=0, atol=1e-13)


# ---- read_structure ---------------------------------------------------------------------------------------------------
def test_read_structure(tmp_path):
    names = ["S003", "S001", "S002"]
    cases.write_structure(str(tmp_path), names, [0.3, -0.1, 0.2], [0.03, 0.01, -0.02])
    vs, qs, tc, ac = lc.read_structure(str(tmp_path), ["S001", "S002 ", "S003"])          # the station file's order
    assert (vs, qs) == (3.1, 240.0)
    assert np.array_equal(tc, [-0.1, 0.2, 0.3]) and np.array_equal(ac, [0.01, -0.02, 0.03])
    with pytest.raises(ValueError, match="station S009 of the station file is not in"):
        lc.read_structure(str(tmp_path), ["S001", "S009"])
    os.remove(tmp_path / "uniform_structure.stat")
    with pytest.raises(FileNotFoundError, match="uniform_structure.stat is missing"):
        lc.read_structure(str(tmp_path), names)
    with pytest.raises(FileNotFoundError, match="station_corrections.stat is missing"):
        cases.write_structure(str(tmp_path), names, [0, 0, 0], [0, 0, 0])
        os.remove(tmp_path / "station_corrections.stat")
        lc.read_structure(str(tmp_path), names)


# ---- the output files -------------------------------------------------------------------------------------------------
def test_text_of_the_output_files():
    quant = np.array([[[-1.5, 0.25, 2.0], [10.0, 11.0, 12.5], [3.0, 4.0, 5.0]], [[np.nan] * 3] * 3])
    text = lc.stat_text([7, 123456], quant)
    assert text == lr.stat_text([7, 123456], quant)
    lines = text.split("\n")
    assert lines[0].startswith("# window ID, x (50%), x (2.5%) x (97.5%)")
    assert lines[1] == "        7     0.250000    -1.500000     2.000000    11.000000    10.000000    12.500000     4.000000     3.000000     5.000000"
    assert lines[2] == "   123456" + "          NaN" * 9 and lines[3] == ""
    grid = [0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2]
    res = {"index": np.array([5, 17, -1]), "best": np.array([[1.5, 1.5, 0.5], [1.5, 1.5, 1.5], [np.nan] * 3]), "lp": np.array([-3.25, -4.0, np.nan]),
           "ell": np.array([-1.0, -2.0, np.nan]), "log_evidence": np.array([0.5, 0.25, np.nan]), "mean": np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [np.nan] * 3])}
    # 4 x 3 x 2 cells: every cell lies on a z face; (1, 1) is off the x and y faces
    assert list(lc.on_face(res["index"], grid)) == [True, True, False]
    assert list(lc.on_face([5 + 12, 5 + 24], [0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 4])) == [False, False]
    lines = lc.best_text([1, 2, 3], res, grid).split("\n")
    assert lines[0] == lc.BEST_HEADER and len(lines) == 5
    assert lines[1] == "        1" + "".join("%15.6f" % v for v in (1.5, 1.5, 0.5, -3.25, -1.0, 0.5, 1.0, 2.0, 3.0)) + "  1"
    assert lines[3] == "        3" + "            NaN" * 9 + "  0"
    assert lc.summary_text(res, grid) == ("3 windows located on 4 x 3 x 2 cells\n2 with the best cell on a face of the box (not resolved by this grid), "
                                          "1 without an included cell\n")
    vol = np.arange(24.0).reshape(2, 3, 4)
    vol[1, 2, 3] = -np.inf
    lines = lc.volume_text(vol, grid).split("\n")
    assert len(lines) == 26 and lines[6].split() == ["5", "1.500000", "1.500000", "0.500000", "5"] and lines[24].split()[-1] == "-inf"


# ---- what the library refuses before any device call --------------------------------------------------------------------
def test_null_handle_needs_no_device():
    """a NULL handle is HTM_EINVAL with a message (the other refusals need a handle: tests/test_gpu_locate.py)"""
    lib = lc._lib.load()
    v, g = np.zeros(16), np.array([0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2])
    p = lc._lib.ptr
    assert lib.htm_forward_locate(None, p(v), 3.0, p(v), 250.0, p(g), None, p(v), None, None) == -1
    assert lib.htm_last_error().decode() == "NULL handle"
