"""CPU: the rule of htm_forward_locate_residuals (include/htm_hip.h) as tests/locate_residuals_restatement.py
restates it -- against the oracle's demeaned synthetics, against the log-likelihood term, at a one-cell posterior and with
excluded cells; the restatement in fp64 against itself in numpy.longdouble under the bounds that the GPU tests hold the library
to, on their cases; the texts of the three files; the program's argument error; and the entry point's refusals that need no
device.  The plan of a residual request: tests/test_locate_residuals_plan.py."""
import numpy as np
import pytest

from hypotremormcmc_amd import _lib
from hypotremormcmc_amd import locate as lc
from oracle import oracle
from tests import locate_cases as cases
from tests import locate_residuals_cases as rc
from tests import locate_residuals_restatement as rr
from tests import locate_restatement as lr

RTOL_L = 1e-12
ENTRY = _lib.load().htm_forward_locate_residuals      # what this file is about: without the entry point none of it says anything


def restated(c, prior, dtype=np.float64):
    return rr.restate(c["sta"], c["obs"], c["use"], c["structure"], c["grid"], c["lp_prior"] if prior else c["ell"], dtype)


# ---- the restatement against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(3, 5, "5x3x2", "both"), (65, 5, "67x3x5", "both"), "missing"])
def test_rho_is_the_observation_minus_the_oracles_demeaned_synthetic(key):
    c = rc.case(key)
    r = restated(c, False)
    tc, vs, ac, qs = c["structure"]
    xyz = lr.cell_xyz(c["grid"]).reshape(-1, 3)
    E = c["obs"][0].shape[0]
    fw = oracle.Forward(c["sta"][0], c["sta"][1], c["sta"][2], *c["obs"])
    worst = 0.0
    for cell in sorted({0, 1, xyz.shape[0] // 2, xyz.shape[0] - 1}):
        hypo = np.tile(xyz[cell], E)
        for e in range(E):
            for d, syn in ((0, fw.calc_travel_time_single(e + 1, hypo, tc, vs)), (1, fw.calc_amp_single(e + 1, hypo, ac, qs, vs))):
                ratio = np.abs(r["rho"][e, d, cell] - (c["obs"][2 * d][e] - syn)) / r["X"][e, d, cell]
                worst = max(worst, float(ratio.max()))
                assert np.all(ratio <= 1e-12), (key, cell, e, d, ratio.max())
    print(f"{key}: worst |rho - (obs - oracle's demeaned synthetic)| / X = {worst:.3e}")


@pytest.mark.parametrize("key", [(3, 5, "5x3x2", "both"), (65, 1, "67x3x5", "amp"), (64, 5, "5x3x2", "time"), "missing"])
def test_weighted_residuals_sum_to_zero_and_chi2_is_the_term(key):
    c = rc.case(key)
    r = restated(c, False)
    for e in range(c["obs"][0].shape[0]):
        p_t, p_a, ct, ca = rr.precisions(c["obs"], e)
        term = np.zeros(r["chi2"].shape[2])
        for d, (p, const) in enumerate(((p_t, ct), (p_a, ca))):
            if not c["use"][d]:
                continue
            assert np.all(np.abs((p[None] * r["rho"][e, d]).sum(axis=1)) <= 1e-12 * (p[None] * r["X"][e, d]).sum(axis=1)), (key, e, d)
            term += -0.5 * r["chi2"][e, d] - const
        ell, ab = c["ell"][e].reshape(-1), c["abs"][e].reshape(-1)
        assert np.all(np.abs(term - ell) <= RTOL_L * ab), (key, e, float(np.max(np.abs(term - ell) / ab)))


def test_a_posterior_of_one_cell_gives_the_best_cell_exactly():
    c = rc.case((6, 2, "5x3x2", "both"))
    vol = np.full(c["ell"].shape, -np.inf)
    vol[:, 1, 2, 3] = c["ell"][:, 1, 2, 3]
    r = rr.restate(c["sta"], c["obs"], c["use"], c["structure"], c["grid"], vol)
    assert np.array_equal(r["res"][:, :, 0], r["res"][:, :, 1]) and np.array_equal(r["res"][:, :, 2], r["res"][:, :, 3])
    for d in range(2):
        assert np.array_equal(r["fit"][:, 5 * d], r["fit"][:, 5 * d + 1]) and np.array_equal(r["fit"][:, 5 * d + 3], r["fit"][:, 5 * d + 4])
        assert np.all(r["fit"][:, 5 * d + 2] == 0.0)
    # a 1 x 1 x 1 grid is one too
    c1 = rc.case((3, 5, "1x1x1", "both"))
    r1 = restated(c1, True)
    assert np.array_equal(r1["res"][:, :, 0], r1["res"][:, :, 1]) and np.all(r1["fit"][:, 2] == 0.0) and np.all(r1["fit"][:, 7] == 0.0)


def test_excluded_cells_do_not_enter():
    """cases.excluded_case(): station 0 on a cell centre (its amplitude residual there is infinite), a layer at z0, an event
    with no cell: every number of the two events that have cells is finite, the third is NaN throughout; and moving the excluded
    cells' values changes nothing"""
    c = cases.excluded_case()
    r = restated(c, True)
    assert list(r["index"] >= 0) == [True, True, False]
    assert np.isfinite(r["res"][:2]).all() and np.isfinite(r["fit"][:2]).all() and np.isnan(r["res"][2]).all() and np.isnan(r["fit"][2]).all()
    assert np.isinf(r["rho"][0, 1, 1 + 5 * 1]).any()                          # (the cell on the station)
    vol = c["lp_prior"].copy()
    vol[np.isneginf(vol)] = np.nan                                           # another way of being excluded
    r2 = rr.restate(c["sta"], c["obs"], c["use"], c["structure"], c["grid"], vol)
    assert np.array_equal(r2["res"], r["res"], equal_nan=True) and np.array_equal(r2["fit"], r["fit"], equal_nan=True)


# ---- the bounds of the GPU tests, without a device -------------------------------------------------------------------------------
@pytest.mark.parametrize("key", rc.GPU_CASES, ids=rc.case_id)
def test_fp64_restatement_stays_within_the_gpu_bounds_of_the_longdouble_one(key):
    c = rc.case(key)
    for prior in (False, True):
        lo, hi = restated(c, prior), restated(c, prior, np.longdouble)
        worst = rr.compare(lo["res"], lo["fit"], hi, c["use"], what=rc.case_id(key))
        print(f"{rc.case_id(key)}, prior {prior}: worst |fp64 - longdouble| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ---- the texts ---------------------------------------------------------------------------------------------------------------
def _text_inputs():
    res = np.array([[[0.25, 0.125, -0.5, -0.25], [-0.25, -0.125, 0.5, 0.25]],
                    [[np.nan] * 4, [np.nan] * 4],                                   # a window without a cell
                    [[0.5, 0.75, 1.0, 1.5], [7.0, 7.0, 7.0, 7.0]]])                  # its second station is missing
    fit = np.array([[1.0, 1.5, 0.25, 4.0, 4.5, -2.0, -2.5, 0.125, 8.0, 8.5], [np.nan] * 10, [0.0, 0.0, 0.0, 1.0, 1.0, 3.0, 3.0, 0.0, 2.0, 2.0]])
    t_stdv = np.array([[0.5, 0.25], [0.5, 0.5], [0.5, 0.0]])
    a_stdv = np.array([[0.125, 0.25], [0.25, 0.25], [0.5, 0.0]])
    return [11, 12, 15], ["STA1", "LONGSTATION123"], res, fit, t_stdv, a_stdv


def test_residuals_text():
    win, names, res, fit, ts, as_ = _text_inputs()
    assert lc.residuals_text(win, names, res, ts, as_) == lc.RESIDUALS_HEADER + "\n" + "\n".join([
        "       11 STA1          0       0.250000       0.125000       0.5000      -0.500000      -0.250000      -4.0000",
        "       11 LONGSTATION1  0      -0.250000      -0.125000      -1.0000       0.500000       0.250000       2.0000",
        "       12 STA1          0            NaN            NaN          NaN            NaN            NaN          NaN",
        "       12 LONGSTATION1  0            NaN            NaN          NaN            NaN            NaN          NaN",
        "       15 STA1          0       0.500000       0.750000       1.0000       1.000000       1.500000       2.0000",
        "       15 LONGSTATION1  1            NaN            NaN          NaN            NaN            NaN          NaN"]) + "\n"
    only_t = lc.residuals_text(win[:1], names[:1], res, ts, as_, use=(True, False)).split("\n")
    assert only_t[1] == "       11 STA1          0       0.250000       0.125000       0.5000"
    only_a = lc.residuals_text(win[:1], names[:1], res, ts, as_, use=(False, True)).split("\n")
    assert only_a[1] == "       11 STA1          0      -0.500000      -0.250000      -4.0000"


def test_fit_text():
    win, names, res, fit, ts, as_ = _text_inputs()
    assert lc.fit_text(win, fit, ts) == lc.FIT_HEADER + "\n" + "\n".join([
        "       11     2       1.000000       1.500000       0.250000       4.000000       4.500000      -2.000000      -2.500000       0.125000"
        "       8.000000       8.500000       2.500000",
        "       12     2" + "            NaN" * 11,
        "       15     1       0.000000       0.000000       0.000000       1.000000       1.000000       3.000000       3.000000       0.000000"
        "       2.000000       2.000000      -3.000000"]) + "\n"
    assert lc.fit_text(win[:1], fit, ts, use=(True, False)).split("\n")[1] == (
        "       11     2       1.000000       1.500000       0.250000       4.000000       4.500000")


def test_stations_text_and_summary():
    win, names, res, fit, ts, as_ = _text_inputs()
    # station 1: windows 11 and 15 (12 has no cell), equal precisions: mean (0.125 + 0.75) / 2, se 0.5 / sqrt 2, rms sqrt((0.125^2 + 0.75^2) / 2);
    # amplitudes: p = 64 and 4: mean (64 * -0.25 + 4 * 1.5) / 68, se 1 / sqrt 68.  Station 2: window 11 alone
    st = lc.station_statistics(win, res, ts, as_)
    assert list(st["n"]) == [2, 1]
    assert st["mean"][0, 0] == 0.4375 and st["mean"][1, 0] == (64 * -0.25 + 4 * 1.5) / 68 and st["mean"][0, 1] == -0.125 and st["mean"][1, 1] == 0.25
    assert st["se"][0, 0] == 1.0 / np.sqrt(8.0) and st["se"][1, 1] == 0.25
    assert list(st["zmax"][:, 0]) == [1.0, 4.0] and list(st["zwin"][:, 0]) == [15, 11] and list(st["zwin"][:, 1]) == [11, 11]
    text = lc.stations_text(win, names, res, ts, as_).split("\n")
    assert text[0] == lc.STATIONS_HEADER and len(text) == 4 and text[3] == ""
    assert text[1] == ("STA1             2       0.437500       0.353553       0.537645       1.0000       15"
                       "      -0.147059       0.121268       0.437237       4.0000       11")
    assert text[2] == ("LONGSTATION1     1      -0.125000       0.250000       0.125000       1.0000       11"
                       "       0.250000       0.250000       0.250000       2.0000       11")
    assert lc.stations_summary_text(win, names, res, ts, as_) == (
        "largest mean residual of a station over the located windows -- time: station STA1 0.437500 (1.24 standard errors, 2 windows); "
        "amplitude: station LONGSTATION123 0.250000 (1.00 standard errors, 1 windows)\n")
    # no window with a cell at all
    none = lc.stations_text(win[1:2], names, res[1:2], ts[1:2], as_[1:2]).split("\n")
    assert none[1] == "STA1             0" + ("            NaN" * 3 + "          NaN" + "       -1") * 2


# ---- the program's arguments ---------------------------------------------------------------------------------------------------
def test_residuals_with_draws_is_an_argument_error(capsys):
    with pytest.raises(SystemExit) as e:
        lc.main(["hypo.in", "--cell", "5", "--residuals", "--draws", "4"])
    assert e.value.code == 2
    assert "--residuals takes a fixed structure" in capsys.readouterr().err


# ---- the entry point without a device ------------------------------------------------------------------------------------------
def test_null_handle_is_refused():
    lib = _lib.load()
    v = np.zeros(16)
    p = _lib.ptr
    assert lib.htm_forward_locate_residuals(None, p(v), 3.0, p(v), 250.0, p(v), None, None, None, p(v), p(v)) == -1
    assert lib.htm_last_error().decode() == "NULL handle"


def test_the_named_views_are_the_columns_of_fit():
    assert lc.FIT_NAMES == ("m_t_best", "m_t_mean", "m_t_sd", "chi2_t_best", "chi2_t_mean", "m_a_best", "m_a_mean", "m_a_sd", "chi2_a_best", "chi2_a_mean")
