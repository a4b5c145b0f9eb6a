"""GPU: htm_forward_locate_residuals (k_locate_res_best, k_locate_residuals, k_locate_res_combine in
hypotremormcmc_amd/csrc/htm_locate.hpp) against the numpy restatement of its rule
(tests/locate_residuals_restatement.py), at the smallest shapes at which the kernels can go wrong.

The moments are pinned as tests/test_gpu_locate.py pins its summaries: `locate.locate(..., volume=True)` gives the device's own
volume, the residual call's loc must equal that call's bitwise, and the restatement is applied to that volume -- which separates
the residual pass from the evaluation of the posterior.  The bounds (the restatement's `bounds`): res and the offsets to 1e-12 of
the posterior mean, about the best cell, of their absolute terms; chi2 to 1e-12 of sum_j p_j |rho_j| X_j; the offset's variance
to 1e-12 of itself plus 8 epsilon Xbar sd; with the single-precision forward each widened by U 2^-24 of the same sums over the
synthetics' scales, U = 4 of tests/locate_fp32_restatement.py (the variance by that file's own propagation, 2 sd delta + delta^2);
the fit identity between loc[5] and chi2(best) is held to RTOL_L of abs_terms in both precisions, unwidened.  tests/test_locate_residuals.py holds the restatement itself to
them, fp64 against numpy.longdouble, on the same cases."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from hypotremormcmc_amd.forward import Forward, ObsArrays
from tests import locate_cases as cases
from tests import locate_fp32_restatement as l32
from tests import locate_residuals_cases as rc
from tests import locate_residuals_restatement as rr

pytestmark = pytest.mark.gpu

RTOL_L = 1e-12
KEYS = ("loc", "marg_x", "marg_y", "marg_z", "res", "fit")


def forward_of(c):
    E, S = c["obs"][0].shape
    return Forward(S, E, c["sta"][0], c["sta"][1], c["sta"][2], ObsArrays(*c["obs"]), use_time=c["use"][0], use_amp=c["use"][1])


def both_calls(c, prior, precision=None):
    """(locate with its volume, residuals) of one Forward"""
    fwd = forward_of(c)
    try:
        tc, vs, ac, qs = c["structure"]
        return (lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=prior, volume=True, precision=precision),
                lc.residuals(fwd, tc, vs, ac, qs, c["grid"], prior=prior, precision=precision))
    finally:
        fwd.close()


def check(c, prior, what, precision=None, ulps=0):
    plain, res = both_calls(c, prior, precision)
    for key in ("loc", "marg_x", "marg_y", "marg_z"):
        assert np.array_equal(plain[key], res[key], equal_nan=True), (what, key)
    assert res["vol"] is None
    r = rr.restate(c["sta"], c["obs"], c["use"], c["structure"], c["grid"], plain["vol"])
    assert np.array_equal(r["index"], res["index"]), what
    worst = rr.compare(res["res"], res["fit"], r, c["use"], ulps=ulps, what=what)
    print(f"{what}: worst |gpu - restated| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    # the named views
    assert np.array_equal(res["res_t_mean"], res["res"][:, :, 1], equal_nan=True) and np.array_equal(res["chi2_a_best"], res["fit"][:, 8], equal_nan=True)
    # the fit identity: the best cell's log-likelihood term from chi2 and the constants.  In either precision: with the fp32 forward
    # k_locate's term and the pass's chi2 are made of the same single-precision synthetics, so the two differ by fp64 rounding alone
    worst_id = 0.0
    for e in range(res["loc"].shape[0]):
        if res["index"][e] < 0:
            continue
        _, _, ct, ca = rr.precisions(c["obs"], e)
        term = sum(-0.5 * res["fit"][e, 5 * d + 3] - k for d, k in enumerate((ct, ca)) if c["use"][d])
        ab = c["abs"][e].reshape(-1)[res["index"][e]]
        worst_id = max(worst_id, abs(res["loc"][e, 5] - term) / ab)
        assert abs(res["loc"][e, 5] - term) <= RTOL_L * ab, (what, e, res["loc"][e, 5], term)
    print(f"{what}: worst |loc[5] - (-chi2(best) / 2 - constants)| / abs_terms = {worst_id:.3e}")
    return plain, res


@pytest.mark.parametrize("key", rc.PARITY, ids=rc.case_id)
def test_residuals_and_fit_match_the_restatement(key):
    c = rc.case(key)
    flat, res = check(c, None, rc.case_id(key) + ", flat")
    check(c, c["prior"], rc.case_id(key) + ", prior")
    if key[2] == "1x1x1":       # a posterior of one cell: the means are the best cell's values bitwise, the spread is 0
        assert np.array_equal(res["res"][:, :, 0::2], res["res"][:, :, 1::2], equal_nan=True)
        for d in range(2):
            if c["use"][d]:
                f = res["fit"][:, 5 * d:5 * d + 5]
                assert np.array_equal(f[:, 0], f[:, 1]) and np.array_equal(f[:, 3], f[:, 4]) and np.all(f[:, 2] == 0.0)


@pytest.mark.parametrize("key", rc.LARGE, ids=rc.case_id)
def test_several_blocks_of_cells_and_a_ragged_last_one(key):
    c = rc.case(key)
    check(c, None, rc.case_id(key) + ", flat")
    check(c, c["prior"], rc.case_id(key) + ", prior")


def test_missing_data_rule():
    c = rc.case("missing")
    assert (c["obs"][1] == 0.0).sum() >= 3
    check(c, None, "missing fixture, flat")
    check(c, c["prior"], "missing fixture, prior")


def test_excluded_cells_enter_by_selection():
    """a cell centre on a station (its amplitude residual is infinite), a lowest layer at z0, an event with no cell left"""
    c = rc.case("excluded")
    _, res = check(c, c["prior"], "excluded, prior")
    assert list(res["index"] >= 0) == [True, True, False]
    assert np.isfinite(res["res"][:2]).all() and np.isfinite(res["fit"][:2]).all() and np.isnan(res["res"][2]).all() and np.isnan(res["fit"][2]).all()
    _, flat = check(c, None, "excluded, flat")
    assert np.isfinite(flat["res"]).all() and np.isfinite(flat["fit"]).all()


@pytest.mark.parametrize("key", rc.FP32_CASES, ids=rc.case_id)
def test_single_precision_forward(key):
    c = rc.case(key)
    plain, res = check(c, c["prior"], rc.case_id(key) + ", fp32", precision="fp32", ulps=l32.U)
    _, res64 = both_calls(c, c["prior"])
    assert not np.array_equal(res["res"], res64["res"])              # (the switch does switch)


def test_two_calls_and_every_batching_give_the_same_bits(monkeypatch):
    c = cases.parity_case(65, 5, "67x3x5", "both")
    for precision in ("fp64", "fp32"):
        monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
        plain, first = both_calls(c, c["prior"], precision)
        _, again = both_calls(c, c["prior"], precision)
        monkeypatch.setenv("HTM_LOCATE_MB", "0.03")          # an event's workspace is 22008 bytes: one fits (tests/test_locate_residuals_plan.py)
        _, single = both_calls(c, c["prior"], precision)
        monkeypatch.setenv("HTM_LOCATE_MB", "0.05")          # two fit: batches of 2, 2, 1
        _, pairs = both_calls(c, c["prior"], precision)
        for other in (again, single, pairs):
            for key in KEYS:
                assert np.array_equal(first[key], other[key], equal_nan=True), (precision, key)
        for key in ("loc", "marg_x", "marg_y", "marg_z"):
            assert np.array_equal(first[key], plain[key], equal_nan=True), (precision, key)


def test_argument_refusals_with_a_real_handle():
    c = cases.parity_case(3, 5, "5x3x2", "both")
    fwd = forward_of(c)
    lib, p = lc._lib.load(), lc._lib.ptr
    last = lambda: lib.htm_last_error().decode()
    v, good = np.zeros(5 * 16), np.array([0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2])
    res, fit = np.zeros((5, 3, 4)), np.zeros((5, 10))

    def call(tc=v, vs=3.0, ac=v, qs=250.0, grid=good, loc=v, res=res, fit=fit):
        return lib.htm_forward_locate_residuals(fwd.handle, p(tc), vs, p(ac), qs, p(grid), None, p(loc), None, p(res), p(fit))

    try:
        assert call() == 0 and call(loc=None) == 0
        for kw in ({"tc": None}, {"ac": None}, {"grid": None}):
            assert call(**kw) == -1 and last() == "NULL argument", kw
        for kw in ({"res": None}, {"fit": None}):
            assert call(**kw) == -1 and last() == "NULL output: res and fit are required", kw
        for kw in ({"vs": 0.0}, {"qs": float("nan")}):
            assert call(**kw) == -1 and "need finite values > 0" in last(), kw
        bad = good.copy()
        bad[1] = 0.0
        assert call(grid=bad) == -1 and "cell size" in last()
    finally:
        fwd.close()


# ---- the program, end to end -----------------------------------------------------------------------------------------------------
def test_program_end_to_end(tmp_path, capsys):
    """cases.e2e_data() (seed 2: 8 windows, 16 stations, made with the structure they are located under, no outlier): the three
    files exist and parse, hypo_grid.stat and hypo_grid.best.dat are byte for byte those of the run without --residuals, and
    every station's weighted mean residual lies within 3 of its standard errors of 0.  The grid has 1 km cells, not the 5 x 5 x 2 km
    of cases.E2E_CELL: there a cell centre lies up to 2.5 km from the window, 0.8 s of travel time against a noise of 0.1 s, and the
    criterion measures the grid, not the data -- on the restatement alone the largest |mean| / standard error is 4.74 at seed 2
    (5.51 and 5.70 at seeds 9 and 10); with 1 km cells it is 2.48 at seed 2 (2.06 and 2.24), and 2.48 still with 0.5 km cells.
    Seed 2 is used."""
    data = cases.e2e_data()
    names = ["S%03d" % (j + 1) for j in range(16)]
    out = {}
    for how, extra in (("plain", []), ("residuals", ["--residuals"])):
        d = str(tmp_path / how)
        os.mkdir(d)
        synth.write_dataset(d, data)
        synth.write_param_file(os.path.join(d, "hypo.in"))
        cases.write_structure(d, names, np.zeros(16), np.zeros(16), vs=3.0, qs=250.0)
        lc.main([os.path.join(d, "hypo.in"), "--cell", "1", "1", "1", "--bounds"] + [str(v) for v in cases.E2E_BOUNDS] + extra)
        out[how] = (d, capsys.readouterr().out)
    d0, d1 = out["plain"][0], out["residuals"][0]
    for name in ("hypo_grid.stat", "hypo_grid.best.dat"):
        assert open(os.path.join(d0, name), "rb").read() == open(os.path.join(d1, name), "rb").read(), name
    assert not os.path.exists(os.path.join(d0, "hypo_grid.fit.dat"))
    assert out["residuals"][1].startswith(out["plain"][1]) and out["residuals"][1][len(out["plain"][1]):].startswith("largest mean residual of a station")
    rows = [ln.split() for ln in open(os.path.join(d1, "hypo_grid.residuals.dat")).read().split("\n")[1:-1]]
    assert len(rows) == 8 * 16 and all(len(r) == 9 for r in rows) and [r[1] for r in rows[:16]] == names
    assert [int(r[0]) for r in rows[::16]] == list(data.win_id) and np.isfinite(np.array([[float(x) for x in r[3:]] for r in rows])).all()
    fit = [ln.split() for ln in open(os.path.join(d1, "hypo_grid.fit.dat")).read().split("\n")[1:-1]]
    assert len(fit) == 8 and all(len(r) == 13 and int(r[1]) == 16 for r in fit)
    assert all(float(r[4]) >= 0.0 and float(r[9]) >= 0.0 and float(r[12]) == pytest.approx(-float(r[8]), abs=1.1e-6) for r in fit)
    sta = [ln.split() for ln in open(os.path.join(d1, "hypo_grid.stations.dat")).read().split("\n")[1:-1]]
    assert len(sta) == 16 and [r[0] for r in sta] == names and all(int(r[1]) == 8 for r in sta)
    for r in sta:
        for k in (2, 7):          # mean and standard error, per data type
            assert abs(float(r[k])) <= 3.0 * float(r[k + 1]), r
