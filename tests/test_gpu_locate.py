"""GPU: htm_forward_locate (hypotremormcmc_amd/csrc/htm_locate.hpp) against the oracle and the numpy restatement
(tests/locate_restatement.py), at the smallest shapes at which the kernels can go wrong.

The volume is pinned to the oracle cell by cell: |lp_gpu - lp_ref| <= RTOL_L * A, A the restatement's sum of the absolute
values of the cell's terms (a cell where the term crosses zero is not judged by cancellation).  The summaries are pinned to
the restatement applied to the device's OWN volume, which separates the reduce from the evaluation: sums of positive weights
(marginals), the log evidence and the variances to 1e-12 relative; a mean to 1e-12 of sum_i m_i |x_i| (its own absolute terms:
|mean| itself wherever the posterior's coordinates have one sign); a mixed moment c_ij, a sum of signed terms, to
1e-12 sd_i sd_j (Cauchy-Schwarz) plus 8 epsilon (X_i sd_j + X_j sd_i), X the axis' largest |coordinate|: the header's contract
for the rows' T_r - mean_x S_r."""
import math
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from hypotremormcmc_amd.forward import Forward, ObsArrays
from tests import locate_cases as cases
from tests import locate_restatement as lr

pytestmark = pytest.mark.gpu

RTOL_L = 1e-12
MIXED_EPS = 8 * np.finfo(float).eps      # the contract of a mixed moment (include/htm_hip.h): 8 epsilon (X_i sd_j + X_j sd_i) on top


def forward_of(sta, obs, use=(True, True)):
    E, S = obs[0].shape
    return Forward(S, E, sta[0], sta[1], sta[2], ObsArrays(*obs), use_time=use[0], use_amp=use[1])


def run(c, prior, **kw):
    fwd = forward_of(c["sta"], c["obs"], c["use"])
    try:
        tc, vs, ac, qs = c["structure"]
        return lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=prior, volume=True, **kw)
    finally:
        fwd.close()


def check_volume(vol, ref, ab, what):
    """same NaN / -inf pattern, and every other cell within RTOL_L of the sum of the absolute values of its terms"""
    assert vol.shape == ref.shape
    assert np.array_equal(np.isnan(vol), np.isnan(ref)), what
    assert np.array_equal(np.isneginf(vol), np.isneginf(ref)), what
    fin = np.isfinite(ref)
    assert np.isfinite(vol[fin]).all(), what
    ratio = np.abs(vol[fin] - ref[fin]) / ab[fin]
    print(f"{what}: {fin.sum()} cells, worst |lp_gpu - lp_ref| / A = {ratio.max() if ratio.size else 0.0:.3e}")
    assert np.all(ratio <= RTOL_L), (what, ratio.max())


def check_summaries(res, grid, ref_vol=None, ell_vol=None, ell_abs=None):
    """loc and the marginals against the restatement applied to the device's own volume (a marginal entry made of weights in
    the subnormal range, below 1e-300, is held to no relative bound); the best index also against the restatement's own volume
    where that has a clear best cell; the best cell's log-likelihood term against the oracle's, by the volume's criterion"""
    axes = [lr.centres(grid, a) for a in range(3)]
    for e, vol in enumerate(res["vol"]):
        s = lr.summarise(vol, grid)
        assert res["index"][e] == s["index"], e
        marg = (res["marg_x"][e], res["marg_y"][e], res["marg_z"][e])
        if s["index"] < 0:
            assert np.isnan(res["loc"][e, 1:]).all() and all(np.isnan(m).all() for m in marg), e
            continue
        assert not np.isnan(res["loc"][e]).any()
        assert np.array_equal(res["best"][e], s["best"]) and res["lp"][e] == s["lp"], e
        assert res["lp"][e] == vol.reshape(-1)[s["index"]]
        assert abs(res["log_evidence"][e] - s["log_evidence"]) <= 1e-12 * abs(s["log_evidence"]), e
        for a in range(3):
            assert np.allclose(marg[a], s["marg"][a], rtol=1e-12, atol=1e-300), (e, a)
            assert abs(marg[a].sum() - 1.0) <= 1e-13, (e, a)
            assert abs(res["mean"][e, a] - s["mean"][a]) <= 1e-12 * s["mean_abs"][a], (e, a)
            span2 = (axes[a][-1] - axes[a][0]) ** 2             # (weights below 1e-300, as for the marginals)
            assert abs(res["cov"][e, a, a] - s["cov"][a, a]) <= 1e-12 * s["cov"][a, a] + 1e-300 * span2, (e, a, res["cov"][e, a, a], s["cov"][a, a])
        sd, big = np.sqrt(np.diag(s["cov"])), np.array([np.abs(ax).max() for ax in axes])
        tol = 1e-12 * np.outer(sd, sd) + MIXED_EPS * (np.outer(big, sd) + np.outer(sd, big))
        assert np.all(np.abs(res["cov"][e] - s["cov"]) <= tol), (e, res["cov"][e], s["cov"])
        if ref_vol is not None:
            r = lr.summarise(ref_vol[e], grid)
            assert r["index"] < 0 or r["lp"] - r["second"] > 1e-9, e      # (a clear best cell: no window is left out)
            assert res["index"][e] == r["index"], e
        if ell_vol is not None:
            assert abs(res["ell"][e] - ell_vol[e].reshape(-1)[s["index"]]) <= RTOL_L * ell_abs[e].reshape(-1)[s["index"]], e


# ---- parity with the oracle, cell by cell, and the summaries ------------------------------------------------------------
@pytest.mark.parametrize("mode", ["both", "time", "amp"])
@pytest.mark.parametrize("grid_name", ["1x1x1", "5x3x2", "67x3x5"])
@pytest.mark.parametrize("n_events", [1, 5])
@pytest.mark.parametrize("n_sta", [3, 64, 65])
def test_volume_and_summaries_match_the_oracle(n_sta, n_events, grid_name, mode):
    c = cases.parity_case(n_sta, n_events, grid_name, mode)
    what = f"{n_sta} stations, {n_events} events, {grid_name}, {mode}"
    flat = run(c, None)
    check_volume(flat["vol"], c["ell"], c["abs"], what + ", flat")
    check_summaries(flat, c["grid"], c["ell"], c["ell"], c["abs"])
    assert np.array_equal(flat["ell"], flat["lp"])                     # a flat prior: lp is the term itself
    pri = run(c, c["prior"])
    check_volume(pri["vol"], c["lp_prior"], c["abs_prior"], what + ", prior")
    check_summaries(pri, c["grid"], c["lp_prior"], c["ell"], c["abs"])


@pytest.mark.parametrize("grid_name,n_sta,mode", [("70x60x2", 5, "both"), ("300x3x1", 4, "both"), ("70x60x2", 3, "time")])
def test_tiles_of_many_cells_rows_and_ragged_ends(grid_name, n_sta, mode):
    """a thread owns up to 16 cells in four chunks; two tiles per layer, the second with 2 of 58 rows; a row longer than a
    workgroup: one event, volume and summaries as above"""
    c = cases.parity_case(n_sta, 1, grid_name, mode)
    for prior, key, ab in ((None, "ell", "abs"), (c["prior"], "lp_prior", "abs_prior")):
        res = run(c, prior)
        check_volume(res["vol"], c[key], c[ab], f"{grid_name}, {n_sta} stations, {mode}, {key}")
        check_summaries(res, c["grid"], c[key], c["ell"], c["abs"])


def test_missing_data_rule():
    c = cases.missing_case()
    assert (c["obs"][1] == 0.0).sum() >= 3                              # the fixture's missing entries are among these events
    for prior, key in ((None, "ell"), (c["prior"], "lp_prior")):
        res = run(c, prior)
        check_volume(res["vol"], c[key], c["abs"] if prior is None else c["abs_prior"], "missing fixture")
        check_summaries(res, c["grid"], c[key], c["ell"], c["abs"])


def test_excluded_cells_match_exactly():
    """a cell centre on a station (NaN), a lowest layer at z0 and below it (-inf), an event with no cell left (-1 and NaN)"""
    c = cases.excluded_case()
    res = run(c, c["prior"])
    check_volume(res["vol"], c["lp_prior"], c["abs_prior"], "excluded")
    check_summaries(res, c["grid"], c["lp_prior"])
    assert list(res["index"] >= 0) == [True, True, False]
    assert np.isnan(res["vol"][0, 0, 1, 1]) and np.isneginf(res["vol"][0, 0]).sum() == 14
    flat = run(c, None)
    check_volume(flat["vol"], c["ell"], c["abs"], "excluded, flat")
    assert np.isnan(flat["vol"][:, 0, 1, 1]).all() and (flat["index"] >= 0).all()


# ---- degenerate events --------------------------------------------------------------------------------------------------
def test_event_without_a_cell_leaves_its_neighbours_untouched():
    c = cases.parity_case(64, 5, "67x3x5", "both")
    ref = run(c, c["prior"])
    prior = c["prior"].copy()
    prior[2, 3] = 100.0                                                  # z0 above every centre: no cell of event 2 is left
    res = run(c, prior)
    assert res["index"][2] == -1 and np.isnan(res["loc"][2, 1:]).all() and np.isneginf(res["vol"][2]).all()
    assert np.isnan(res["marg_x"][2]).all() and np.isnan(res["marg_y"][2]).all() and np.isnan(res["marg_z"][2]).all()
    keep = [0, 1, 3, 4]
    for key in ("loc", "marg_x", "marg_y", "marg_z", "vol"):
        assert np.array_equal(res[key][keep], ref[key][keep]), key


def test_weights_that_underflow_leave_one_cell():
    """standard deviations so small that every weight but the best cell's underflows: marginals exactly 1 there, no NaN"""
    c = cases.parity_case(64, 5, "67x3x5", "both")
    t_obs, t_stdv, a_obs, a_stdv = (o.copy() for o in c["obs"])
    t_stdv[1], a_stdv[1] = 1e-7, 1e-7
    res = run(dict(c, obs=(t_obs, t_stdv, a_obs, a_stdv)), c["prior"])
    assert not np.isnan(res["loc"]).any() and np.isfinite(res["vol"][1]).all()
    i = res["index"][1]
    ix, iy, iz = i % 67, (i // 67) % 3, i // 201
    for m, k in ((res["marg_x"][1], ix), (res["marg_y"][1], iy), (res["marg_z"][1], iz)):
        want = np.zeros(m.size)
        want[k] = 1.0
        assert np.array_equal(m, want)
    assert np.array_equal(res["mean"][1], res["best"][1]) and np.array_equal(res["cov"][1], np.zeros((3, 3)))
    assert abs(res["log_evidence"][1] - (res["lp"][1] + math.log(1.3 * 14.0 * 3.1))) <= 2 * np.spacing(abs(res["lp"][1]))


def test_tied_cells_give_the_lowest_index():
    """two stations mirrored in x = 0 with the same observations, 4 x 1 x 1 cells mirrored too: cells 1 and 2 tie bit for bit"""
    sta = (np.array([-10.0, 10.0]), np.array([3.0, 3.0]), np.array([0.5, 0.5]))
    one = np.ones((1, 2))
    obs = (0.0 * one, 0.1 * one, -2.0 * one, 0.05 * one)
    fwd = forward_of(sta, obs)
    res = lc.locate(fwd, np.zeros(2), 3.0, np.zeros(2), 250.0, [-2.0, 1.0, 4, 2.5, 1.0, 1, 7.0, 1.0, 1], volume=True)
    fwd.close()
    v = res["vol"][0].reshape(-1)
    assert v[1] == v[2] and v[0] == v[3] and v[1] > v[0]
    assert res["index"][0] == 1 and res["best"][0, 0] == -0.5
    assert res["marg_x"][0][1] == res["marg_x"][0][2] and abs(res["mean"][0, 0]) < 1e-15


# ---- determinism and batching ----------------------------------------------------------------------------------------------
def test_two_calls_and_every_batching_give_the_same_bits(monkeypatch):
    c = cases.parity_case(65, 5, "67x3x5", "both")
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    first = run(c, c["prior"])
    again = run(c, c["prior"])
    monkeypatch.setenv("HTM_LOCATE_MB", "0.02")          # an event's workspace is 17.3 KiB: one fits -- five batches of one event
    single = run(c, c["prior"])
    monkeypatch.setenv("HTM_LOCATE_MB", "0.04")          # two fit: batches of 2, 2, 1
    pairs = run(c, c["prior"])
    for other in (again, single, pairs):
        for key in ("loc", "marg_x", "marg_y", "marg_z", "vol"):
            assert np.array_equal(first[key], other[key], equal_nan=True), key
    monkeypatch.setenv("HTM_LOCATE_MB", "0")
    with pytest.raises(lc._lib.HtmError, match="HTM_LOCATE_MB"):
        run(c, None)


def test_argument_refusals_with_a_real_handle():
    """NULL arrays, a bad structure and a bad grid are HTM_EINVAL with a message (the NULL handle: tests/test_locate.py)"""
    c = cases.parity_case(3, 5, "5x3x2", "both")
    fwd = forward_of(c["sta"], c["obs"])
    lib, p = lc._lib.load(), lc._lib.ptr
    last = lambda: lib.htm_last_error().decode()
    v, good = np.zeros(5 * 16), np.array([0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2])

    def call(tc=v, vs=3.0, ac=v, qs=250.0, grid=good, loc=v):
        return lib.htm_forward_locate(fwd.handle, p(tc), vs, p(ac), qs, p(None if grid is None else np.array(grid, dtype=np.float64)), None, p(loc), None, None)

    try:
        assert call() == 0
        for kw in ({"tc": None}, {"ac": None}, {"grid": None}, {"loc": None}):
            assert call(**kw) == -1 and last() == "NULL argument", kw
        for kw in ({"vs": 0.0}, {"vs": -1.0}, {"vs": float("nan")}, {"vs": float("inf")}, {"qs": 0.0}, {"qs": float("nan")}):
            assert call(**kw) == -1 and "need finite values > 0" in last(), kw
        bad = lambda i, val: [val if k == i else g for k, g in enumerate(good)]
        for i, val, msg in ((1, 0.0, "cell size"), (4, -1.0, "cell size"), (0, float("inf"), "origin"), (2, 0.0, "cells"), (5, 2.5, "cells"),
                            (8, 4097.0, "cells"), (7, float("nan"), "cell size")):
            assert call(grid=bad(i, val)) == -1 and msg in last(), (i, val)
        assert call(grid=[0.0, 1.0, 4096, 0.0, 1.0, 4096, 0.0, 1.0, 128]) == -1 and "more than 2^31 - 1" in last()
    finally:
        fwd.close()


def test_prior_widths_are_checked():
    c = cases.parity_case(3, 5, "5x3x2", "both")
    for col, val in ((2, 0.0), (4, -1.0), (2, float("nan"))):
        prior = c["prior"].copy()
        prior[3, col] = val
        with pytest.raises(lc._lib.HtmError, match="event 3: prior widths"):
            run(c, prior)


# ---- noise-free recovery ---------------------------------------------------------------------------------------------------
def test_noise_free_recovery_on_the_device():
    rec = cases.recovery_case()
    fwd = forward_of(rec["sta"], rec["obs"])
    res = lc.locate(fwd, *rec["structure"], rec["grid"])
    fwd.close()
    assert list(res["index"]) == list(rec["index"]) and np.array_equal(res["best"], rec["truth"])
    assert res["vol"] is None and res["marg_x"].shape == (6, 10)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(tmp_path, capsys):
    data = cases.e2e_data()
    d = str(tmp_path)
    synth.write_dataset(d, data)
    synth.write_param_file(os.path.join(d, "hypo.in"))
    cases.write_structure(d, ["S%03d" % (j + 1) for j in range(16)], np.zeros(16), np.zeros(16), vs=3.0, qs=250.0)
    lc.main([os.path.join(d, "hypo.in"), "--cell"] + [str(v) for v in cases.E2E_CELL] + ["--bounds"] + [str(v) for v in cases.E2E_BOUNDS]
            + ["--volume-of", "3"])
    ref = cases.e2e_reference()
    want = lr.stat_text(data.win_id, ref["quant"]).split("\n")
    got = open(os.path.join(d, "hypo_grid.stat")).read().split("\n")
    assert len(got) == len(want) == 10 and got[0] == want[0]
    quant = np.empty((8, 3, 3))
    for e, (g, w) in enumerate(zip(got[1:9], want[1:9])):
        assert len(g) == len(w) == 9 + 9 * 13 and g[:9] == w[:9], e
        for k in range(9):          # a field may differ by one unit in its last printed decimal
            a, b = g[9 + 13 * k:22 + 13 * k], w[9 + 13 * k:22 + 13 * k]
            assert a == b or abs(round(float(a) * 1e6) - round(float(b) * 1e6)) <= 1, (e, k, a, b)
        v = [float(x) for x in g[9:].split()]
        quant[e] = [[v[3 * a + 1], v[3 * a], v[3 * a + 2]] for a in range(3)]
    inside = (quant[:, :, 0] <= data.ev_xyz) & (data.ev_xyz <= quant[:, :, 2])
    assert np.all(inside.sum(axis=1) >= 2), inside
    best = open(os.path.join(d, "hypo_grid.best.dat")).read().split("\n")
    assert best[0] == lc.BEST_HEADER and len(best) == 10 and [int(ln.split()[0]) for ln in best[1:9]] == list(data.win_id)
    n = lr.counts(ref["grid"])
    vol = open(os.path.join(d, "hypo_grid.3.vol.dat")).read().split("\n")
    assert len(vol) == n[0] * n[1] * n[2] + 2 and vol[1].split()[0] == "0"
    out = capsys.readouterr().out.split("\n")
    assert out[0] == f"8 windows located on {n[0]} x {n[1]} x {n[2]} cells" and out[1].endswith("0 without an included cell") and len(out) == 3
