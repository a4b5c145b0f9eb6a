"""GPU: htm_forward_locate_marginal (k_locate_marginal in hypotremormcmc_amd/csrc/htm_locate.hpp) against numpy's
log-mean-exp over the oracle's volume of every draw (tests/locate_marginal_cases.py), at the smallest shapes at which the
kernel can go wrong: draw counts on both sides of every power-of-two block up to 32, one draw that dominates (wide) and
several that share the weight (tight), ragged tiles, excluded cells.

The volume is pinned cell by cell: the same NaN / -inf pattern, and |lp_gpu - lp_ref| <= 1e-12 A elsewhere, A the largest sum
of the absolute values of the cell's terms among the draws (the log-sum-exp adds a few epsilon of |m| <= A to what
tests/test_gpu_locate.py allows one draw).  The summaries are pinned as there, to the restatement applied to the device's own
volume.  The worst ratio over every case of this file was 9.1e-15 (it is printed per case)."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from tests import locate_cases as cases
from tests import locate_marginal_cases as mc
from tests import locate_restatement as lr
from tests.test_gpu_locate import check_summaries, check_volume, forward_of

pytestmark = pytest.mark.gpu


def run(c, prior, draws=None, **kw):
    fwd = forward_of(c["sta"], c["obs"], c["use"])
    try:
        tc, vs, ac, qs = c["draws"] if draws is None else draws
        return lc.locate_marginal(fwd, tc, vs, ac, qs, c["grid"], prior=prior, volume=True, **kw)
    finally:
        fwd.close()


def run_fixed(c, prior, structure):
    fwd = forward_of(c["sta"], c["obs"], c["use"])
    try:
        tc, vs, ac, qs = structure
        return lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=prior, volume=True)
    finally:
        fwd.close()


def same_bits(a, b):
    for key in ("loc", "marg_x", "marg_y", "marg_z", "vol"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


# ---- parity with the reference, cell by cell, and the summaries -----------------------------------------------------------
# every K and every mode with both sets on the 30-cell grid; the larger grids, 65 stations and two events thinned
PARITY = ([((3, 1, "5x3x2", mode), K) for mode in ("both", "time", "amp") for K in mc.KS]
          + [((65, 2, "67x3x5", "both"), K) for K in (8, 9)]
          + [((65, 1, "1x1x1", "time"), 33), ((65, 1, "1x1x1", "amp"), 17), ((65, 1, "1x1x1", "both"), 2), ((3, 1, "1x1x1", "both"), 1),
             ((3, 1, "67x3x5", "time"), 7), ((3, 1, "67x3x5", "amp"), 2), ((65, 1, "5x3x2", "amp"), 33), ((65, 1, "5x3x2", "time"), 1)])


@pytest.mark.parametrize("which", ["wide", "tight"])
@pytest.mark.parametrize("key,K", PARITY, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_volume_and_summaries_match_the_reference(key, K, which):
    c = mc.marginal_case(key, K, which)
    what = f"{key}, K = {K}, {which}"
    flat = run(c, None)
    check_volume(flat["vol"], c["ell"], c["abs"], what + ", flat")
    check_summaries(flat, c["grid"], None, c["ell"], c["abs"])
    assert np.array_equal(flat["ell"], flat["lp"])                     # a flat prior: lp is the term itself
    pri = run(c, c["prior"])
    check_volume(pri["vol"], c["lp_prior"], c["abs_prior"], what + ", prior")
    check_summaries(pri, c["grid"], None, c["ell"], c["abs"])


@pytest.mark.parametrize("grid_name,n_sta", [("70x60x2", 5), ("300x3x1", 4)])
def test_tiles_of_many_cells_rows_and_ragged_ends(grid_name, n_sta):
    """two tiles per layer, the second with 2 of 58 rows, a thread with up to 16 cells; a row longer than a workgroup"""
    c = mc.marginal_case((n_sta, 1, grid_name, "both"), 9, "tight")
    for prior, key, ab in ((None, "ell", "abs"), (c["prior"], "lp_prior", "abs_prior")):
        res = run(c, prior)
        check_volume(res["vol"], c[key], c[ab], f"{grid_name}, {n_sta} stations, K = 9, tight, {key}")
        check_summaries(res, c["grid"], None, c["ell"], c["abs"])


# ---- one draw, equal draws ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(3, 1, "5x3x2", "both"), (5, 1, "70x60x2", "both")])
def test_one_draw_is_htm_forward_locate(key):
    c = cases.parity_case(*key)
    tc, vs, ac, qs = c["structure"]
    for prior in (None, c["prior"]):
        same_bits(run(c, prior, draws=(tc[None], [vs], ac[None], [qs])), run_fixed(c, prior, c["structure"]))


@pytest.mark.parametrize("K", [5, 9])
@pytest.mark.parametrize("key", [(3, 1, "5x3x2", "both"), (65, 2, "67x3x5", "both")])
def test_equal_draws_are_one_draw(key, K):
    c = cases.parity_case(*key)
    tc, vs, ac, qs = c["structure"]
    one = run_fixed(c, c["prior"], c["structure"])
    same_bits(run(c, c["prior"], draws=(np.tile(tc, (K, 1)), np.full(K, vs), np.tile(ac, (K, 1)), np.full(K, qs))), one)


# ---- excluded cells -------------------------------------------------------------------------------------------------------
def test_excluded_cells_match_exactly():
    """a cell centre on a station is NaN under every draw, a lowest layer at z0 and below is -inf; an event with no cell left
    gives -1 and NaN and leaves its neighbours untouched"""
    c = mc.marginal_case("excluded", 3, "tight")
    res = run(c, c["prior"])
    check_volume(res["vol"], c["lp_prior"], c["abs_prior"], "excluded, K = 3")
    check_summaries(res, c["grid"])
    assert list(res["index"] >= 0) == [True, True, False]
    assert np.isnan(res["vol"][0, 0, 1, 1]) and np.isneginf(res["vol"][0, 0]).sum() == 14
    assert np.isnan(res["loc"][2, 1:]).all() and np.isnan(res["marg_x"][2]).all() and not lr.included(res["vol"][2]).any()
    prior = c["prior"].copy()
    prior[2, 3] = -1.0                                                   # event 2 gets its cells back: events 0 and 1 keep their bits
    other = run(c, prior)
    assert other["index"][2] >= 0
    for key in ("loc", "marg_x", "marg_y", "marg_z", "vol"):
        assert np.array_equal(res[key][:2], other[key][:2], equal_nan=True), key
    flat = run(c, None)
    check_volume(flat["vol"], c["ell"], c["abs"], "excluded, K = 3, flat")
    assert np.isnan(flat["vol"][:, 0, 1, 1]).all() and (flat["index"] >= 0).all()


# ---- the evidence of the mixture is the mixture of the evidences ----------------------------------------------------------
@pytest.mark.parametrize("which", ["wide", "tight"])
def test_evidence_identity(which):
    """sum over cells and mean over draws commute: log_evidence = logsumexp_k(log_evidence of htm_forward_locate under draw k)
    - log K, to the sum of the two sides' bounds (1e-12 A each)"""
    c = mc.marginal_case((3, 1, "5x3x2", "both"), 7, which)
    tc, vs, ac, qs = c["draws"]
    got = run(c, c["prior"])["log_evidence"]
    per = np.stack([run_fixed(c, c["prior"], (tc[k], vs[k], ac[k], qs[k]))["log_evidence"] for k in range(7)])
    want = mc.mixture(per)
    A = np.max(c["abs_prior"][np.isfinite(c["abs_prior"])])
    print(f"evidence identity, {which}: |difference| / A = {np.max(np.abs(got - want)) / A:.3e}")
    assert np.all(np.abs(got - want) <= 2e-12 * A)


# ---- determinism and batching ---------------------------------------------------------------------------------------------
def test_two_calls_and_every_batching_give_the_same_bits(monkeypatch):
    c = dict(cases.parity_case(65, 5, "67x3x5", "both"))
    c["draws"] = mc.draws(65, 7 * 65 + 5, "tight", 9)
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    first = run(c, c["prior"])
    again = run(c, c["prior"])
    # an event's workspace is 17.3 KiB, the draws' table and its input 25.8 KiB (blocks of 8 draws; 18.6 .. 25.8 KiB with blocks
    # of 1 .. 16): 51.2 KiB hold the table and one event, not two -- five batches of one event
    monkeypatch.setenv("HTM_LOCATE_MB", "0.05")
    single = run(c, c["prior"])
    monkeypatch.setenv("HTM_LOCATE_MB", "0.065")         # 66.6 KiB: the table and two events, not three: batches of 2, 2, 1
    pairs = run(c, c["prior"])
    for other in (again, single, pairs):
        same_bits(first, other)
    monkeypatch.setenv("HTM_LOCATE_MB", "0.03")          # 30.7 KiB: the table fits, an event with it does not
    with pytest.raises(lc._lib.HtmError, match="HTM_LOCATE_MB"):
        run(c, c["prior"])
    monkeypatch.setenv("HTM_LOCATE_MB", "0.01")          # less than the table
    with pytest.raises(lc._lib.HtmError, match="HTM_LOCATE_MB = 0.01: the table of 9 draws"):
        run(c, None)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_argument_refusals_with_a_real_handle():
    c = cases.parity_case(3, 5, "5x3x2", "both")
    fwd = forward_of(c["sta"], c["obs"])
    lib, p = lc._lib.load(), lc._lib.ptr
    last = lambda: lib.htm_last_error().decode()
    out, good = np.zeros(5 * 16), np.array([0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2])
    corr = np.zeros(4097 * 3)

    def call(K=3, tc=corr, vs=(3.0, 3.1, 3.2), ac=corr, qs=(250.0, 240.0, 260.0), grid=good, loc=out):
        f = lambda v: None if v is None else np.array(v, dtype=np.float64)
        return lib.htm_forward_locate_marginal(fwd.handle, K, p(tc), p(f(vs)), p(ac), p(f(qs)), p(f(grid)), None, p(loc), None, None)

    try:
        assert call() == 0
        for kw in ({"tc": None}, {"vs": None}, {"ac": None}, {"qs": None}, {"grid": None}, {"loc": None}):
            assert call(**kw) == -1 and last() == "NULL argument", kw
        big = np.full(4097, 3.0)
        for K in (0, -1, 4097):
            assert call(K=K, vs=big, qs=big) == -1 and last() == f"n_draws = {K}: need 1..4096", K
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(vs=(3.0, bad, 3.2)) == -1 and last().startswith("draw 1: vs = ") and "need finite values > 0" in last(), bad
        for bad in (0.0, -5.0, float("nan"), float("inf")):
            assert call(qs=(250.0, 240.0, bad)) == -1 and last().startswith("draw 2: vs = 3.2, qs = ") and "need finite values > 0" in last(), bad
        assert call(grid=[0.0, 0.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2]) == -1 and "cell size" in last()
        assert call(grid=[0.0, 1.0, 4096, 0.0, 1.0, 4096, 0.0, 1.0, 128]) == -1 and "more than 2^31 - 1" in last()
        assert call(K=4096, vs=big[:4096], qs=big[:4096] + 200.0) == 0
    finally:
        fwd.close()
    with pytest.raises(lc._lib.HtmError, match="event 3: prior widths"):
        prior = c["prior"].copy()
        prior[3, 2] = 0.0
        run(dict(c, draws=(np.zeros((2, 3)), [3.0, 3.1], np.zeros((2, 3)), [250.0, 240.0])), prior)
    with pytest.raises(ValueError, match="2 draws of vs"):
        run(dict(c, draws=(np.zeros((2, 3)), [3.0, 3.1], np.zeros((3, 3)), [250.0, 240.0])), None)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def stat_lines_agree(got, want):
    """a field may differ by one unit in its last printed decimal"""
    assert len(got) == len(want) == 10 and got[0] == want[0]
    for e, (g, w) in enumerate(zip(got[1:9], want[1:9])):
        assert len(g) == len(w) == 9 + 9 * 13 and g[:9] == w[:9], e
        for k in range(9):
            a, b = g[9 + 13 * k:22 + 13 * k], w[9 + 13 * k:22 + 13 * k]
            assert a == b or abs(round(float(a) * 1e6) - round(float(b) * 1e6)) <= 1, (e, k, a, b)


def test_program_end_to_end(tmp_path, capsys):
    from hypotremormcmc_amd.obs_data import ObsData

    data = cases.e2e_data()
    d, cal = str(tmp_path / "data"), str(tmp_path / "calibration")
    os.mkdir(d)
    os.mkdir(cal)
    synth.write_dataset(d, data)
    synth.write_param_file(os.path.join(d, "hypo.in"))
    names = ["S%03d" % (j + 1) for j in range(16)]
    vs, qs, tc, ac = mc.write_calibration(cal, names, n_ranks=2, n_rec=6, vs=3.0, qs=250.0)
    common = [os.path.join(d, "hypo.in"), "--cell"] + [str(v) for v in cases.E2E_CELL] + ["--bounds"] + [str(v) for v in cases.E2E_BOUNDS] + ["--structure", cal]
    lc.main(common + ["--draws", "6", "--volume-of", "3"])
    out = capsys.readouterr().out.split("\n")

    # the restatement: the six records the even thinning keeps, the oracle's volume under each, the mixture, step 5's prior
    ref = cases.e2e_reference()
    grid = ref["grid"]
    keep = [1, 3, 5, 7, 9, 11]
    sta, obs = cases.arrays(data)
    ell = mc.mixture(np.stack([lr.ell_volume(sta, obs, True, True, tc[k], vs[k], ac[k], qs[k], grid) for k in keep]))
    mu_x, mu_y = ObsData.from_arrays(data.sta_x, data.sta_y, *obs).make_initial_guess()
    p = synth.DEFAULT_PARAMS
    quant = [lr.quantiles(lr.summarise(ell[e] + lr.log_prior(grid, [mu_x[e], mu_y[e], p["prior_width_xy"], p["prior_z"], p["prior_width_z"]])[0], grid)["marg"], grid)
             for e in range(8)]
    marginal_stat = open(os.path.join(d, "hypo_grid_marginal.stat")).read()
    stat_lines_agree(marginal_stat.split("\n"), lr.stat_text(data.win_id, np.array(quant)).split("\n"))
    best = open(os.path.join(d, "hypo_grid_marginal.best.dat")).read().split("\n")
    assert best[0] == lc.BEST_HEADER and len(best) == 10 and [int(ln.split()[0]) for ln in best[1:9]] == list(data.win_id)
    n = lr.counts(grid)
    vol = open(os.path.join(d, "hypo_grid_marginal.3.vol.dat")).read().split("\n")
    assert len(vol) == n[0] * n[1] * n[2] + 2 and vol[1].split()[0] == "0"
    assert out[0] == f"8 windows located on {n[0]} x {n[1]} x {n[2]} cells, the structure marginalised over 6 draws" and len(out) == 3
    assert not os.path.exists(os.path.join(d, "hypo_grid.stat"))

    # without --draws, in the same directory: the medians' files as before, and the marginal files stay
    lc.main(common)
    stat_lines_agree(open(os.path.join(d, "hypo_grid.stat")).read().split("\n"), lr.stat_text(data.win_id, ref["quant"]).split("\n"))
    out = capsys.readouterr().out.split("\n")
    assert out[0] == f"8 windows located on {n[0]} x {n[1]} x {n[2]} cells" and os.path.exists(os.path.join(d, "hypo_grid.best.dat"))
    assert open(os.path.join(d, "hypo_grid_marginal.stat")).read() == marginal_stat
    assert open(os.path.join(d, "hypo_grid.stat")).read() != marginal_stat
