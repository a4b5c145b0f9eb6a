"""GPU: htm_forward_locate_draw_evidence (k_locate_draw_evidence, k_locate_draw_combine in hypotremormcmc_amd/csrc/htm_locate.hpp,
DESIGN.md 3.12) against numpy's log-sum-exp over the oracle's volume of every draw (tests/locate_draws_restatement.py over
tests/locate_marginal_cases.py), at the smallest shapes at which the kernels can go wrong: draw counts on both sides of every
block of draws, one draw that dominates (wide) and several that share the weight (tight), ragged tiles, excluded cells.

log_z is pinned per (window, draw): the same -inf pattern, and |log_z_gpu - log_z_ref| <= 2e-12 A elsewhere, A the largest finite
sum of the absolute values of a cell's terms (a cell's value is good to 1e-12 A by the contract of htm_forward_locate, a
log-sum-exp does not amplify a uniform error, the other 1e-12 A is for the sums).  The summary is pinned to the restatement
applied to the device's OWN log_z to 1e-12 relative (the weights are exponentials of differences below 745 in size, 750 epsilon
each), k_max exactly; n_eff also to the full reference, to 8e-12 A relative (a ratio of sums of weights whose logs are good to
2e-12 A).  The worst |log_z_gpu - log_z_ref| / A over every case of this file was 1.1e-15 (it is printed per case)."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from tests import locate_cases as cases
from tests import locate_draws_restatement as dr
from tests import locate_marginal_cases as mc
from tests import locate_restatement as lr
from tests.test_gpu_locate import forward_of

pytestmark = pytest.mark.gpu

RTOL_Z = 2e-12          # of A
IDS = lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def with_forward(c, call):
    fwd = forward_of(c["sta"], c["obs"], c["use"])
    try:
        return call(fwd)
    finally:
        fwd.close()


def run(c, prior, draws=None):
    tc, vs, ac, qs = c["draws"] if draws is None else draws
    return with_forward(c, lambda fwd: lc.draw_evidence(fwd, tc, vs, ac, qs, c["grid"], prior=prior))


def same_bits(a, b, events=slice(None)):
    for key in ("log_z", "n_eff", "w_max", "k_max", "log_evidence"):
        assert np.array_equal(a[key][events], b[key][events], equal_nan=True), key


def check_log_z(got, ref, A, what):
    """got [E][K] against ref [K][E]: the same -inf pattern, no NaN, the others within RTOL_Z A"""
    ref = ref.T
    assert got.shape == ref.shape and not np.isnan(got).any(), what
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)), what
    fin = np.isfinite(ref)
    ratio = np.abs(got[fin] - ref[fin]) / A
    print(f"{what}: {fin.sum()} evidences, worst |log_z_gpu - log_z_ref| / A = {ratio.max() if ratio.size else 0.0:.3e}")
    assert np.all(ratio <= RTOL_Z), (what, ratio.max())


def check_summary(res, ref_log_z=None, A=None):
    """the summary against the restatement applied to the device's own log_z; n_eff also against the full reference"""
    s = dr.summarise(res["log_z"])
    assert np.array_equal(res["k_max"], s["k_max"])
    none = s["k_max"] < 0
    for key in ("n_eff", "w_max", "log_evidence"):
        assert np.isnan(res[key][none]).all() and not np.isnan(res[key][~none]).any(), key
        assert np.all(np.abs(res[key][~none] - s[key][~none]) <= 1e-12 * np.abs(s[key][~none])), (key, res[key], s[key])
    if ref_log_z is not None:
        r = dr.summarise(ref_log_z.T)
        assert np.array_equal(np.isnan(res["n_eff"]), np.isnan(r["n_eff"]))
        assert np.all(np.abs(res["n_eff"][~none] - r["n_eff"][~none]) <= 8e-12 * A * r["n_eff"][~none]), (res["n_eff"], r["n_eff"])


# ---- parity with the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["wide", "tight"])
@pytest.mark.parametrize("key,K", dr.PARITY, ids=IDS)
def test_log_z_and_summary_match_the_reference(key, K, which):
    c = mc.marginal_case(key, K, which)
    for prior in (None, c["prior"]):
        ref, A = dr.log_z_ref(c, prior is not None), dr.bound_scale(c, prior is not None)
        res = run(c, prior)
        check_log_z(res["log_z"], ref, A, f"{key}, K = {K}, {which}, {'flat' if prior is None else 'prior'}")
        check_summary(res, ref, A)


# ---- against the existing device code ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["wide", "tight"])
def test_a_column_is_htm_forward_locate_under_that_draw(which):
    c = mc.marginal_case((3, 1, "5x3x2", "both"), 7, which)
    tc, vs, ac, qs = c["draws"]
    A = dr.bound_scale(c)
    got = run(c, c["prior"])["log_z"]
    per = with_forward(c, lambda fwd: np.stack([lc.locate(fwd, tc[k], vs[k], ac[k], qs[k], c["grid"], prior=c["prior"])["log_evidence"] for k in range(7)], axis=1))
    print(f"columns against htm_forward_locate, {which}: |difference| / A = {np.max(np.abs(got - per)) / A:.3e}")
    assert np.all(np.abs(got - per) <= RTOL_Z * A)


@pytest.mark.parametrize("key,K", [((3, 1, "5x3x2", "both"), 7), ((65, 2, "67x3x5", "both"), 9)], ids=IDS)
@pytest.mark.parametrize("which", ["wide", "tight"])
def test_log_evidence_is_htm_forward_locate_marginal(key, K, which):
    c = mc.marginal_case(key, K, which)
    tc, vs, ac, qs = c["draws"]
    A = dr.bound_scale(c)
    got = run(c, c["prior"])["log_evidence"]
    want = with_forward(c, lambda fwd: lc.locate_marginal(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], marginals=False))["log_evidence"]
    print(f"{key}, K = {K}, {which}: |log_evidence - htm_forward_locate_marginal's| / A = {np.max(np.abs(got - want)) / A:.3e}")
    assert np.all(np.abs(got - want) <= RTOL_Z * A)


# ---- equal draws ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 9])
@pytest.mark.parametrize("key", [(3, 1, "5x3x2", "both"), (65, 2, "67x3x5", "both")], ids=IDS)
def test_equal_draws_count_as_K(key, K):
    """K copies of one structure: equal columns bit for bit, n_eff = K and w_max = 1 / K exactly, the first draw the heaviest; a
    padding draw that was counted would give n_eff = 8 or 16"""
    c = cases.parity_case(*key)
    tc, vs, ac, qs = c["structure"]
    res = run(c, c["prior"], draws=(np.tile(tc, (K, 1)), np.full(K, vs), np.tile(ac, (K, 1)), np.full(K, qs)))
    assert np.isfinite(res["log_z"]).all()
    for k in range(1, K):
        assert np.array_equal(res["log_z"][:, k], res["log_z"][:, 0]), k
    assert np.all(res["n_eff"] == K) and np.all(res["w_max"] == 1.0 / K) and np.all(res["k_max"] == 0)
    assert np.array_equal(res["log_evidence"], res["log_z"][:, 0])      # (S1 = K exactly: log S1 - log K is exactly 0)


# ---- excluded cells ------------------------------------------------------------------------------------------------------------
def test_excluded_cells_and_a_window_without_a_cell():
    """a cell centre on a station is NaN under every draw, a layer at z0 and below is -inf: left out per draw; event 2 has no
    cell left under any draw and leaves its neighbours untouched"""
    c = mc.marginal_case("excluded", 3, "tight")
    ref, A = dr.log_z_ref(c), dr.bound_scale(c)
    res = run(c, c["prior"])
    check_log_z(res["log_z"], ref, A, "excluded, K = 3")
    check_summary(res, ref, A)
    assert np.isfinite(res["log_z"][:2]).all() and np.isneginf(res["log_z"][2]).all()
    assert np.isnan([res["n_eff"][2], res["w_max"][2], res["log_evidence"][2]]).all() and res["k_max"][2] == -1
    prior = c["prior"].copy()
    prior[2, 3] = -1.0                                                   # event 2 gets its cells back: events 0 and 1 keep their bits
    other = run(c, prior)
    assert other["k_max"][2] >= 0 and np.isfinite(other["log_z"][2]).all()
    same_bits(res, other, slice(0, 2))
    flat = run(c, None)
    check_log_z(flat["log_z"], dr.log_z_ref(c, False), dr.bound_scale(c, False), "excluded, K = 3, flat")
    assert (flat["k_max"] >= 0).all()


# ---- determinism and batching --------------------------------------------------------------------------------------------------
def test_two_calls_and_every_batching_give_the_same_bits(monkeypatch):
    c = dict(cases.parity_case(65, 5, "67x3x5", "both"))
    c["draws"] = mc.draws(65, 7 * 65 + 5, "tight", 9)
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    first = run(c, c["prior"])
    again = run(c, c["prior"])
    # 5 tiles (a layer each), the 9 draws padded to 16: an event's workspace is 8 (5 * 16 * 2 + 9 + 4) bytes, its prior tables
    # 8 * 75 and its station records 65 * 80 + 32, 7216 bytes in all; the draws' table and its input are 26400 bytes (blocks of 8
    # draws).  36700 bytes hold the table and one event (33616), not two (40832) -- five batches of one event
    monkeypatch.setenv("HTM_LOCATE_MB", "0.035")
    single = run(c, c["prior"])
    monkeypatch.setenv("HTM_LOCATE_MB", "0.042")         # 44040 bytes: the table and two events, not three (48048): batches of 2, 2, 1
    pairs = run(c, c["prior"])
    for other in (again, single, pairs):
        same_bits(first, other)
    monkeypatch.setenv("HTM_LOCATE_MB", "0.03")          # 31457 bytes: the table fits, an event with it does not
    with pytest.raises(lc._lib.HtmError, match="HTM_LOCATE_MB"):
        run(c, c["prior"])
    monkeypatch.setenv("HTM_LOCATE_MB", "0.01")          # less than the table
    with pytest.raises(lc._lib.HtmError, match="HTM_LOCATE_MB = 0.01: the table of 9 draws"):
        run(c, None)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_with_a_real_handle():
    c = cases.parity_case(3, 5, "5x3x2", "both")
    fwd = forward_of(c["sta"], c["obs"])
    lib, p = lc._lib.load(), lc._lib.ptr
    last = lambda: lib.htm_last_error().decode()
    out, summ, good = np.zeros(5 * 4097), np.zeros(5 * 4), np.array([0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2])
    corr = np.zeros(4097 * 3)

    def call(K=3, tc=corr, vs=(3.0, 3.1, 3.2), ac=corr, qs=(250.0, 240.0, 260.0), grid=good, log_z=out, summary=summ):
        f = lambda v: None if v is None else np.array(v, dtype=np.float64)
        return lib.htm_forward_locate_draw_evidence(fwd.handle, K, p(tc), p(f(vs)), p(ac), p(f(qs)), p(f(grid)), None, p(log_z), p(summary))

    try:
        assert call() == 0 and summ[2] >= 0.0
        assert call(summary=None) == 0                                   # the summary may be left out
        for kw in ({"tc": None}, {"vs": None}, {"ac": None}, {"qs": None}, {"grid": None}, {"log_z": None}):
            assert call(**kw) == -1 and last() == "NULL argument", kw
        big = np.full(4097, 3.0)
        for K in (0, -1, 4097):
            assert call(K=K, vs=big, qs=big) == -1 and last() == f"n_draws = {K}: need 1..4096", K
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(vs=(3.0, bad, 3.2)) == -1 and last().startswith("draw 1: vs = ") and "need finite values > 0" in last(), bad
        for bad in (0.0, -5.0, float("nan"), float("inf")):
            assert call(qs=(250.0, 240.0, bad)) == -1 and last().startswith("draw 2: vs = 3.2, qs = ") and "need finite values > 0" in last(), bad
        assert call(grid=[0.0, 0.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2]) == -1 and "cell size" in last()
        assert call(grid=[0.0, 1.0, 4.5, 0.0, 1.0, 3, 0.0, 1.0, 2]) == -1 and "grid axis x: 4.5 cells" in last()
        assert call(grid=[0.0, 1.0, 4096, 0.0, 1.0, 4096, 0.0, 1.0, 128]) == -1 and "more than 2^31 - 1" in last()
    finally:
        fwd.close()
    with pytest.raises(lc._lib.HtmError, match="event 3: prior widths"):
        prior = c["prior"].copy()
        prior[3, 2] = 0.0
        run(dict(c, draws=(np.zeros((2, 3)), [3.0, 3.1], np.zeros((2, 3)), [250.0, 240.0])), prior)
    with pytest.raises(ValueError, match="2 draws of vs"):
        run(dict(c, draws=(np.zeros((2, 3)), [3.0, 3.1], np.zeros((3, 3)), [250.0, 240.0])), None)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(tmp_path, capsys):
    from hypotremormcmc_amd.forward import Forward
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.run_files import Step5Run

    data = cases.e2e_data()
    names = ["S%03d" % (j + 1) for j in range(16)]

    def job(where):
        d, cal = str(tmp_path / where / "data"), str(tmp_path / where / "calibration")
        os.makedirs(d)
        os.makedirs(cal)
        synth.write_dataset(d, data)
        synth.write_param_file(os.path.join(d, "hypo.in"))
        smp = mc.write_calibration(cal, names, n_ranks=2, n_rec=6, vs=3.0, qs=250.0)
        common = [os.path.join(d, "hypo.in"), "--cell"] + [str(v) for v in cases.E2E_CELL] + ["--bounds"] + [str(v) for v in cases.E2E_BOUNDS] + ["--structure", cal]
        return d, cal, smp, common + ["--draws", "6"]

    d, cal, (vs, qs, tc, ac), argv = job("with")
    lc.main(argv + ["--draw-weights"])
    out = capsys.readouterr().out.split("\n")
    grid = cases.e2e_reference()["grid"]
    n = lr.counts(grid)
    assert out[0] == f"8 windows located on {n[0]} x {n[1]} x {n[2]} cells, the structure marginalised over 6 draws"
    assert len(out) == 4 and out[2].startswith("the 6 draws' effective number per window: median ") and out[3] == ""

    # draw_evidence called directly on the files the program read: the six records the even thinning keeps, step 5's prior
    keep = lc.draw_records(12, 6)
    assert keep == [1, 3, 5, 7, 9, 11]
    par = Step5Run.open(os.path.join(d, "hypo.in")).par
    obs = ObsData(list(data.win_id), par.n_stations, par.sta_x, par.sta_y, directory=d)
    fwd = Forward(par.n_stations, 8, par.sta_x, par.sta_y, par.sta_z, obs, use_amp=par.get_use_amp(), use_time=par.get_use_time())
    try:
        ev = lc.draw_evidence(fwd, tc[keep], vs[keep], ac[keep], qs[keep], grid, prior=lc.step5_prior(par, obs))
    finally:
        fwd.close()
    assert (ev["k_max"] >= 0).all() and lc.read_structure_draws(cal, par.stations, par.n_stations, 6, records=True)[4] == keep

    rows = [ln.split() for ln in open(os.path.join(d, "hypo_grid_marginal.draws.dat")).read().split("\n")[1:] if ln]
    assert open(os.path.join(d, "hypo_grid_marginal.draws.dat")).readline().rstrip("\n") == lc.DRAWS_HEADER
    assert len(rows) == 8 and all(len(r) == 7 for r in rows) and [int(r[0]) for r in rows] == list(data.win_id)
    col = lambda j: np.array([float(r[j]) for r in rows])
    assert np.all(np.abs(col(1) - ev["n_eff"]) <= 1e-6) and np.all(np.abs(col(2) - ev["n_eff"] / 6) <= 1e-6) and np.all(np.abs(col(3) - ev["w_max"]) <= 1e-9)
    assert [int(r[4]) for r in rows] == [keep[k] for k in ev["k_max"]] and np.all(np.abs(col(5) - ev["log_evidence"]) <= 1e-6)
    assert [int(r[6]) for r in rows] == [int(w > 0.5) for w in ev["w_max"]]
    assert open(os.path.join(d, "hypo_grid_marginal.draws.dat")).read() == lc.draws_text(data.win_id, ev, keep)

    rows = [ln.split() for ln in open(os.path.join(d, "hypo_grid_marginal.structure.dat")).read().split("\n")[1:] if ln]
    assert len(rows) == 6 and all(len(r) == 5 for r in rows) and [int(r[0]) for r in rows] == keep
    assert np.all(np.abs(col(1) - vs[keep]) <= 1e-6) and np.all(np.abs(col(2) - qs[keep]) <= 1e-6)
    assert max(col(3)) == 0.0 and abs(col(4).sum() - 1.0) <= 6e-9
    assert open(os.path.join(d, "hypo_grid_marginal.structure.dat")).read() == lc.structure_text(keep, vs[keep], qs[keep], ev["log_z"])
    assert os.path.exists(os.path.join(d, "hypo_grid_marginal.stat")) and os.path.exists(os.path.join(d, "hypo_grid_marginal.best.dat"))

    # without --draw-weights, in a fresh directory: neither file, three lines
    d2, _, _, argv = job("without")
    lc.main(argv)
    out2 = capsys.readouterr().out.split("\n")
    assert len(out2) == 3 and out2[:2] == out[:2]
    assert sorted(os.listdir(d2)) == sorted(f for f in os.listdir(d) if f not in ("hypo_grid_marginal.draws.dat", "hypo_grid_marginal.structure.dat"))
    for f in ("hypo_grid_marginal.stat", "hypo_grid_marginal.best.dat"):
        assert open(os.path.join(d2, f)).read() == open(os.path.join(d, f)).read(), f
