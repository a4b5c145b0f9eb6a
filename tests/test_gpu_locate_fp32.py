"""GPU: the single-precision forward of htm_forward_locate, htm_forward_locate_marginal and htm_forward_locate_draw_evidence
(htm_forward_locate_set_precision; loc_station<.., F32> in hypotremormcmc_amd/csrc/htm_locate.hpp) against its
definition in numpy.longdouble (tests/locate_fp32_restatement.py), at the shapes of tests/test_gpu_locate.py.

The volume is pinned cell by cell: the reference's NaN / -inf pattern, and |lp - lp_reference| <= U 2^-24 D32 + 1e-12 A elsewhere
(U, D32: the restatement; A: tests/test_gpu_locate.py's sum of absolute terms).  Everything behind a cell's term is fp64 in this
mode too, so the summaries are held to the restatement applied to the device's OWN fp32 volume at tests/test_gpu_locate.py's
tolerances, and the relations between the three entry points hold at the tolerances of their own tests, bitwise where those
are bitwise."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from tests import locate_cases as cases
from tests import locate_draws_restatement as dr
from tests import locate_fp32_restatement as l32
from tests import locate_marginal_cases as mc
from tests import locate_restatement as lr
from tests.test_gpu_locate import check_summaries, forward_of
from tests.test_gpu_locate_draws import RTOL_Z

pytestmark = pytest.mark.gpu

KEYS = ("loc", "marg_x", "marg_y", "marg_z", "vol")
EV_KEYS = ("log_z", "n_eff", "w_max", "k_max", "log_evidence")
KS = (1, 7, 9, 33)              # one block of draws, ragged blocks, several blocks


def with_forward(c, call, precision="fp32"):
    fwd = forward_of(c["sta"], c["obs"], c["use"])
    try:
        if precision is not None:
            fwd.set_locate_precision(precision)
        return call(fwd)
    finally:
        fwd.close()


def run(c, prior, structure=None, precision="fp32", **kw):
    tc, vs, ac, qs = c["structure"] if structure is None else structure
    return with_forward(c, lambda fwd: lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=prior, volume=True, **kw), precision)


def run_marginal(c, prior, draws, precision="fp32", **kw):
    tc, vs, ac, qs = draws
    return with_forward(c, lambda fwd: lc.locate_marginal(fwd, tc, vs, ac, qs, c["grid"], prior=prior, volume=True, **kw), precision)


def run_evidence(c, prior, draws, precision="fp32"):
    tc, vs, ac, qs = draws
    return with_forward(c, lambda fwd: lc.draw_evidence(fwd, tc, vs, ac, qs, c["grid"], prior=prior), precision)


def differ(a, b):
    """whether two arrays differ in a value's bits somewhere (NaN against NaN does not count)"""
    return bool(((a != b) & ~(np.isnan(a) & np.isnan(b))).any())


def same_bits(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


# ---- 1, 2: the volume to the bound; the summaries are fp64 --------------------------------------------------------------------
@pytest.mark.parametrize("key", l32.volume_cases(), ids=l32.case_id)
def test_volume_is_within_the_bound_and_the_summaries_are_fp64(key):
    c, ref = l32.case(key), l32.references(key)
    what = l32.case_id(key)
    # (flat: the keyword, on a handle that was never switched; with the prior: the handle's own setting)
    flat = with_forward(c, lambda fwd: lc.locate(fwd, *c["structure"], c["grid"], volume=True, precision="fp32"), None)
    l32.check_volume(flat["vol"], ref.ell, ref.D32, c["abs"], what + ", flat")
    assert np.array_equal(flat["ell"], flat["lp"])                        # a flat prior: lp is the term itself
    pri = run(c, c["prior"])
    l32.check_volume(pri["vol"], ref.lp_prior, ref.D32, c["abs_prior"], what + ", prior")
    # the device's own fp32 volume through the restatement's summaries: best cell and lp exact, the sums to their fp64 tolerances
    check_summaries(flat, c["grid"])
    check_summaries(pri, c["grid"])
    for res in (flat, pri):
        for e, vol in enumerate(res["vol"]):
            if res["index"][e] >= 0:
                assert res["lp"][e] == vol.reshape(-1)[res["index"][e]] and res["lp"][e] == np.max(vol[lr.included(vol)])


# ---- 3: the mode ran, and it comes off ------------------------------------------------------------------------------------------
def test_the_mode_ran_and_it_comes_off():
    c = cases.parity_case(5, 1, "70x60x2", "both")
    tc, vs, ac, qs = c["structure"]
    d = mc.draws(5, 7 * 5 + 1, "tight", 9)
    fwd = forward_of(c["sta"], c["obs"], c["use"])
    try:
        every = lambda: (lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True),
                         lc.locate_marginal(fwd, *d, c["grid"], prior=c["prior"], volume=True), lc.draw_evidence(fwd, *d, c["grid"], prior=c["prior"]))
        before = every()
        assert fwd.locate_precision == "fp64"
        fwd.set_locate_precision("fp32")
        assert fwd.locate_precision == "fp32"
        single = every()
        for a, b in zip(before[:2], single[:2]):
            assert differ(a["vol"], b["vol"])
        assert differ(before[2]["log_z"], single[2]["log_z"])
        # the keyword sets the precision for a call and puts the previous setting back
        same_bits(lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True, precision="fp64"), before[0])
        assert fwd.locate_precision == "fp32"
        same_bits(lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True), single[0])
        fwd.set_locate_precision("fp64")
        after = every()
        same_bits(after[0], before[0])
        same_bits(after[1], before[1])
        same_bits(after[2], before[2], EV_KEYS)
        # step 5's switch alone leaves locate's fp64 bits
        fwd.set_precision("fp32")
        step5 = every()
        same_bits(step5[0], before[0])
        same_bits(step5[1], before[1])
        same_bits(step5[2], before[2], EV_KEYS)
        with pytest.raises(ValueError, match="locate precision"):
            fwd.set_locate_precision("fp16")
    finally:
        fwd.close()


# ---- 4: excluded cells -----------------------------------------------------------------------------------------------------------
def test_excluded_cells_keep_their_meaning():
    """a cell centre on a station (NaN), a lowest layer at z0 and below it (-inf), an event with no cell left (-1 and NaN): as in
    fp64, cell for cell; the neighbours of the event without a cell are untouched"""
    c = cases.excluded_case()
    ell, D32, _ = l32.reference(c["sta"], c["obs"], c["use"], c["structure"], c["grid"])
    with np.errstate(invalid="ignore"):
        lp = ell + np.stack([lr.log_prior(c["grid"], p)[0] for p in c["prior"]]).astype(l32.LD)
    res, res64 = run(c, c["prior"]), run(c, c["prior"], precision="fp64")
    assert np.array_equal(np.isnan(res["vol"]), np.isnan(res64["vol"])) and np.array_equal(np.isneginf(res["vol"]), np.isneginf(res64["vol"]))
    l32.check_volume(res["vol"], lp, D32, c["abs_prior"], "excluded")
    check_summaries(res, c["grid"])
    assert list(res["index"] >= 0) == [True, True, False] and list(res64["index"] >= 0) == [True, True, False]
    assert np.isnan(res["vol"][0, 0, 1, 1]) and np.isneginf(res["vol"][0, 0]).sum() == 14
    assert np.isnan(res["loc"][2, 1:]).all() and np.isnan(res["marg_x"][2]).all() and not lr.included(res["vol"][2]).any()
    prior = c["prior"].copy()
    prior[2, 3] = -1.0                                                   # event 2 gets its cells back: events 0 and 1 keep their bits
    other = run(c, prior)
    assert other["index"][2] >= 0
    for key in KEYS:
        assert np.array_equal(res[key][:2], other[key][:2], equal_nan=True), key
    flat = run(c, None)
    l32.check_volume(flat["vol"], ell, D32, c["abs"], "excluded, flat")
    assert np.isnan(flat["vol"][:, 0, 1, 1]).all() and (flat["index"] >= 0).all()
    # under draws: NaN under every draw, -inf kept, the window without a cell
    d = mc.draws(6, 41, "tight", 3)
    m = run_marginal(c, c["prior"], d)
    assert np.array_equal(np.isnan(m["vol"]), np.isnan(res["vol"])) and np.array_equal(np.isneginf(m["vol"]), np.isneginf(res["vol"]))
    assert list(m["index"] >= 0) == [True, True, False]
    ev = run_evidence(c, c["prior"], d)
    assert np.isfinite(ev["log_z"][:2]).all() and np.isneginf(ev["log_z"][2]).all() and ev["k_max"][2] == -1 and np.isnan(ev["n_eff"][2])


# ---- 5: the three entry points agree in fp32 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(3, 1, "5x3x2", "both"), (5, 1, "70x60x2", "both")])
def test_one_draw_is_htm_forward_locate(key):
    c = cases.parity_case(*key)
    tc, vs, ac, qs = c["structure"]
    for prior in (None, c["prior"]):
        one = run(c, prior)
        same_bits(run_marginal(c, prior, (tc[None], [vs], ac[None], [qs])), one)
        ev = run_evidence(c, prior, (tc[None], [vs], ac[None], [qs]))
        A = np.max(c["abs_prior"][np.isfinite(c["abs_prior"])])
        assert np.all(np.abs(ev["log_z"][:, 0] - one["log_evidence"]) <= RTOL_Z * A)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("key", [(3, 1, "5x3x2", "both"), (65, 2, "67x3x5", "both")])
def test_equal_draws_are_one_draw(key, K):
    c = cases.parity_case(*key)
    tc, vs, ac, qs = c["structure"]
    one = run(c, c["prior"])
    same_bits(run_marginal(c, c["prior"], (np.tile(tc, (K, 1)), np.full(K, vs), np.tile(ac, (K, 1)), np.full(K, qs))), one)


@pytest.mark.parametrize("which", ["wide", "tight"])
@pytest.mark.parametrize("K", KS)
def test_evidence_identity_columns_and_mixture(K, which):
    """at their own tests' tolerances: the mixture's log evidence is the log-mean-exp of htm_forward_locate's under every draw
    (2e-12 A); a column of log_z is htm_forward_locate's log evidence under that draw (2e-12 A); draw_evidence's log evidence is
    htm_forward_locate_marginal's (2e-12 A).  The fp32 terms of a (cell, draw) are the same bits in all three kernels: what is
    left is their fp64 sums."""
    c = mc.marginal_case((3, 1, "5x3x2", "both"), K, which)
    tc, vs, ac, qs = c["draws"]
    A = dr.bound_scale(c)
    marg = run_marginal(c, c["prior"], c["draws"])
    ev = run_evidence(c, c["prior"], c["draws"])
    per = with_forward(c, lambda fwd: np.stack([lc.locate(fwd, tc[k], vs[k], ac[k], qs[k], c["grid"], prior=c["prior"])["log_evidence"] for k in range(K)]))
    print(f"K = {K}, {which}, in A: identity {np.max(np.abs(marg['log_evidence'] - mc.mixture(per))) / A:.3e}, columns "
          f"{np.max(np.abs(ev['log_z'] - per.T)) / A:.3e}, mixture {np.max(np.abs(ev['log_evidence'] - marg['log_evidence'])) / A:.3e}")
    assert np.all(np.abs(marg["log_evidence"] - mc.mixture(per)) <= 2e-12 * A)
    assert np.all(np.abs(ev["log_z"] - per.T) <= RTOL_Z * A)
    assert np.all(np.abs(ev["log_evidence"] - marg["log_evidence"]) <= RTOL_Z * A)
    # the marginal volume against the fp64 one: the mode ran here too (K = 1: test_the_mode_ran_and_it_comes_off)
    assert differ(marg["vol"], run_marginal(c, c["prior"], c["draws"], precision="fp64")["vol"])


def test_marginal_volume_is_within_the_largest_draw_s_bound():
    """K = 7: |lp - log-mean-exp of the per-draw reference terms| <= max_k U 2^-24 D32_k + 1e-12 A: a log-sum-exp moves by no more
    than its largest argument does"""
    for key, which in (((3, 1, "5x3x2", "both"), "wide"), ((3, 1, "5x3x2", "both"), "tight"), ((65, 2, "67x3x5", "both"), "tight")):
        c = mc.marginal_case(key, 7, which)
        ell, D32 = l32.marginal_reference(c)
        flat = run_marginal(c, None, c["draws"])
        l32.check_volume(flat["vol"], ell, D32, c["abs"], f"{key}, K = 7, {which}, flat")
        pri = run_marginal(c, c["prior"], c["draws"])
        with np.errstate(invalid="ignore"):
            l32.check_volume(pri["vol"], ell + c["log_prior"].astype(l32.LD), D32, c["abs_prior"], f"{key}, K = 7, {which}, prior")
        check_summaries(pri, c["grid"])


# ---- 6: determinism ------------------------------------------------------------------------------------------------------------
def test_two_calls_and_one_event_per_batch_give_the_same_bits(monkeypatch):
    c = cases.parity_case(65, 5, "67x3x5", "both")
    d = mc.draws(65, 7 * 65 + 5, "tight", 9)
    # an event's workspace is 17680 bytes with the volume and 7216 for the evidences; the fp32 table of 9 draws (padded to 16)
    # and its input are 8 * 66 * 16 + 8 * 132 * 9 = 17952 bytes.  One event fits, not two: 20972 of 17680 / 35360; 41943 of 35632 /
    # 53312; 28311 of 25168 / 32384
    for call, keys, mb in ((lambda: run(c, c["prior"]), KEYS, "0.02"), (lambda: run_marginal(c, c["prior"], d), KEYS, "0.04"),
                           (lambda: run_evidence(c, c["prior"], d), EV_KEYS, "0.027")):
        monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
        first, again = call(), call()
        monkeypatch.setenv("HTM_LOCATE_MB", mb)
        single = call()
        same_bits(first, again, keys)
        same_bits(first, single, keys)


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_real_handle():
    c = cases.parity_case(3, 5, "5x3x2", "both")
    tc, vs, ac, qs = c["structure"]
    lib = lc._lib.load()
    last = lambda: lib.htm_last_error().decode()
    fwd = forward_of(c["sta"], c["obs"])
    try:
        before = lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True)
        assert lib.htm_forward_locate_set_precision(None, 1) == -1 and last() == "NULL handle"
        for bad in (2, -1):
            assert lib.htm_forward_locate_set_precision(fwd.handle, bad) == -1 and last() == f"forward_fp32 = {bad}: need 0 (fp64) or 1 (fp32)"
        same_bits(lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True), before)
        assert lib.htm_forward_locate_set_precision(fwd.handle, 1) == 0
        single = lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True)
        assert differ(single["vol"], before["vol"])
        assert lib.htm_forward_locate_set_precision(fwd.handle, 2) == -1                    # refused: the setting stays
        same_bits(lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True), single)
        assert lib.htm_forward_locate_set_precision(fwd.handle, 0) == 0
        same_bits(lc.locate(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True), before)
    finally:
        fwd.close()


# ---- 8: the program end to end ---------------------------------------------------------------------------------------------------
def test_program_end_to_end(tmp_path, capsys):
    from hypotremormcmc_amd.forward import Forward
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.run_files import Step5Run

    data = cases.e2e_data()
    names = ["S%03d" % (j + 1) for j in range(16)]
    grid = cases.e2e_reference()["grid"]
    n = lr.counts(grid)
    read = lambda d, f: open(os.path.join(d, f)).read()

    def job(where):
        d, cal = str(tmp_path / where / "data"), str(tmp_path / where / "calibration")
        os.makedirs(d)
        os.makedirs(cal)
        synth.write_dataset(d, data)
        synth.write_param_file(os.path.join(d, "hypo.in"))
        smp = mc.write_calibration(cal, names, n_ranks=2, n_rec=6, vs=3.0, qs=250.0)
        return d, smp, [os.path.join(d, "hypo.in"), "--cell"] + [str(v) for v in cases.E2E_CELL] + ["--bounds"] + [str(v) for v in cases.E2E_BOUNDS] + ["--structure", cal]

    def api(d, precision, draws):
        """the program's files from the Python API's results: (stat, best, volume of window 3[, draws, structure])"""
        par = Step5Run.open(os.path.join(d, "hypo.in")).par
        obs = ObsData(list(data.win_id), par.n_stations, par.sta_x, par.sta_y, directory=d)
        fwd = Forward(par.n_stations, 8, par.sta_x, par.sta_y, par.sta_z, obs, use_amp=par.get_use_amp(), use_time=par.get_use_time())
        try:
            prior = lc.step5_prior(par, obs)
            if draws is None:
                res = lc.locate(fwd, np.zeros(16), 3.0, np.zeros(16), 250.0, grid, prior=prior, volume=True, precision=precision)
                ev = None
            else:
                res = lc.locate_marginal(fwd, *draws, grid, prior=prior, volume=True, precision=precision)
                ev = lc.draw_evidence(fwd, *draws, grid, prior=prior, precision=precision)
            assert fwd.locate_precision == "fp64"
        finally:
            fwd.close()
        marg = np.concatenate([res["marg_x"], res["marg_y"], res["marg_z"]], axis=1)
        return res, ev, (lc.stat_text(data.win_id, lc.marginal_quantiles(marg, grid)), lc.best_text(data.win_id, res, grid),
                         lc.volume_text(res["vol"][list(data.win_id).index(3)], grid))

    # a fixed structure
    d, _, argv = job("fixed32")
    lc.main(argv + ["--volume-of", "3", "--precision", "fp32"])
    out = capsys.readouterr().out.split("\n")
    _, _, want = api(d, "fp32", None)
    assert (read(d, "hypo_grid.stat"), read(d, "hypo_grid.best.dat"), read(d, "hypo_grid.3.vol.dat")) == want
    assert out[0] == f"8 windows located on {n[0]} x {n[1]} x {n[2]} cells" and out[2].startswith("forward precision: fp32") and len(out) == 4
    d64, _, argv = job("fixed64")
    lc.main(argv + ["--volume-of", "3"])
    out64 = capsys.readouterr().out.split("\n")
    _, _, want64 = api(d64, None, None)
    assert (read(d64, "hypo_grid.stat"), read(d64, "hypo_grid.best.dat"), read(d64, "hypo_grid.3.vol.dat")) == want64
    assert len(out64) == 3 and out64[:2] == out[:2] and sorted(os.listdir(d64)) == sorted(os.listdir(d))
    assert want64[2] != want[2]                                            # the fp32 volume is not the fp64 one
    d64b, _, argv = job("fixed64b")
    lc.main(argv + ["--volume-of", "3", "--precision", "fp64"])
    assert capsys.readouterr().out.split("\n") == out64
    for f in ("hypo_grid.stat", "hypo_grid.best.dat", "hypo_grid.3.vol.dat"):
        assert read(d64b, f) == read(d64, f), f

    # draws and their weights
    keep = lc.draw_records(12, 6)
    d, (vs, qs, tc, ac), argv = job("draws32")
    lc.main(argv + ["--draws", "6", "--draw-weights", "--volume-of", "3", "--precision", "fp32"])
    out = capsys.readouterr().out.split("\n")
    _, ev, want = api(d, "fp32", (tc[keep], vs[keep], ac[keep], qs[keep]))
    assert (read(d, "hypo_grid_marginal.stat"), read(d, "hypo_grid_marginal.best.dat"), read(d, "hypo_grid_marginal.3.vol.dat")) == want
    assert read(d, "hypo_grid_marginal.draws.dat") == lc.draws_text(data.win_id, ev, keep)
    assert read(d, "hypo_grid_marginal.structure.dat") == lc.structure_text(keep, vs[keep], qs[keep], ev["log_z"])
    assert out[0].endswith("the structure marginalised over 6 draws") and out[2].startswith("forward precision: fp32")
    assert out[3].startswith("the 6 draws' effective number per window") and len(out) == 5
    d64, _, argv = job("draws64")
    lc.main(argv + ["--draws", "6", "--draw-weights", "--volume-of", "3"])
    out64 = capsys.readouterr().out.split("\n")
    _, ev64, want64 = api(d64, None, (tc[keep], vs[keep], ac[keep], qs[keep]))
    assert (read(d64, "hypo_grid_marginal.stat"), read(d64, "hypo_grid_marginal.best.dat"), read(d64, "hypo_grid_marginal.3.vol.dat")) == want64
    assert read(d64, "hypo_grid_marginal.draws.dat") == lc.draws_text(data.win_id, ev64, keep)
    assert len(out64) == 4 and not any("precision" in ln for ln in out64) and sorted(os.listdir(d64)) == sorted(os.listdir(d))
    assert want64[2] != want[2]
