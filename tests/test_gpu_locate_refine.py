"""GPU: htm_forward_locate_boxes and the coarse-to-fine refinement over it.

THE RULE is pinned bit for bit: row e of `locate_boxes` against row e of `locate` (or `locate_marginal`) on event e's own grid,
on the same Forward -- loc, the three marginals and the volume with np.array_equal, the NaN patterns compared separately.  The
shapes are those at which tests/test_gpu_locate.py finds the kernels' paths: one cell; a few; a row longer than a wave with five
tiles and 65 stations; two tiles per layer, the second ragged (the combine's mixed moments across tiles).  Every axis -- mode,
precision, prior, draws -- is varied at least once, not in all combinations.  Then the batching (an origin indexed by the wrong
event number would show there), a window without a cell, the refusals, the noise-free recovery of
tests/locate_refine_cases.py (re-checked with numpy in tests/test_locate_refine.py), and the program end to end."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from hypotremormcmc_amd.forward import Forward, ObsArrays
from hypotremormcmc_amd.obs_data import ObsData
from tests import locate_cases as cases
from tests import locate_marginal_cases as mc
from tests import locate_refine_cases as rc
from tests import locate_restatement as lr

pytestmark = pytest.mark.gpu

E = 5
KEYS = ("loc", "marg_x", "marg_y", "marg_z", "vol")


def make(n_sta, grid_name, mode, prior, K):
    """data of E events, the grid, E origins -- the first exactly the grid's --, a structure or K draws of it, a prior or None"""
    seed = 7 * n_sta + E
    data = synth.make_synthetic(E, n_sta, seed)
    sta, obs = cases.arrays(data)
    grid = cases.GRIDS[grid_name]
    rng = np.random.default_rng(4000 + seed)
    origins = rng.uniform(-30, 30, (E, 3))
    origins[0] = grid[0::3]
    structure = cases.structure(n_sta, seed) if K == 0 else mc.draws(n_sta, seed, "tight", K)
    return {"sta": sta, "obs": obs, "use": cases.MODES[mode], "grid": grid, "origins": origins, "structure": structure, "K": K,
            "prior": cases.prior_of(sta, obs, seed) if prior else None}


def forward_of(c):
    n_ev, S = c["obs"][0].shape
    return Forward(S, n_ev, c["sta"][0], c["sta"][1], c["sta"][2], ObsArrays(*c["obs"]), use_time=c["use"][0], use_amp=c["use"][1])


def own_grid(c, e):
    g = c["grid"].copy()
    g[0::3] = c["origins"][e]
    return g


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), what


def check_rule(c, fwd, precision, res=None):
    if res is None:
        res = lc.locate_boxes(fwd, *c["structure"], c["grid"], c["origins"], prior=c["prior"], volume=True, precision=precision)
    assert np.array_equal(res["origin"], c["origins"])
    single = lc.locate if c["K"] == 0 else lc.locate_marginal
    for e in range(E):
        ref = single(fwd, *c["structure"], own_grid(c, e), prior=c["prior"], volume=True, precision=precision)
        for key in KEYS:
            same_bits(res[key][e], ref[key][e], (e, key))
    return res


# (stations, grid, mode, precision, prior, draws)
RULE_CASES = [
    (3, "1x1x1", "both", "fp64", False, 0),
    (3, "1x1x1", "time", "fp32", True, 9),
    (3, "5x3x2", "time", "fp32", True, 0),
    (3, "5x3x2", "both", "fp64", True, 1),
    (3, "5x3x2", "amp", "fp64", False, 9),
    (65, "67x3x5", "both", "fp64", True, 0),
    (65, "67x3x5", "amp", "fp32", False, 0),
    (65, "67x3x5", "both", "fp32", True, 9),
    (5, "70x60x2", "both", "fp64", True, 0),
    (5, "70x60x2", "amp", "fp64", False, 0),
    (5, "70x60x2", "time", "fp32", False, 1),
    (5, "70x60x2", "both", "fp64", True, 9),
]


@pytest.mark.parametrize("n_sta,grid_name,mode,precision,prior,K", RULE_CASES)
def test_every_event_has_the_bits_of_a_call_on_its_own_grid(n_sta, grid_name, mode, precision, prior, K):
    c = make(n_sta, grid_name, mode, prior, K)
    fwd = forward_of(c)
    try:
        res = check_rule(c, fwd, precision)
        assert res["index"][0] >= 0 and (prior or ((res["index"] >= 0).all() and not np.isnan(res["loc"]).any()))
        # the index is the cell within the event's own box, the coordinates are absolute
        nx, ny, _ = lr.counts(c["grid"])
        for e in range(E):
            i = res["index"][e]
            if i < 0:                                          # (the prior's z0 above a box that was drawn low)
                continue
            ijk = (i % nx, (i // nx) % ny, i // (nx * ny))
            want = [c["origins"][e, a] + (ijk[a] + 0.5) * c["grid"][3 * a + 1] for a in range(3)]
            assert list(res["best"][e]) == want, e
        assert fwd.locate_precision == "fp64"
    finally:
        fwd.close()


def test_the_batching_leaves_the_bits(monkeypatch):
    c = make(65, "67x3x5", "both", True, 0)
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    kw = dict(n_sta=65, n_events=E, grid=c["grid"], volume=True, prior=True, boxes=True)
    mb = 2.5 * lc.plan(**kw)["per_event_bytes"] / 1048576.0
    fwd = forward_of(c)
    try:
        whole = check_rule(c, fwd, None)
        monkeypatch.setenv("HTM_LOCATE_MB", repr(mb))
        assert lc.plan(**kw)["nb"] == 2                       # batches of 2, 2 and 1 events
        parts = lc.locate_boxes(fwd, *c["structure"], c["grid"], c["origins"], prior=c["prior"], volume=True)
        for key in KEYS:
            same_bits(parts[key], whole[key], key)
    finally:
        fwd.close()


def test_a_window_without_a_cell_in_its_box():
    """the prior's z0 lies above every centre of event 1's box and inside event 0's"""
    c = make(3, "5x3x2", "both", True, 0)                          # layers' centres: the box's z0 + 3.5 and + 10.5
    c["origins"][1, 2] = -30.0
    c["prior"][:, 3] = 0.0
    assert c["origins"][0, 2] + 3.5 > 0.0 > c["origins"][1, 2] + 10.5
    fwd = forward_of(c)
    try:
        res = check_rule(c, fwd, None)
        assert res["index"][1] == -1 and np.isnan(res["loc"][1, 1:]).all() and np.isneginf(res["vol"][1]).all()
        assert all(np.isnan(res[k][1]).all() for k in ("marg_x", "marg_y", "marg_z"))
        assert res["index"][0] >= 0 and not np.isnan(res["loc"][0]).any()
        # the other rows are what they are when event 1 has a cell
        other = dict(c, origins=c["origins"].copy())
        other["origins"][1, 2] = c["grid"][6]
        ref = lc.locate_boxes(fwd, *other["structure"], other["grid"], other["origins"], prior=other["prior"], volume=True)
        assert ref["index"][1] >= 0
        for key in KEYS:
            same_bits(res[key][[0, 2, 3, 4]], ref[key][[0, 2, 3, 4]], key)
    finally:
        fwd.close()


def test_refusals_leave_the_outputs_and_the_handle_alone():
    c = make(3, "5x3x2", "both", False, 0)
    fwd = forward_of(c)
    lib, p = lc._lib.load(), lc._lib.ptr
    last = lambda: lib.htm_last_error().decode()
    tc, vs, ac, qs = c["structure"]
    one = lambda v: np.array([float(v)])
    try:
        before = lc.locate(fwd, tc, vs, ac, qs, c["grid"], volume=True)
        loc = np.full((E, 16), 7.25)

        def call(origins, grid=c["grid"], v=vs):
            g = np.array(grid, dtype=np.float64)
            return lib.htm_forward_locate_boxes(fwd.handle, 0, p(tc), p(one(v)), p(ac), p(one(qs)), p(g), p(origins), None, p(loc), None, None)

        assert call(None) == -1 and "NULL origin3" in last()
        for e, a, bad in ((2, 1, np.nan), (4, 2, np.inf), (0, 0, -np.inf)):
            org = c["origins"].copy()
            org[e, a] = bad
            assert call(org) == -1 and f"event {e}: box origin {'xyz'[a]}" in last(), (e, a, last())
        # what the two entry points refuse, with their texts
        assert call(c["origins"], v=0.0) == -1 and "need finite values > 0" in last()
        g = c["grid"].copy()
        g[1] = 0.0
        assert call(c["origins"], grid=g) == -1 and "cell size" in last()
        g = c["grid"].copy()
        g[0] = np.nan                                          # grid9's own origins are checked, though not read
        assert call(c["origins"], grid=g) == -1 and "origin" in last()
        assert lib.htm_forward_locate_boxes(None, 0, p(tc), p(one(vs)), p(ac), p(one(qs)), p(c["grid"]), p(c["origins"]), None, p(loc), None, None) == -1
        assert last() == "NULL handle"
        assert np.all(loc == 7.25)
        with pytest.raises(ValueError, match="origins is"):
            lc.locate_boxes(fwd, tc, vs, ac, qs, c["grid"], c["origins"][:4])
        assert call(c["origins"]) == 0 and not np.all(loc == 7.25)
        after = lc.locate(fwd, tc, vs, ac, qs, c["grid"], volume=True)
        for key in KEYS:
            same_bits(after[key], before[key], key)
    finally:
        fwd.close()


# ---- noise-free recovery -------------------------------------------------------------------------------------------------------
def test_noise_free_recovery_through_the_refinement():
    rec = rc.recovery_case()
    fwd = Forward(12, 6, *rec["sta"], ObsArrays(*rec["obs"]))
    try:
        r2 = lc.refine(fwd, *rec["structure"], rec["grid"], rec["factor"], radius=2)
        r1 = lc.refine(fwd, *rec["structure"], rec["grid"], rec["factor"], radius=1)
    finally:
        fwd.close()
    print("radius 2: index", list(r2["index"]), "worst |best - truth|", np.abs(r2["best"] - rec["truth"]).max(), "mass bound", list(r2["mass_bound"]))
    assert lr.counts(r2["fine_grid"]) == (20, 20, 20) and lr.counts(r1["fine_grid"]) == (12, 12, 12)
    assert list(r2["index"]) == list(rc.truth_index(rec, r2["i0"], r2["fine_grid"]))
    assert np.abs(r2["best"] - rec["truth"]).max() <= 1e-12
    assert not r2["inner_face"].any()
    t1 = rc.truth_index(rec, r1["i0"], r1["fine_grid"])
    assert r1["index"][3] != t1[3] and r1["inner_face"][3]
    assert np.array_equal(r1["coarse_index"], r2["coarse_index"])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end_with_refine(tmp_path, capsys):
    data = cases.e2e_data()
    argv = ["--cell"] + [str(v) for v in cases.E2E_CELL] + ["--bounds"] + [str(v) for v in cases.E2E_BOUNDS]
    text = {}
    for name, extra in (("plain", []), ("refined", ["--refine", "3", "--refine-radius", "1"])):
        d = str(tmp_path / name)
        os.makedirs(d)
        synth.write_dataset(d, data)
        synth.write_param_file(os.path.join(d, "hypo.in"))
        cases.write_structure(d, ["S%03d" % (j + 1) for j in range(16)], np.zeros(16), np.zeros(16), vs=3.0, qs=250.0)
        before = set(os.listdir(d))
        lc.main([os.path.join(d, "hypo.in")] + argv + extra)
        text[name] = {f: open(os.path.join(d, f)).read() for f in set(os.listdir(d)) - before}
        text[name]["out"] = capsys.readouterr().out
    assert sorted(text["plain"]) == ["hypo_grid.best.dat", "hypo_grid.stat", "out"]
    assert sorted(text["refined"]) == ["hypo_grid.best.dat", "hypo_grid.refined.best.dat", "hypo_grid.refined.stat", "hypo_grid.stat", "out"]
    for f in ("hypo_grid.stat", "hypo_grid.best.dat"):
        assert text["refined"][f] == text["plain"][f], f
    out = text["refined"]["out"]
    assert out.startswith(text["plain"]["out"])
    last = out[len(text["plain"]["out"]):]
    assert last.count("\n") == 1 and "boxes of 3 x 3 x 3 coarse cells, 9 x 9 x 9 fine cells" in last and "0.99" in last
    # the medians against the restatement applied to the oracle's volume on each window's 9 x 9 x 9 box
    best = text["refined"]["hypo_grid.refined.best.dat"].split("\n")
    stat = text["refined"]["hypo_grid.refined.stat"].split("\n")
    assert len(best) == 10 and len(stat) == 11 and stat[0] == lc.REFINED_STAT_HEADER and stat[1] == lc.HYPO_HEADER
    sta, obs = cases.arrays(data)
    mu_x, mu_y = ObsData.from_arrays(data.sta_x, data.sta_y, *obs).make_initial_guess()
    par = synth.DEFAULT_PARAMS
    coarse = cases.e2e_reference()["grid"]
    fine_cell = [coarse[3 * a + 1] / 3.0 for a in range(3)]
    zero = np.zeros(16)
    for e in range(8):
        row = best[1 + e].split()
        corner = [float(v) for v in row[11:14]]
        for a in range(3):                                       # the corner is a coarse cell's edge
            k = (corner[a] - coarse[3 * a]) / coarse[3 * a + 1]
            assert k == round(k) and 0 <= k <= coarse[3 * a + 2] - 3, (e, a, corner)
        box = np.array([v for a in range(3) for v in (corner[a], fine_cell[a], 9.0)])
        ell = lr.ell_volume(sta, tuple(o[e:e + 1] for o in obs), True, True, zero, 3.0, zero, 250.0, box)[0]
        lp = ell + lr.log_prior(box, [mu_x[e], mu_y[e], par["prior_width_xy"], par["prior_z"], par["prior_width_z"]])[0]
        want = lr.quantiles(lr.summarise(lp, box)["marg"], box)
        got = [float(stat[2 + e][9 + 13 * k:22 + 13 * k]) for k in range(9)]
        assert int(stat[2 + e][:9]) == data.win_id[e] == int(row[0])
        for a in range(3):
            print(f"window {e} axis {a}: median {got[3 * a]:.6f}, restatement {want[a][1]:.6f}, fine cell {fine_cell[a]:.4f}")
            assert abs(got[3 * a] - want[a][1]) <= fine_cell[a], (e, a)
