"""CPU: what the coarse-to-fine refinement of `locate` decides without a device -- the plan of a request with
a box per event, the refinement policy (locate.refine_boxes), the mass bound, `refine`'s order of calls, masking and flags, and
what `locate.main` asks for and writes under --refine -- and the recovery construction that tests/test_gpu_locate_refine.py
holds the device to, re-checked here with plain numpy."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import _lib
from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from hypotremormcmc_amd.grid import grid_counts
from tests import locate_cases as cases
from tests import locate_marginal_cases as mc
from tests import locate_refine_cases as rc
from tests import locate_restatement as lr
from tests.test_locate_plan import restated

GRID = cases.GRIDS["67x3x5"]
BOXES_REFUSED = "a box per event comes under a fixed structure or its mixture over draws, without a stack and without residuals"


# ---- the plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("job,K", [("fixed", 0), ("marginal", 9)])
@pytest.mark.parametrize("volume,prior", [(False, False), (True, True)])
def test_boxes_add_32_bytes_per_event(job, K, volume, prior, monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    kw = dict(n_sta=65, n_events=5, grid=GRID, job=job, n_draws=K, volume=volume, prior=prior)
    plain, boxes = lc.plan(**kw), lc.plan(boxes=True, **kw)
    assert boxes["per_event_bytes"] == plain["per_event_bytes"] + 32.0
    assert boxes["per_event"].pop("org") == 4 and "org" not in plain["per_event"]
    assert boxes["nb_limit"][:3] == plain["nb_limit"][:3]          # (the fourth, the budget's, follows the bytes: the next test)
    for key in plain:
        if key not in ("per_event_bytes", "nb_limit"):
            assert boxes[key] == plain[key], key
    # a request without boxes has the dict it had: the restatement of tests/test_locate_plan.py, key for key
    want = restated(65, 5, GRID, 1024.0, job=job, n_draws=K, volume=volume, prior=prior)[0]
    assert plain == want and list(plain["per_event"]) == list(_lib.LocatePlan.PER_EVENT)


@pytest.mark.parametrize("job,K", [("fixed", 0), ("marginal", 9)])
def test_the_batch_follows_the_boxes_bytes(job, K, monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    kw = dict(n_sta=65, n_events=70, grid=GRID, job=job, n_draws=K, volume=True, prior=True)
    plain = lc.plan(**kw)
    mb = (plain["table_bytes"] + 5.0 * plain["per_event_bytes"] + 16.0) / 1048576.0      # five plain events fit, with 16 bytes to spare
    monkeypatch.setenv("HTM_LOCATE_MB", repr(mb))
    plain, boxes = lc.plan(**kw), lc.plan(boxes=True, **kw)
    budget = float(repr(mb)) * 1048576.0
    for p in (plain, boxes):
        assert p["nb"] == p["nb_limit"][3] == int((budget - p["table_bytes"]) / p["per_event_bytes"])
    assert plain["nb"] == 5 and boxes["nb"] == 4


@pytest.mark.parametrize("kw", [dict(job="draw_evidence", n_draws=8), dict(n_layer=1), dict(residuals=True)])
def test_boxes_are_refused_where_no_entry_point_takes_them(kw):
    lc.plan(65, 5, GRID, **kw)                                    # the request itself is one that an entry point makes
    with pytest.raises(_lib.HtmError) as e:
        lc.plan(65, 5, GRID, boxes=True, **kw)
    assert str(e.value) == "libhtm_hip error -1: " + BOXES_REFUSED
    assert sorted(lc.JOBS) == ["draw_evidence", "fixed", "marginal"]


# ---- refine_boxes ----------------------------------------------------------------------------------------------------------
COARSE = np.array([-40.0, 8.0, 10, -24.0, 6.0, 7, 2.0, 3.0, 4])      # 10 x 7 x 4 cells


def lin(ix, iy, iz, n=(10, 7, 4)):
    return ix + n[0] * (iy + n[1] * iz)


def test_refine_boxes_middle_faces_corner_short_axis():
    # the middle; each of the six faces; a corner; with R = 2 the z axis (4 cells) is shorter than 2 R + 1: the width is the axis
    cells = [(5, 3, 2), (0, 3, 1), (9, 3, 1), (5, 0, 1), (5, 6, 1), (5, 3, 0), (5, 3, 3), (9, 6, 3), (0, 0, 0), (1, 5, 2)]
    index = np.array([lin(*c) for c in cells])
    for R, F in ((2, 4), (1, 3), (0, 5)):
        bx = lc.refine_boxes(index, COARSE, F, R)
        n = grid_counts(COARSE)
        w = tuple(min(2 * R + 1, n[a]) for a in range(3))
        assert bx["widths"] == w and not bx["none"].any()
        assert (w[2] == 4) == (R == 2)
        for a in range(3):
            want = np.array([min(max(c[a] - R, 0), n[a] - w[a]) for c in cells])
            assert np.array_equal(bx["i0"][:, a], want), (R, a)
            assert np.all(bx["i0"][:, a] + w[a] <= n[a]) and np.all(bx["i0"][:, a] >= 0)
            # the box holds the best cell
            assert np.all((bx["i0"][:, a] <= [c[a] for c in cells]) & ([c[a] for c in cells] < bx["i0"][:, a] + w[a]))
            # the origin: one multiplication, then one addition
            assert np.array_equal(bx["origins"][:, a], COARSE[3 * a] + bx["i0"][:, a].astype(np.float64) * COARSE[3 * a + 1])
            assert bx["fine_grid"][3 * a] == COARSE[3 * a] and bx["fine_grid"][3 * a + 1] == COARSE[3 * a + 1] / F
            assert bx["fine_grid"][3 * a + 2] == w[a] * F
            # the fine cells are cells of the whole-box grid of cell dv / F
            whole = lr.centres(rc.fine_whole_grid(COARSE, F), a)
            dv = COARSE[3 * a + 1] / F
            for e in range(len(cells)):
                own = bx["origins"][e, a] + (np.arange(w[a] * F) + 0.5) * dv
                assert np.allclose(own, whole[bx["i0"][e, a] * F:(bx["i0"][e, a] + w[a]) * F], rtol=0.0, atol=4 * np.spacing(50.0)), (R, a, e)
    # R = 0: the box is the best cell itself
    bx = lc.refine_boxes(index, COARSE, 5, 0)
    assert bx["widths"] == (1, 1, 1) and np.array_equal(bx["i0"], np.array(cells))


def test_refine_boxes_marks_a_window_without_a_cell():
    bx = lc.refine_boxes(np.array([lin(5, 3, 2), -1, lin(9, 6, 3)]), COARSE, 4, 1)
    assert list(bx["none"]) == [False, True, False] and list(bx["i0"][1]) == [0, 0, 0]
    assert list(bx["origins"][1]) == [-40.0, -24.0, 2.0] and list(bx["i0"][2]) == [7, 4, 1]
    for bad in (dict(factor=0, radius=1), dict(factor=2, radius=-1), dict(factor=2.5, radius=1)):
        with pytest.raises(ValueError, match="factor"):
            lc.refine_boxes(np.array([0]), COARSE, **bad)


# ---- box_mass_bound --------------------------------------------------------------------------------------------------------
def test_box_mass_bound():
    mx, my, mz = np.zeros((3, 10)), np.zeros((3, 7)), np.zeros((3, 4))
    i0 = np.array([[3, 2, 0], [3, 2, 0], [0, 0, 0]])
    w = (3, 3, 4)
    mx[0, 4] = my[0, 3] = mz[0, 1] = 1.0                         # one cell, inside the box: 1
    mx[1, 4], mx[1, 6] = 0.75, 0.25                              # a quarter of the mass beyond the box's edge in x,
    my[1, 1], my[1, 2] = 0.125, 0.875                            # an eighth below it in y: 1 - (0.25 + 0.125 + 0)
    mz[1, 3] = 1.0
    mx[2], my[2], mz[2] = np.nan, np.nan, np.nan
    mx[2, 0] = 1.0
    got = lc.box_mass_bound(mx, my, mz, i0, w)
    assert got[0] == 1.0 and got[1] == 1.0 - (0.25 + 0.125) and np.isnan(got[2])
    # the bound is floored at 0
    mx[1], my[1] = 0.0, 0.0
    mx[1, 9], my[1, 6] = 1.0, 1.0
    assert lc.box_mass_bound(mx, my, mz, i0, w)[1] == 0.0


def test_marginal_quantiles_take_an_origin_per_event():
    rng = np.random.default_rng(5)
    m = rng.uniform(0.1, 1.0, (3, 5 + 3 + 2))
    for s in (slice(0, 5), slice(5, 8), slice(8, 10)):
        m[:, s] /= m[:, s].sum(axis=1, keepdims=True)
    grid = cases.GRIDS["5x3x2"]
    org = rng.uniform(-30, 30, (3, 3))
    got = lc.marginal_quantiles(m, grid, origin=org)
    for e in range(3):
        ge = grid.copy()
        ge[0::3] = org[e]
        assert np.array_equal(got[e], lc.marginal_quantiles(m[e], ge))
    assert np.array_equal(lc.marginal_quantiles(m, grid), lc.marginal_quantiles(m, grid, origin=np.tile(grid[0::3], (3, 1))))


# ---- refine, the library's calls replaced by recorders -------------------------------------------------------------------------
class FakeForward:
    n_sta, n_events = 4, 4


def fake_result(E, grid, index):
    nx, ny, nz = grid_counts(grid)
    return {"index": np.asarray(index, dtype=np.int64), "best": np.ones((E, 3)), "lp": np.full(E, -2.0), "ell": np.full(E, -1.0),
            "log_evidence": np.full(E, -3.0), "mean": np.full((E, 3), 0.5), "cov": np.ones((E, 3, 3)), "loc": np.ones((E, 16)),
            "marg_x": np.full((E, nx), 1.0 / nx), "marg_y": np.full((E, ny), 1.0 / ny), "marg_z": np.full((E, nz), 1.0 / nz), "vol": None}


def test_refine_calls_masks_and_flags(monkeypatch):
    calls = []
    # window 0 in the middle, window 1 without a cell, window 2 in the outer box's upper corner, window 3 at its lower x face
    coarse_index = [lin(5, 3, 2), -1, lin(9, 6, 3), lin(0, 3, 1)]
    # fine cells within the 12 x 12 x 12 boxes (R = 1, F = 4): window 0 on its box's lower x face (inner), window 2 on the upper x
    # face (the outer box's) and the lower y face (inner), window 3 on the lower x face (the outer box's) only
    fine_index = [0 + 12 * (5 + 12 * 5), 7, 11 + 12 * (0 + 12 * 5), 0 + 12 * (5 + 12 * 5)]

    def locate(fwd, t_corr, vs, a_corr, qs, grid, prior=None, marginals=True, volume=False, precision=None):
        calls.append(("locate", precision))
        return fake_result(4, grid, coarse_index)

    def locate_marginal(*a, **kw):
        calls.append(("locate_marginal", kw.get("precision")))
        return fake_result(4, a[5], coarse_index)

    def locate_boxes(fwd, t_corr, vs, a_corr, qs, grid, origins, prior=None, marginals=True, volume=False, precision=None):
        calls.append(("locate_boxes", precision, list(grid), np.array(origins)))
        return dict(fake_result(4, grid, fine_index), origin=np.array(origins))

    for name, f in (("locate", locate), ("locate_marginal", locate_marginal), ("locate_boxes", locate_boxes)):
        monkeypatch.setattr(lc, name, f)
    res = lc.refine(FakeForward(), np.zeros(4), 3.0, np.zeros(4), 250.0, COARSE, 4, radius=1, precision="fp32")
    assert [c[:2] for c in calls] == [("locate", "fp32"), ("locate_boxes", "fp32")]
    bx = lc.refine_boxes(coarse_index, COARSE, 4, 1)
    assert calls[1][2] == list(bx["fine_grid"]) and np.array_equal(calls[1][3], bx["origins"])
    assert list(res["coarse_index"]) == coarse_index and np.array_equal(res["i0"], bx["i0"]) and res["widths"] == (3, 3, 3)
    # the window without a coarse cell comes back without a cell
    assert list(res["index"]) == [fine_index[0], -1, fine_index[2], fine_index[3]]
    for key in ("best", "lp", "ell", "log_evidence", "mean", "cov", "marg_x", "marg_y", "marg_z"):
        assert np.isnan(res[key][1]).all() and not np.isnan(res[key][[0, 2, 3]]).any(), key
    assert res["loc"][1, 0] == -1.0 and np.isnan(res["loc"][1, 1:]).all()
    assert list(res["inner_face"]) == [True, False, True, False] and list(res["outer_face"]) == [False, False, True, True]
    # the recorders' flat marginals: 3 of 10, 3 of 7, 3 of 4 cells
    assert np.allclose(res["mass_bound"][[0, 2, 3]], max(0.0, 1.0 - (0.7 + 4.0 / 7.0 + 0.25))) and np.isnan(res["mass_bound"][1])
    # draws are told as `stack` tells them; a coarse result handed in is not evaluated again
    del calls[:]
    lc.refine(FakeForward(), np.zeros((2, 4)), np.full(2, 3.0), np.zeros((2, 4)), np.full(2, 250.0), COARSE, 2)
    assert [c[0] for c in calls] == ["locate_marginal", "locate_boxes"] and calls[1][2][2::3] == [10.0, 10.0, 8.0]
    del calls[:]
    lc.refine(FakeForward(), np.zeros(4), 3.0, np.zeros(4), 250.0, COARSE, 2, coarse=fake_result(4, COARSE, coarse_index))
    assert [c[0] for c in calls] == ["locate_boxes"]


# ---- the recovery construction, with numpy --------------------------------------------------------------------------------------
def test_recovery_construction():
    """what tests/test_gpu_locate_refine.py asks of the device holds for a plain numpy evaluation: radius 2 recovers all six
    truths with a clear best cell and no flag; radius 1 misses window 3, whose best coarse cell lies two cells from the truth,
    and flags it"""
    rec = rc.recovery_case()
    r2 = rc.numpy_refine(rec, 2)
    assert np.array_equal(r2["index"], rc.truth_index(rec, r2["i0"], r2["fine_grid"])) and not r2["inner_face"].any()
    assert np.abs(r2["best"] - rec["truth"]).max() <= 1e-12 and r2["gap"].min() > 0.5
    r1 = rc.numpy_refine(rec, 1)
    miss = r1["index"] != rc.truth_index(rec, r1["i0"], r1["fine_grid"])
    assert list(miss) == [False, False, False, True, False, False] and list(r1["inner_face"]) == list(miss)
    n = grid_counts(rec["grid"])
    coarse = np.stack([r1["coarse_index"] % n[0], (r1["coarse_index"] // n[0]) % n[1], r1["coarse_index"] // (n[0] * n[1])], axis=1)
    assert np.abs(coarse[3] - rec["cell"][3] // rec["factor"]).max() >= 2


# ---- main, the library's calls replaced by recorders (as tests/test_locate_main.py builds them) ---------------------------------
NAMES = ["S%03d" % (j + 1) for j in range(16)]
CELL, BOUNDS = ["30", "30", "10"], ["-45", "45", "-45", "45", "0", "20"]      # 3 x 3 x 2 cells


class Recorder:
    """Forward and the calls: every one appends (name, events of its Forward, what main chose for it) to `calls`"""

    def __init__(self, monkeypatch):
        self.calls, self.results = [], []
        rec = self

        class Forward:
            def __init__(self, n_sta, n_events, sta_x, sta_y, sta_z, obs, use_amp=True, use_time=True, device=0):
                self.n_sta, self.n_events, self.locate_precision = n_sta, n_events, "fp64"
                rec.calls.append(("Forward", n_events))

            def set_locate_precision(self, precision):
                self.locate_precision = precision
                rec.calls.append(("precision", precision))

            def close(self):
                rec.calls.append(("close", self.n_events))

        monkeypatch.setattr(lc, "Forward", Forward)
        for name in ("locate", "locate_marginal", "residuals", "locate_boxes"):
            monkeypatch.setattr(lc, name, getattr(self, name))

    def _located(self, fwd, grid):
        E, (nx, ny, nz) = fwd.n_events, grid_counts(grid)
        # (every call another best cell, so that the files tell which call they were written from)
        res = fake_result(E, grid, (np.arange(E, dtype=np.int64) + len(self.results)) % (nx * ny * nz))
        self.results.append(res)
        return res

    def locate(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, marginals=True, volume=False, precision=None):
        assert np.ndim(vs) == 0 and precision is None
        self.calls.append(("locate", fwd.n_events, dict(marginals=marginals, volume=volume, prior=prior is not None)))
        return self._located(fwd, grid)

    def locate_marginal(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, marginals=True, volume=False, precision=None):
        assert np.shape(vs) == (4,) and precision is None
        self.calls.append(("locate_marginal", fwd.n_events, dict(marginals=marginals, volume=volume, prior=prior is not None)))
        return self._located(fwd, grid)

    def residuals(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, precision=None):
        assert np.ndim(vs) == 0 and precision is None
        self.calls.append(("residuals", fwd.n_events, dict(prior=prior is not None)))
        res = self._located(fwd, grid)
        res.update(res=np.full((fwd.n_events, 16, 4), 0.25), fit=np.full((fwd.n_events, 10), 1.5))
        return res

    def locate_boxes(self, fwd, t_corr, vs, a_corr, qs, grid, origins, prior=None, marginals=True, volume=False, precision=None):
        assert precision is None and np.shape(origins) == (fwd.n_events, 3)
        self.calls.append(("locate_boxes", fwd.n_events, dict(draws=np.ndim(vs) == 1, counts=grid_counts(grid), prior=prior is not None)))
        return dict(self._located(fwd, grid), origin=np.array(origins, dtype=np.float64))


@pytest.fixture
def job(tmp_path):
    """(data directory, leading arguments, the windows' ids)"""
    data = cases.e2e_data()
    d, cal = str(tmp_path / "data"), str(tmp_path / "calibration")
    os.makedirs(d)
    os.makedirs(cal)
    synth.write_dataset(d, data)
    synth.write_param_file(os.path.join(d, "hypo.in"))
    mc.write_calibration(cal, NAMES, n_ranks=2, n_rec=6, vs=3.0, qs=250.0)
    return d, [os.path.join(d, "hypo.in"), "--cell"] + CELL + ["--bounds"] + BOUNDS + ["--structure", cal], [int(w) for w in data.win_id]


def one(n, *calls):
    return [("Forward", n), ("precision", "fp64")] + [(c[0], n) + c[1:] for c in calls] + [("close", n)]


PLAIN = dict(marginals=True, volume=False, prior=True)
RESIDUALS = ["hypo_grid.%s.dat" % nm for nm in ("residuals", "fit", "stations")]
# the box of --refine 4 at the default radius 2 is the whole 3 x 3 x 2 grid: 12 x 12 x 8 fine cells
BOXES = dict(counts=(12, 12, 8), prior=True)
OPTION_SETS = {
    "refine": ([], "hypo_grid", ("locate", PLAIN), dict(BOXES, draws=False), []),
    "refine-draws": (["--draws", "4"], "hypo_grid_marginal", ("locate_marginal", PLAIN), dict(BOXES, draws=True), []),
    "refine-residuals": (["--residuals"], "hypo_grid", ("residuals", dict(prior=True)), dict(BOXES, draws=False), RESIDUALS),
}


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_main_calls_and_files_under_refine(name, job, monkeypatch, capsys):
    d, argv, win_id = job
    extra, stem, first, boxes, more = OPTION_SETS[name]
    before = set(os.listdir(d))
    # without --refine: what the invocation writes and prints anyway
    rec = Recorder(monkeypatch)
    lc.main(argv + extra)
    assert rec.calls == one(8, first)
    plain_files = sorted(set(os.listdir(d)) - before)
    assert plain_files == sorted([stem + ".stat", stem + ".best.dat"] + more)
    plain_text = {f: open(os.path.join(d, f)).read() for f in plain_files}
    plain_out = capsys.readouterr().out
    for f in plain_files:
        os.remove(os.path.join(d, f))
    # with it: one more call on the same Forward, behind the others; two more files; one more line
    rec = Recorder(monkeypatch)
    lc.main(argv + extra + ["--refine", "4"])
    assert rec.calls == one(8, first, ("locate_boxes", boxes))
    files = sorted(set(os.listdir(d)) - before)
    assert files == sorted(plain_files + [stem + ".refined.stat", stem + ".refined.best.dat"])
    for f in plain_files:
        assert open(os.path.join(d, f)).read() == plain_text[f], f
    out = capsys.readouterr().out
    assert out.startswith(plain_out) and out[len(plain_out):].count("\n") == 1
    last = out[len(plain_out):]
    assert "boxes of 3 x 3 x 2 coarse cells, 12 x 12 x 8 fine cells" in last and "0.99" in last and " 0 windows with the best fine cell on an inner face" in last
    # the refined files come from the fine call's result, the second
    fine = rec.results[1]
    stat = open(os.path.join(d, stem + ".refined.stat")).read().split("\n")
    assert stat[0] == lc.REFINED_STAT_HEADER and "conditional" in stat[0] and stat[1] == lc.HYPO_HEADER and len(stat) == 11
    best = open(os.path.join(d, stem + ".refined.best.dat")).read().split("\n")
    assert best[0].startswith(lc.BEST_HEADER) and len(best) == 10
    row = best[1].split()
    assert int(row[0]) == win_id[0] and len(row) == 17 and [float(v) for v in row[11:14]] == [-45.0, -45.0, 0.0]
    assert float(row[14]) == 1.0 and row[15:] == ["0", "1"] and float(row[4]) == fine["lp"][0]


def test_refine_argument_errors(job, monkeypatch, capsys):
    d, argv, _ = job
    rec = Recorder(monkeypatch)
    for extra, text in ((["--refine-radius", "1"], "--refine-radius needs --refine"), (["--refine", "1"], "--refine 1"),
                        (["--refine", "0"], "--refine 0"), (["--refine", "3", "--refine-radius", "-1"], "--refine-radius -1")):
        with pytest.raises(SystemExit) as e:
            lc.main(argv + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    assert rec.calls == []
    lc.main(argv + ["--refine", "2", "--refine-radius", "0"])                  # R = 0: the box is the best cell, 2 x 2 x 2 fine cells
    assert rec.calls[3] == ("locate_boxes", 8, dict(draws=False, counts=(2, 2, 2), prior=True))
