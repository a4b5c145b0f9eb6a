"""What `locate.main` asks of the library, in which order, and what it writes, per option set: the five library-facing calls
and Forward are replaced by recorders that return small canned results, so no device is needed.  The parameter file, the data
and the calibration run's files are real ones under tmp_path."""
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from hypotremormcmc_amd.grid import grid_counts
from tests import locate_cases as cases
from tests import locate_marginal_cases as mc

NAMES = ["S%03d" % (j + 1) for j in range(16)]
CELL, BOUNDS = ["30", "30", "10"], ["-45", "45", "-45", "45", "0", "20"]      # 3 x 3 x 2 cells


class Recorder:
    """Forward and the five calls: every one appends (name, events of its Forward, what main chose for it) to `calls`"""

    def __init__(self, monkeypatch):
        self.calls, self.results = [], []
        rec = self

        class FakeForward:
            def __init__(self, n_sta, n_events, sta_x, sta_y, sta_z, obs, use_amp=True, use_time=True, device=0):
                self.n_sta, self.n_events, self.locate_precision = n_sta, n_events, "fp64"
                rec.calls.append(("Forward", n_events))

            def set_locate_precision(self, precision):
                self.locate_precision = precision
                rec.calls.append(("precision", precision))

            def close(self):
                rec.calls.append(("close", self.n_events))

        monkeypatch.setattr(lc, "Forward", FakeForward)
        for name in ("locate", "locate_marginal", "draw_evidence", "stack", "residuals"):
            monkeypatch.setattr(lc, name, getattr(self, name))

    def _located(self, fwd, grid, marginals=True, volume=False):
        E, (nx, ny, nz) = fwd.n_events, grid_counts(grid)
        marg = [np.full((E, n), 1.0 / n) if marginals else None for n in (nx, ny, nz)]
        # (every call another best cell, so that the files tell which call they were written from)
        res = {"index": (np.arange(E, dtype=np.int64) + len(self.results)) % (nx * ny * nz), "best": np.ones((E, 3)), "lp": np.full(E, -2.0), "ell": np.full(E, -1.0),
               "log_evidence": np.full(E, -3.0), "mean": np.full((E, 3), 0.5), "marg_x": marg[0], "marg_y": marg[1], "marg_z": marg[2],
               "vol": np.arange(E * nz * ny * nx, dtype=np.float64).reshape(E, nz, ny, nx) if volume else None}
        self.results.append(res)
        return res

    def locate(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, marginals=True, volume=False, precision=None):
        assert np.ndim(vs) == 0 and np.shape(t_corr) == (16,) and precision is None
        self.calls.append(("locate", fwd.n_events, dict(marginals=marginals, volume=volume, prior=prior is not None)))
        return self._located(fwd, grid, marginals, volume)

    def locate_marginal(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, marginals=True, volume=False, precision=None):
        assert np.shape(vs) == (4,) and np.shape(t_corr) == (4, 16) and precision is None
        self.calls.append(("locate_marginal", fwd.n_events, dict(marginals=marginals, volume=volume, prior=prior is not None)))
        return self._located(fwd, grid, marginals, volume)

    def draw_evidence(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, precision=None):
        assert np.shape(vs) == (4,) and precision is None
        self.calls.append(("draw_evidence", fwd.n_events, dict(prior=prior is not None)))
        E = fwd.n_events
        res = {"log_z": np.tile(-np.arange(4.0), (E, 1)), "n_eff": np.full(E, 2.5), "w_max": np.full(E, 0.6), "k_max": np.zeros(E, dtype=np.int64),
               "log_evidence": np.full(E, -3.0)}
        self.results.append(res)
        return res

    def stack(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, layer=None, n_layer=1, volume=False, precision=None):
        assert precision is None
        self.calls.append(("stack", fwd.n_events, dict(layer=None if layer is None else [int(v) for v in layer], n_layer=n_layer, volume=volume,
                                                       prior=prior is not None)))
        nx, ny, nz = grid_counts(grid)
        res = self._located(fwd, grid)
        res.update(xy=np.ones((n_layer, ny, nx)), xz=np.ones((n_layer, nz, nx)), yz=np.ones((n_layer, nz, ny)), stack=np.ones((n_layer, nz, ny, nx)),
                   tally=np.array([[fwd.n_events, 0.0]] * n_layer))
        return res

    def residuals(self, fwd, t_corr, vs, a_corr, qs, grid, prior=None, precision=None):
        assert np.ndim(vs) == 0 and precision is None
        self.calls.append(("residuals", fwd.n_events, dict(prior=prior is not None)))
        res = self._located(fwd, grid)
        res.update(res=np.full((fwd.n_events, 16, 4), 0.25), fit=np.full((fwd.n_events, 10), 1.5))
        return res


@pytest.fixture
def job(tmp_path, monkeypatch):
    """(data directory, leading arguments, the windows' ids, recorder)"""
    data = cases.e2e_data()
    d, cal = str(tmp_path / "data"), str(tmp_path / "calibration")
    os.makedirs(d)
    os.makedirs(cal)
    synth.write_dataset(d, data)
    synth.write_param_file(os.path.join(d, "hypo.in"))
    mc.write_calibration(cal, NAMES, n_ranks=2, n_rec=6, vs=3.0, qs=250.0)
    return d, [os.path.join(d, "hypo.in"), "--cell"] + CELL + ["--bounds"] + BOUNDS + ["--structure", cal], [int(w) for w in data.win_id], Recorder(monkeypatch)


def one(n, *calls):
    """a Forward of n windows in fp64, the calls on it, its end"""
    return [("Forward", n), ("precision", "fp64")] + [(c[0], n) + c[1:] for c in calls] + [("close", n)]


PLAIN = dict(marginals=True, volume=False, prior=True)
FILES = ["hypo_grid.stat", "hypo_grid.best.dat"]
DENSITY = ["hypo_grid.density.%s.dat" % nm for nm in ("xy", "xz", "yz")]
RESIDUALS = ["hypo_grid.%s.dat" % nm for nm in ("residuals", "fit", "stations")]
# the first window's id is 1: cases.e2e_data numbers them from 1
OPTION_SETS = {
    "plain": ([], one(8, ("locate", PLAIN)), FILES, 2),
    "draw-weights": (["--draws", "4", "--draw-weights"], one(8, ("locate_marginal", PLAIN), ("draw_evidence", dict(prior=True))),
                     ["hypo_grid_marginal." + nm for nm in ("stat", "best.dat", "draws.dat", "structure.dat")], 3),
    # the recorders' best cells are cells 0 .. 7 of the 3 x 3 x 2 box: every one lies on a face
    "stack-resolved": (["--stack", "--stack-resolved"],
                       one(8, ("locate", dict(marginals=False, volume=False, prior=True)),
                           ("stack", dict(layer=[-1] * 8, n_layer=1, volume=True, prior=True))), FILES + DENSITY, 4),
    "stack-residuals": (["--stack", "--residuals"], one(8, ("stack", dict(layer=[0] * 8, n_layer=1, volume=True, prior=True)), ("residuals", dict(prior=True))),
                        FILES + DENSITY + RESIDUALS, 4),
    "residuals": (["--residuals"], one(8, ("residuals", dict(prior=True))), FILES + RESIDUALS, 3),
    "volume-of": (["--volume-of", "1", "--flat-prior"], one(8, ("locate", dict(marginals=True, volume=False, prior=False)))
                  + one(1, ("locate", dict(marginals=True, volume=True, prior=False))), FILES + ["hypo_grid.1.vol.dat"], 2),
}


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_main_calls_and_files(name, job, capsys):
    d, argv, win_id, rec = job
    extra, calls, files, n_lines = OPTION_SETS[name]
    before = set(os.listdir(d))
    lc.main(argv + extra)
    assert rec.calls == calls
    assert sorted(set(os.listdir(d)) - before) == sorted(files)
    out = capsys.readouterr().out
    assert out.count("\n") == n_lines and out.startswith("8 windows located on 3 x 3 x 2 cells")
    # .stat and .best.dat come from the call that the option set names for them: the stack's with --stack, the residuals' with
    # --residuals alone, the first evaluation otherwise
    stem = files[0][:-len(".stat")]
    serving = {"stack-resolved": 1, "stack-residuals": 0}.get(name, 0)
    grid = [-45.0, 30.0, 3, -45.0, 30.0, 3, 0.0, 10.0, 2]
    assert open(os.path.join(d, stem + ".best.dat")).read() == lc.best_text(win_id, rec.results[serving], grid)


def test_volume_of_an_unknown_window_is_refused_after_the_evaluation(job):
    d, argv, _, rec = job
    with pytest.raises(SystemExit, match="--volume-of 999 is not among the windows"):
        lc.main(argv + ["--volume-of", "999"])
    assert rec.calls == one(8, ("locate", PLAIN)) and os.path.exists(os.path.join(d, "hypo_grid.best.dat"))
