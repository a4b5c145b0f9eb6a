"""Stacked density maps on the device (hypotremormcmc_amd/csrc/htm_density.hpp) against the numpy restatement
(tests/density_restatement.py) at the smallest shapes and grids where the kernels can go wrong, and end to end on the files of
a small step-5 run.  The counts are integers: every comparison is exact equality of uint64 arrays."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from hypotremormcmc_amd import density as dn
from tests import density_restatement as dr
from tests.helpers import load_case, write_fake_samples, write_run_dir

pytestmark = pytest.mark.gpu

# (n_mod, n_win)
SHAPES = [
    (1, 1),
    (3, 21),            # 63 columns
    (5, 22),            # 66 columns: window 21 straddles the 64-lane boundary of the first load
    (7, 64),            # exactly one wave's 192 columns
    (9, 65),            # one window past a wave
    (1001, 43),         # rows not a multiple of anything
    (4100, 130),        # several row slabs by default, three waves of a workgroup
]
_LNY, _LNZ = 8, 4
_LNX = (dn.LDS_MAX_CELLS - _LNY * _LNZ) // (_LNY + _LNZ)          # the most cells on x that the LDS path takes beside 8 x 4
GRIDS = {
    "1x1x1": (-1.0, 2.0, 1.0, 5.0, 3.0, 1.0, 20.0, 40.0, 1.0),
    "3x2x5": (-3.0, 0.7, 3.0, 10.0, 1.3, 2.0, 0.5, 2.1, 5.0),     # unequal on purpose: a transposed index fails it
    "lds_max": (0.0, 0.01, float(_LNX), -2.0, 0.5, float(_LNY), 3.0, 1.5, float(_LNZ)),
    "lds_max+1": (0.0, 0.01, float(_LNX + 1), -2.0, 0.5, float(_LNY), 3.0, 1.5, float(_LNZ)),
    "4096x1x1": (100.0, 0.25, 4096.0, 0.0, 1.0, 1.0, -7.0, 2.0, 1.0),
}
ENV = ("HTM_DENSITY_LDS", "HTM_DENSITY_SLABS", "HTM_DENSITY_MB", "HTM_DENSITY_NAIVE")
_ids = lambda s: "x".join(map(str, s))


def _clean(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def test_the_two_lds_grids_sit_on_the_limit():
    assert dn.lds_fits(GRIDS["lds_max"]) and not dn.lds_fits(GRIDS["lds_max+1"])
    nx, ny, nz = dn.grid_counts(GRIDS["lds_max"])
    assert nx * ny + nx * nz + ny * nz > dn.LDS_MAX_CELLS - (ny + nz)          # one more cell on x no longer fits


@functools.lru_cache(maxsize=None)
def _samples(n_mod, n_win, grid_name):
    """clustered windows: per window a centre drawn over the box widened by a tenth of its size on every side (about a tenth of
    the samples outside on each side), samples about it with a standard deviation of one cell.  Made once."""
    g = np.array(GRIDS[grid_name]).reshape(3, 3)
    rng = np.random.default_rng(1000 * n_mod + n_win + sum(map(ord, grid_name)))
    centre = rng.uniform(-0.1 * g[:, 2], 1.1 * g[:, 2], size=(n_win, 3))
    q = centre[None, :, :] + rng.normal(size=(n_mod, n_win, 3))
    x = (g[:, 0] + q * g[:, 1]).reshape(n_mod, 3 * n_win)
    x.setflags(write=False)
    return x


def _layers(n_win):
    """4 layers: 0, 1, 2 interleaved by window, nobody in 3; window 4 (where there is one) has -1 and the last window of a
    set of more than 8 has n_layer: neither takes part"""
    lay = (np.arange(n_win) % 3).astype(np.int32)
    if n_win > 4:
        lay[4] = -1
    if n_win > 8:
        lay[-1] = 4
    return lay, 4


@functools.lru_cache(maxsize=None)
def _reference(n_mod, n_win, grid_name, layered):
    x = _samples(n_mod, n_win, grid_name)
    lay, n_layer = _layers(n_win) if layered else (None, 1)
    ref = dr.density(x, GRIDS[grid_name], lay, n_layer)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _equal(got, ref, what=""):
    for nm in ("xy", "xz", "yz", "tally"):
        assert got[nm].dtype == np.uint64 and np.array_equal(got[nm], ref[nm]), (what, nm)
    if got["vol"] is not None:
        assert got["vol"].dtype == np.uint64 and np.array_equal(got["vol"], ref["vol"]), (what, "vol")


@pytest.mark.parametrize("grid_name", list(GRIDS))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_device_equals_restatement(shape, grid_name, monkeypatch):
    """four layers of which one is empty, windows that take no part; with the volume and without it"""
    _clean(monkeypatch)
    n_mod, n_win = shape
    x, grid = _samples(n_mod, n_win, grid_name), GRIDS[grid_name]
    lay, n_layer = _layers(n_win)
    ref = _reference(n_mod, n_win, grid_name, True)
    if n_mod * n_win > 100:
        assert ref["tally"][:, 0].sum() > 0 and ref["tally"][:, 1].sum() > 0
    if grid_name == "lds_max" and n_mod > 1000:         # about a tenth of the centres outside on each side of each axis
        assert 0.15 < int(ref["tally"][:, 1].sum()) / float(ref["tally"].sum()) < 0.75
    assert ref["tally"][3].tolist() == [0, 0] and not ref["xy"][3].any()
    with_vol = dn.density(x, grid, layer=lay, n_layer=n_layer, volume=True)
    _equal(with_vol, ref, "volume")
    maps_only = dn.density(x, grid, layer=lay, n_layer=n_layer)
    assert maps_only["vol"] is None
    _equal(maps_only, ref, "maps only")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_without_layers(shape, monkeypatch):
    _clean(monkeypatch)
    x = _samples(*shape, "3x2x5")
    _equal(dn.density(x, GRIDS["3x2x5"], volume=True), _reference(*shape, "3x2x5", False))


@pytest.mark.parametrize("lds", [None, "0", "1"])
@pytest.mark.parametrize("grid_name", ["lds_max", "lds_max+1"])
@pytest.mark.parametrize("shape", [(1001, 43), (4100, 130)], ids=_ids)
def test_lds_switch_at_the_limit(shape, grid_name, lds, monkeypatch):
    _clean(monkeypatch)
    if lds is not None:
        monkeypatch.setenv("HTM_DENSITY_LDS", lds)
    x, grid = _samples(*shape, grid_name), GRIDS[grid_name]
    lay, n_layer = _layers(shape[1])
    if lds == "1" and grid_name == "lds_max+1":
        with pytest.raises(dn._lib.HtmError, match=r"error -1: HTM_DENSITY_LDS = 1, but"):
            dn.density(x, grid, layer=lay, n_layer=n_layer)
        return
    _equal(dn.density(x, grid, layer=lay, n_layer=n_layer, volume=True), _reference(*shape, grid_name, True), "lds=%s" % lds)


@pytest.mark.parametrize("slabs", ["1", "2", "7"])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_row_slabs(slabs, lds, monkeypatch):
    _clean(monkeypatch)
    monkeypatch.setenv("HTM_DENSITY_SLABS", slabs)
    monkeypatch.setenv("HTM_DENSITY_LDS", lds)
    lay, n_layer = _layers(43)
    got = dn.density(_samples(1001, 43, "3x2x5"), GRIDS["3x2x5"], layer=lay, n_layer=n_layer, volume=True)
    _equal(got, _reference(1001, 43, "3x2x5", True), "slabs=%s lds=%s" % (slabs, lds))


@pytest.mark.parametrize("path", ["lds", "plain", "naive"])
def test_every_sample_in_one_cell(path, monkeypatch):
    """(4100, 130): 533 000 adds on one counter of every map"""
    _clean(monkeypatch)
    monkeypatch.setenv("HTM_DENSITY_LDS", "1" if path == "lds" else "0")
    if path == "naive":
        monkeypatch.setenv("HTM_DENSITY_NAIVE", "1")
    n_mod, n_win = 4100, 130
    grid = GRIDS["3x2x5"]
    x = np.tile([-3.0 + 2.5 * 0.7, 10.0 + 0.5 * 1.3, 0.5 + 3.5 * 2.1], (n_mod, n_win))        # cell (2, 0, 3)
    got = dn.density(x, grid, volume=True)
    assert got["tally"].tolist() == [[n_mod * n_win, 0]]
    for nm, idx in (("xy", (0, 0, 2)), ("xz", (0, 3, 2)), ("yz", (0, 3, 0)), ("vol", (0, 3, 0, 2))):
        want = np.zeros_like(got[nm])
        want[idx] = n_mod * n_win
        assert np.array_equal(got[nm], want), nm


@pytest.mark.parametrize("lds", ["0", "1"])
def test_edge_points_where_the_kernels_index(lds, monkeypatch):
    """the edge, NaN and +-inf points of tests/test_density.py in the first row, the last row, lane 0, lane 63 and the last
    window of (67, 130), the rest of the samples inside"""
    _clean(monkeypatch)
    monkeypatch.setenv("HTM_DENSITY_LDS", lds)
    pts, inside, _ = dr.edge_samples()
    n_mod, n_win, n_pts = 67, 130, len(pts)
    assert n_mod >= n_pts
    g = np.array(dr.EDGE_GRID).reshape(3, 3)
    rng = np.random.default_rng(3)
    x = (g[:, 0] + rng.uniform(0.05, 0.95, size=(n_mod, n_win, 3)) * g[:, 2] * g[:, 1])
    for w in range(n_win):
        x[0, w], x[-1, w] = pts[w % n_pts], pts[(w + 17) % n_pts]
    for w in (0, 63, n_win - 1):
        x[1:1 + n_pts - 1, w] = pts[1:]
    x = x.reshape(n_mod, 3 * n_win)
    ref = dr.density(x, dr.EDGE_GRID)
    assert int(ref["tally"][0, 1]) > 2 * n_win // 3
    _equal(dn.density(x, dr.EDGE_GRID, volume=True), ref)
    # -0.0 at an origin of 0.0 is in cell 0, the smallest negative number outside
    z = np.array([[-0.0, -0.0, -0.0, 0.0, -0.0, 0.0], [-5e-324, 0.0, 0.0, 1.0, -0.0, 1.5]])
    got = dn.density(z, dr.ZERO_GRID, volume=True)
    _equal(got, dr.density(z, dr.ZERO_GRID))
    assert got["tally"].tolist() == [[3, 1]] and got["vol"][0, 0, 0, 0] == 2 and got["vol"][0, 1, 0, 1] == 1


def test_dev_form_with_a_row_stride_zeroes_its_outputs():
    """device pointers, ld = 3 n_win + 5 with NaN beyond the columns (never read), on a stream of its own, the outputs full of
    garbage before the call; a second call gives the same bits"""
    import torch

    n_mod, n_win = 1001, 43
    x, grid = _samples(n_mod, n_win, "3x2x5"), np.array(GRIDS["3x2x5"])
    lay, n_layer = _layers(n_win)
    ref = _reference(n_mod, n_win, "3x2x5", True)
    d_x = torch.full((n_mod, 3 * n_win + 5), float("nan"), dtype=torch.float64, device="cuda")
    d_x[:, :3 * n_win] = torch.from_numpy(np.array(x)).cuda()
    d_l = torch.from_numpy(lay).cuda()
    garbage = lambda shape: torch.full(shape, 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    lib = dn._lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for _ in range(2):
        outs = {nm: garbage(ref[nm].shape) for nm in ("xy", "xz", "yz", "vol", "tally")}
        st.wait_stream(torch.cuda.current_stream())
        dn._lib.check(lib.htm_hypo_density_dev(0, p(d_x), 3 * n_win + 5, n_mod, n_win, p(d_l), n_layer, dn._lib.ptr(grid), p(outs["xy"]), p(outs["xz"]),
                                               p(outs["yz"]), p(outs["vol"]), p(outs["tally"]), C.c_void_p(st.cuda_stream)))
        st.synchronize()
        results.append({nm: t.cpu().numpy().view(np.uint64) for nm, t in outs.items()})
    _equal(results[0], ref, "dev form")
    _equal(results[1], results[0], "second call")


# ---- end to end: the files of a small step-5 run -------------------------------------------------------------------
def test_program_writes_the_density_files(tmp_path, monkeypatch, capsys):
    """hypo/vs/qs.RR.out of two ranks in the record format [int32 iteration][float64 values], selected_win.dat, the parameter
    and station files; `density.main` with three time bins, --removed, --volume and row batches of 31 rows (four of them): the
    files are what the restatement and the host helpers give for the samples read back"""
    _, data, params = load_case("fixedcorr")
    params = dict(params, n_procs="2")
    n_ev, n_rows = data.n_events, 60
    # windows 0 and 1 (ids 10, 11) share a posterior: 11 is a double count; the others are apart.  Some samples leave the box.
    win_id = [10, 11, 12, 20, 21, 30, 40][:n_ev] + list(range(50, 50 + max(0, n_ev - 7)))
    param_file, _ = write_run_dir(tmp_path, data, params, win_id)
    from hypotremormcmc_amd.param import Param

    par = Param(param_file)
    wxy, z0, wz = par.get_prior_width_xy(), par.get_prior_z(), par.get_prior_width_z()
    cell = [wxy / 2.0, wxy / 3.0, wz]
    bounds = [par.sta_x.min() - wxy, par.sta_x.max() + wxy, par.sta_y.min() - wxy, par.sta_y.max() + wxy, z0, z0 + 5.0 * wz]
    grid = [v for a in range(3) for v in (bounds[2 * a], cell[a], float(int(np.ceil((bounds[2 * a + 1] - bounds[2 * a]) / cell[a] - 1e-9))))]
    assert grid[8] == 5.0
    rng = np.random.default_rng(8)
    mid = np.array([0.5 * (bounds[0] + bounds[1]), 0.5 * (bounds[2] + bounds[3]), z0 + 2.5 * wz])
    centre = mid + rng.uniform(-1.0, 1.0, size=(n_ev, 3)) * [wxy, wxy, wz]
    centre[1] = centre[0]
    centre[-1, 2] = z0 + 0.2 * wz                     # near the top of the box in depth: a share of it outside
    for r in range(2):
        hyp = (centre[None] + rng.normal(size=(n_rows, n_ev, 3)) * [0.4 * wxy, 0.4 * wxy, 0.4 * wz]).reshape(n_rows, 3 * n_ev)
        write_fake_samples(tmp_path, r, 10 * np.arange(1, n_rows + 1), {"hypo": hyp, "vs": rng.normal(size=(n_rows, 1)), "qs": rng.normal(size=(n_rows, 1))})
    _clean(monkeypatch)
    monkeypatch.delenv("HTM_SAMPLE_ENDIAN", raising=False)
    monkeypatch.setenv("HTM_DENSITY_MB", "%.6f" % (31.5 * 3 * n_ev * 8 / 1048576.0))
    dn.main([param_file, "--cell", *["%r" % c for c in cell], "--time-bins", "3", "--removed", "--volume", "--level", "0.5", "0.9"])
    # what is expected, from the files
    read = lambda r: np.fromfile(str(tmp_path / ("hypo.%02d.out" % r)), dtype=np.dtype([("it", "<i4"), ("v", "<f8", (3 * n_ev,))]))["v"]
    hypo = np.vstack([read(0), read(1)]).reshape(2 * n_rows, 3 * n_ev)
    keep = dn.kept_windows(win_id, hypo)
    assert 1 not in keep and 0 in keep and len(keep) >= n_ev - 2
    layer = dn.removed_layer(dn.time_layers(win_id, 3), keep)
    assert set(layer.tolist()) >= {-1, 0, 1, 2}
    ref = dr.density(hypo, grid, layer, 3)
    assert 0 < int(ref["tally"][:, 1].sum()) < int(ref["tally"][:, 0].sum())
    for nm in ("xy", "xz", "yz", "vol"):
        got = (tmp_path / ("tremor_density.%s.dat" % nm)).read_text()
        assert got == dn.map_text(nm, ref[nm], grid, 2 * n_rows, [0.5, 0.9]), nm
        assert len(got.split("\n")) == ref[nm].size + 2
    assert capsys.readouterr().out == dn.summary_text(ref["tally"])
