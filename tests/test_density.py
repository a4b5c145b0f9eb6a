"""CPU: the parts of the stacked density maps that need no device -- the numpy restatement of the binning
rule against np.histogramdd and at the edges, what htm_hypo_density[_dev] refuses before any device call, the host helpers
and the text layer of `python -m hypotremormcmc_amd.density`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hypotremormcmc_amd import density as dn
from tests import density_restatement as dr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GRID = (-3.0, 0.7, 9.0, 10.0, 1.3, 4.0, 0.5, 2.1, 6.0)


def _points(rng, n, grid, margin=1e-6):
    """n points, about a fifth outside the box, none nearer than `margin` of a cell to a cell edge"""
    g = np.array(grid).reshape(3, 3)
    q = rng.uniform(-0.1 * g[:, 2], 1.1 * g[:, 2], size=(n, 3))
    f = q - np.floor(q)
    q = np.floor(q) + np.clip(f, margin, 1.0 - margin)
    return g[:, 0] + q * g[:, 1]


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_restatement_equals_histogramdd_away_from_the_edges():
    rng = np.random.default_rng(11)
    n_mod, n_win = 400, 5
    x = _points(rng, n_mod * n_win, GRID).reshape(n_mod, 3 * n_win)
    ref = dr.density(x, GRID)
    g = np.array(GRID).reshape(3, 3)
    edges = [g[a, 0] + g[a, 1] * np.arange(int(g[a, 2]) + 1) for a in range(3)]
    pts = x.reshape(-1, 3)
    q = (pts - g[:, 0]) / g[:, 1]
    pts = pts[np.all((q >= 0) & (q < g[:, 2]), axis=1)]          # histogramdd's last cell is closed at the top: no point is near it
    h, _ = np.histogramdd(pts, bins=edges)                        # [nx][ny][nz]
    assert 0 < len(pts) < n_mod * n_win
    assert np.array_equal(ref["vol"][0], h.transpose(2, 1, 0).astype(np.uint64))
    assert np.array_equal(ref["xy"][0], h.sum(axis=2).T.astype(np.uint64))
    assert np.array_equal(ref["xz"][0], h.sum(axis=1).T.astype(np.uint64))
    assert np.array_equal(ref["yz"][0], h.sum(axis=0).T.astype(np.uint64))
    assert ref["tally"].tolist() == [[len(pts), n_mod * n_win - len(pts)]]


def check_invariant(res, n_mod, layer, n_layer, n_win):
    """every map of a layer sums to the layer's inside; inside + outside = n_mod x the layer's windows"""
    lay = np.zeros(n_win, dtype=int) if layer is None else np.asarray(layer)
    for L in range(n_layer):
        n_in, n_out = (int(v) for v in res["tally"][L])
        for nm in ("xy", "xz", "yz", "vol"):
            if res[nm] is not None:
                assert int(res[nm][L].sum(dtype=np.uint64)) == n_in, (nm, L)
        assert n_in + n_out == n_mod * int(np.sum(lay == L)), L


def test_invariant_of_every_layer():
    rng = np.random.default_rng(12)
    n_mod, n_win = 50, 11
    x = _points(rng, n_mod * n_win, GRID, margin=0.0).reshape(n_mod, 3 * n_win)
    x[3, 4] = np.nan
    layer = np.array([0, 1, 2, 0, 1, 2, -1, 3, 0, 0, 2])        # 3 = n_layer: takes no part, like -1
    ref = dr.density(x, GRID, layer, 3)
    check_invariant(ref, n_mod, layer, 3, n_win)
    assert int(ref["tally"].sum()) == n_mod * 9
    allw = dr.density(x, GRID)
    check_invariant(allw, n_mod, None, 1, n_win)
    assert int(allw["tally"][0, 1]) > 0 and dr.density(x, GRID, volume=False)["vol"] is None


def test_edges_are_half_open():
    pts, inside, cell = dr.edge_samples()
    assert inside.sum() > 20 and (~inside).sum() > 12
    for p, ok, c in zip(pts, inside, cell):
        ref = dr.density(p[None, :], dr.EDGE_GRID)
        assert ref["tally"].tolist() == [[int(ok), int(not ok)]], p
        if ok:
            assert ref["vol"][0, c[2], c[1], c[0]] == 1 and ref["xy"][0, c[1], c[0]] == 1, (p, c)
            assert ref["xz"][0, c[2], c[0]] == 1 and ref["yz"][0, c[2], c[1]] == 1, (p, c)
    # all at once, as one window per point
    ref = dr.density(pts.reshape(1, -1), dr.EDGE_GRID)
    assert ref["tally"].tolist() == [[int(inside.sum()), int((~inside).sum())]]
    want = np.zeros_like(ref["vol"])
    np.add.at(want[0], (cell[inside, 2], cell[inside, 1], cell[inside, 0]), np.uint64(1))
    assert np.array_equal(ref["vol"], want)
    # -0.0 at the origin 0.0: q = -0.0 >= 0, cell 0; the smallest negative number is outside
    z = dr.density(np.array([[-0.0, -0.0, -0.0, 0.0, -0.0, 0.0, -5e-324, 0.0, 0.0]]), dr.ZERO_GRID)
    assert z["tally"].tolist() == [[2, 1]] and z["vol"][0, 0, 0, 0] == 2


# ---- what the library refuses before any device call -----------------------------------------------------------------
_G9 = np.array(GRID)


def _dev_call(lib, hypo=1, ld=6, n_mod=10, n_win=2, layer=0, n_layer=1, grid=_G9, xy=1, xz=1, yz=1, vol=1, tally=1, device=-1):
    """htm_hypo_density_dev with stand-in addresses (1 = some address that is never followed, 0 = NULL); grid9 is read"""
    p = lambda a: C.c_void_p(4096 if a else None)
    g = None if grid is None else np.ascontiguousarray(grid, dtype=np.float64)
    return lib.htm_hypo_density_dev(device, p(hypo), ld, n_mod, n_win, p(layer), n_layer, None if g is None else g.ctypes.data_as(dn._lib.dp),
                                    p(xy), p(xz), p(yz), p(vol), p(tally), None)


def _grid(**kw):
    g = dict(zip(("x0", "dx", "nx", "y0", "dy", "ny", "z0", "dz", "nz"), GRID))
    g.update(kw)
    return np.array(list(g.values()), dtype=np.float64)


def _clean(monkeypatch):
    for k in ("HTM_DENSITY_LDS", "HTM_DENSITY_SLABS", "HTM_DENSITY_MB", "HTM_DENSITY_NAIVE"):
        monkeypatch.delenv(k, raising=False)


def _past_the_plan(msg):
    """device = -1 after every check: the device selection's refusal (with a GPU) or the missing device (without)"""
    return "out of range" in msg or "no HIP device" in msg


def test_arguments_are_checked_before_any_device_call(monkeypatch):
    """device = -1 would fail in hipSetDevice: each of these returns HTM_EINVAL with its own message first"""
    lib = dn._lib.load()
    last = lambda: lib.htm_last_error().decode()
    _clean(monkeypatch)
    for null in ("hypo", "xy", "xz", "yz", "tally"):
        assert _dev_call(lib, **{null: 0}) == -1 and last() == "NULL argument", null
    assert _dev_call(lib, grid=None) == -1 and last() == "NULL argument"
    assert _dev_call(lib, n_mod=0) == -1 and "need n_mod >= 1" in last()
    assert _dev_call(lib, n_win=0) == -1 and "n_win >= 1" in last()
    assert _dev_call(lib, layer=1, n_layer=0) == -1 and "n_layer >= 1" in last()
    assert _dev_call(lib, layer=0, n_layer=2) == -1 and "n_layer 2 without a layer per window" in last()
    assert _dev_call(lib, ld=5) == -1 and "ld 5 < 3 n_win = 6" in last()
    for bad in (dict(x0=np.nan), dict(y0=np.inf), dict(dz=0.0), dict(dx=-1.0), dict(dy=np.inf), dict(dz=np.nan)):
        assert _dev_call(lib, grid=_grid(**bad)) == -1 and "need a finite origin and a finite cell size > 0" in last(), bad
    assert "grid axis z" in last()
    for bad in (dict(nx=0.0), dict(ny=4097.0), dict(nz=2.5), dict(nx=-3.0), dict(ny=np.nan)):
        assert _dev_call(lib, grid=_grid(**bad)) == -1 and "need an integer in 1..4096" in last(), bad
    big = _grid(nx=4096.0, ny=4096.0, nz=4096.0)
    assert _dev_call(lib, grid=big) == -1 and "more than 2^31 - 1 counters" in last()
    assert _dev_call(lib, grid=_grid(nx=4096.0, ny=4096.0, nz=1.0), vol=0, layer=1, n_layer=200) == -1 and "200 layers" in last()
    assert _dev_call(lib, n_win=2 ** 31, ld=2 ** 33) == -1 and "2^32 - 1 work-items" in last()
    monkeypatch.setenv("HTM_DENSITY_SLABS", "65535")            # 4096 workgroups of windows x 65535 row slabs
    assert _dev_call(lib, n_win=2 ** 20, ld=2 ** 22, n_mod=10 ** 6) == -1 and "in 62500 row slabs needs more than 2^32 - 1 work-items" in last()   # 16 rows each: no empty slab
    _clean(monkeypatch)
    # the LDS path forced on a grid that it does not take: one cell too many on the x axis
    ny, nz = 8, 4
    nx = (dn.LDS_MAX_CELLS - ny * nz) // (ny + nz)
    monkeypatch.setenv("HTM_DENSITY_LDS", "1")
    assert _dev_call(lib, grid=_grid(nx=nx + 1.0, ny=float(ny), nz=float(nz))) == -1 and "HTM_DENSITY_LDS = 1, but" in last()
    assert _dev_call(lib, grid=_grid(nx=float(nx), ny=float(ny), nz=float(nz))) in (-1, -2) and _past_the_plan(last())
    monkeypatch.setenv("HTM_DENSITY_LDS", "yes")
    assert _dev_call(lib) == -1 and "HTM_DENSITY_LDS = yes: 0 or 1" in last()
    _clean(monkeypatch)
    # the host form: the same rules with ld = 3 n_win; vol and layer may be NULL
    x, lay = np.zeros((10, 6)), np.zeros(2, dtype=np.int32)
    bufs = [np.zeros(64, dtype=np.uint64) for _ in range(5)]
    u = lambda a: None if a is None else a.ctypes.data_as(dn._lib.u64p)

    def host(hypo=x, n_mod=10, n_win=2, layer=None, n_layer=1, grid=_grid(nx=2.0, ny=2.0, nz=2.0), outs=bufs, device=-1):
        return lib.htm_hypo_density(device, dn._lib.ptr(hypo), n_mod, n_win, None if layer is None else layer.ctypes.data_as(dn._lib.ip), n_layer,
                                    dn._lib.ptr(grid), *[u(a) for a in outs])

    assert host(hypo=None) == -1 and last() == "NULL argument"
    assert host(outs=bufs[:4] + [None]) == -1 and last() == "NULL argument"
    assert host(n_mod=0) == -1 and "need n_mod >= 1" in last()
    assert host(n_layer=3) == -1 and "without a layer per window" in last()
    assert host(layer=lay, n_layer=0) == -1 and "n_layer >= 1" in last()
    assert host(grid=_grid(dx=0.0)) == -1 and "grid axis x" in last()
    assert host(grid=_grid(nz=1.5)) == -1 and "need an integer in 1..4096" in last()
    assert host(grid=big) == -1 and "more than 2^31 - 1 counters" in last()
    monkeypatch.setenv("HTM_DENSITY_MB", "-1")
    assert host() == -1 and "HTM_DENSITY_MB = -1" in last()
    _clean(monkeypatch)
    assert host(outs=bufs[:3] + [None, bufs[4]]) in (-1, -2) and _past_the_plan(last())


def test_no_device_is_an_error_not_a_fallback(monkeypatch):
    lib = dn._lib.load()
    n = C.c_int(-1)
    if lib.htm_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present; the no-device behaviour is exercised on the CPU-only container")
    _clean(monkeypatch)
    assert _dev_call(lib, device=0) == -2 and "no HIP device" in lib.htm_last_error().decode()
    x = np.random.default_rng(0).normal(size=(10, 6))
    with pytest.raises(dn._lib.HtmError, match="no HIP device"):
        dn.density(x, _grid(nx=2.0, ny=2.0, nz=2.0))


def test_python_entry_checks_its_input():
    x = np.zeros((10, 6))
    g = _grid()
    for hypo, grid, kw in ((x[:, :5], g, {}), (x[:0], g, {}), (x, g[:8], {}), (x, _grid(dx=0.0), {}), (x, _grid(nx=2.5), {}), (x, _grid(nz=5000.0), {}),
                           (x, g, dict(n_layer=2)), (x, g, dict(layer=[0, 1, 0], n_layer=2)), (x, g, dict(n_layer=0)),
                           (x, _grid(nx=4096.0, ny=4096.0, nz=4096.0), dict(volume=True))):
        with pytest.raises(ValueError):
            dn.density(hypo, grid, **kw)


def test_module_mirrors_the_kernels_constants():
    src = open(os.path.join(ROOT, "hypotremormcmc_amd", "csrc", "htm_density.hpp")).read()
    assert int(re.search(r"constexpr int kDensLdsCells = (\d+);", src).group(1)) == dn.LDS_MAX_CELLS
    grid_src = open(os.path.join(ROOT, "hypotremormcmc_amd", "csrc", "htm_grid.hpp")).read()
    assert int(re.search(r"constexpr int kMapMaxCells = (\d+);", grid_src).group(1)) == dn.MAX_CELLS
    assert dn.lds_fits(_grid(nx=680.0, ny=8.0, nz=4.0)) and not dn.lds_fits(_grid(nx=681.0, ny=8.0, nz=4.0))


# ---- host helpers ----------------------------------------------------------------------------------------------------
def test_hpd_levels_with_ties():
    c = np.array([[10, 5, 5, 0], [3, 3, 3, 1]], dtype=np.uint64)           # 30 samples
    lev = dn.hpd_levels(c, [0.95, 0.3, 0.5, 0.68])
    # 10 reaches 0.3 (9); the two 5s enter together: 20 reaches 0.5 (15) but not 0.68 (20.4); the three 3s: 29 reaches 0.68 and
    # 0.95 (28.5); the 1 is in no region, nor is the empty cell
    assert lev.tolist() == [[0.3, 0.5, 0.5, 0.0], [0.68, 0.68, 0.68, 0.0]]
    assert dn.hpd_levels(c, [1.0]).tolist() == [[1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0]]
    assert dn.hpd_levels(c, [0.34]).tolist() == [[0.34, 0.34, 0.34, 0.0], [0.0] * 4]      # 10 < 10.2: the tied pair enters whole
    assert dn.hpd_levels(np.zeros((2, 2), dtype=np.uint64), [0.5]).tolist() == [[0.0, 0.0], [0.0, 0.0]]
    assert dn.hpd_levels(np.array([7], dtype=np.uint64), [0.5]).tolist() == [0.5]
    v = dn.hpd_levels(np.arange(24, dtype=np.uint64).reshape(2, 3, 4), [0.5, 0.9])         # a volume
    assert v.shape == (2, 3, 4) and v[1, 2, 3] == 0.5 and v[0, 0, 0] == 0.0
    for bad in ([0.0], [1.5], [float("nan")]):
        with pytest.raises(ValueError):
            dn.hpd_levels(c, bad)


def test_time_layers_and_removed_windows():
    assert dn.time_layers([10, 11, 12, 13, 14, 15], 3).tolist() == [0, 0, 1, 1, 2, 2]
    assert dn.time_layers([5, 100, 7, 52, 53], 2).tolist() == [0, 1, 0, 0, 1]              # [5, 52] and [53, 100]
    assert dn.time_layers([3, 4, 5], 1).tolist() == [0, 0, 0] and dn.time_layers([9], 4).tolist() == [0]
    assert dn.time_layers([1, 2, 3], 7).tolist() == [0, 2, 4]
    assert dn.time_layers([1, 2], 2).dtype == np.int32
    with pytest.raises(ValueError):
        dn.time_layers([1, 2], 0)
    with pytest.raises(ValueError):
        dn.time_layers([], 2)
    lay = dn.removed_layer([0, 0, 1, 1, 2], [0, 2, 4])
    assert lay.tolist() == [0, -1, 1, -1, 2] and lay.dtype == np.int32
    # a removed window is in nobody's tally
    x = np.full((4, 15), 1.0)
    ref = dr.density(x, (0.0, 2.0, 1.0, 0.0, 2.0, 1.0, 0.0, 2.0, 1.0), lay, 3)
    assert ref["tally"].tolist() == [[4, 0], [4, 0], [4, 0]]


# ---- the text layer --------------------------------------------------------------------------------------------------
def test_writers_on_hand_made_maps():
    grid = (10.0, 2.0, 2.0, -1.0, 0.5, 1.0, 3.0, 1.0, 2.0)
    xy = np.array([[[3, 1]], [[0, 0]]], dtype=np.uint64)                      # [2 layers][ny = 1][nx = 2]
    text = dn.map_text("xy", xy, grid, 4, [0.5, 0.9])
    assert text == (dn.HEADERS["xy"] + "\n"
                    "    0     0     0     11.000000     -0.750000           3      0.750000  0.5000\n"
                    "    0     1     0     13.000000     -0.750000           1      0.250000  0.9000\n"
                    "    1     0     0     11.000000     -0.750000           0      0.000000  0.0000\n"
                    "    1     1     0     13.000000     -0.750000           0      0.000000  0.0000\n")
    yz = np.array([[[2], [2]]], dtype=np.uint64)                              # [1][nz = 2][ny = 1]
    assert dn.map_text("yz", yz, grid, 8, [0.68]).split("\n")[1:] == [
        "    0     0     0     -0.750000      3.500000           2      0.250000  0.6800",
        "    0     0     1     -0.750000      4.500000           2      0.250000  0.6800", ""]
    vol = np.zeros((1, 2, 1, 2), dtype=np.uint64)
    vol[0, 1, 0, 1] = 5
    got = dn.map_text("vol", vol, grid, 5, [0.95]).split("\n")
    assert got[0] == dn.HEADERS["vol"] and got[0].startswith("# layer, cell ix iy iz, centre x y z, samples") and len(got) == 6
    assert got[4] == "    0     1     0     1     13.000000     -0.750000      4.500000           5      1.000000  0.9500"
    assert got[1] == "    0     0     0     0     11.000000     -0.750000      3.500000           0      0.000000  0.0000"
    assert dn.summary_text(np.array([[70, 30], [0, 0], [5, 0]], dtype=np.uint64)) == (
        "layer 0: 70 samples inside the box, 30 outside (30.00 %)\n"
        "layer 1: 0 samples inside the box, 0 outside (NaN)\n"
        "layer 2: 5 samples inside the box, 0 outside (0.00 %)\n")


def test_grid_from_bounds():
    g = dn.make_grid([0.0, 10.0, -5.0, 5.5, 2.0, 3.0], [0.5, 1.0, 4.0])
    assert g.tolist() == [0.0, 0.5, 20.0, -5.0, 1.0, 11.0, 2.0, 4.0, 1.0]
    with pytest.raises(ValueError):
        dn.make_grid([0.0, 0.0, 0.0, 1.0, 0.0, 1.0], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        dn.make_grid([0.0, 1e6, 0.0, 1.0, 0.0, 1.0], [0.1, 1.0, 1.0])         # more than 4096 cells
