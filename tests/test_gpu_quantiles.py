"""GPU: the exact radix select of step 6 (k_select, k_select_pass in hypotremormcmc_amd/csrc/htm_select.hpp, behind
htm_quantiles and htm_quantiles_dev) against tests/quantile_restatement.select at the shapes, ranks and values its callers
use and the suite did not: fewer rows than row-group waves, rows around the 32-row unrolled body, 1 and 64 columns, rank 1,
rank n_mod, repeated and descending ranks, +-0, +-inf, denormals, +-DBL_MAX, NaN of either sign, columns whose candidates
survive to the last radix digits, one-row slabs, more slabs than rows, the clamp at 65 535 slabs, the library's own switch
between its two kernels, a column window of a wider matrix and two calls queued on one stream.

The select is exact, so there is no tolerance anywhere: every comparison is on the uint64 views of the doubles (NaN != NaN
and -0.0 == +0.0 as values).  The order is the restatement's total order,
-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, NaNs among themselves by payload."""
import ctypes as C
import functools

import numpy as np
import pytest

from hypotremormcmc_amd import _lib, statistics as st
from tests import quantile_restatement as qr

pytestmark = pytest.mark.gpu

ENV = "HTM_SELECT_SLABS"      # unset: the library chooses between k_select and the slab path; n: the slab path with n slabs


def _path(monkeypatch, slabs):
    if slabs is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, slabs)


def _quantiles(x, ranks):
    """htm_quantiles (host form) with explicit ranks: statistics.quantiles can only pass ranks(n)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n_mod, n_par = x.shape
    out = np.full((n_par, 3), -7.0)
    _lib.check(_lib.load().htm_quantiles(0, _lib.ptr(x), n_mod, n_par, (C.c_int * 3)(*ranks), _lib.ptr(out)))
    return out


def _same_bits(got, ref, what, names=None):
    g, r = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(ref).view(np.uint64)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        first = ["column %d%s, position %d: got %016x, expected %016x"
                 % (p, " (%s)" % names[p] if names else "", j, g[p, j], r[p, j]) for p, j in bad[:6]]
        raise AssertionError("%s: %d of %d elements differ; %s" % (what, len(bad), g.size, "; ".join(first)))


def _triples(n):
    return ((1, (n + 1) // 2, n), (n, 1, n), (n // 3 + 1,) * 3)      # ascending with both ends; descending, repeated; one interior rank


# ---- a. shapes and ranks, both kernel forms --------------------------------------------------------------------------------
N_MOD = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257)
N_PAR = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def _shape_case(n_mod, n_par):
    """x [n_mod][n_par] (read-only) and the restatement's answer for every triple of the shape, computed once for all paths"""
    rng = np.random.default_rng([n_mod, n_par])
    x = rng.normal(size=(n_mod, n_par)) * rng.choice([1e-3, 1.0, 1e6], size=n_par)
    x[:, 0] = np.round(3.0 * rng.normal(size=n_mod))        # many duplicates, -0.0 and +0.0 among them
    if n_par > 2:
        x[:, 1] = -np.abs(x[:, 1])                          # all negative
        x[:, 2] = x[0, 2]                                   # constant
    x.flags.writeable = False
    return x, {t: qr.select(x, t) for t in _triples(n_mod)}


@pytest.mark.parametrize("slabs", [None, "1", "2", "3", "7", "64"])
def test_select_at_edge_shapes_and_ranks(slabs, monkeypatch):
    """None: k_select, one launch.  "1": the slab path with one slab; "2", "3", "7": slabs whose row count is no multiple of
    the four row groups, ragged and empty last slabs; "64": one-row slabs, and more slabs asked for than there are rows
    (clamped to n_mod).  n_mod below 4 leaves row-group waves without a row; 31 .. 33 and 63 .. 65 lie around one and two
    32-row unrolled bodies; n_par 64 fills a column group exactly, 65 and 129 put one column into the last."""
    _path(monkeypatch, slabs)
    for n_mod in N_MOD:
        for n_par in N_PAR:
            x, refs = _shape_case(n_mod, n_par)
            for t, ref in refs.items():
                _same_bits(_quantiles(x, t), ref, "n_mod %d, n_par %d, ranks %s, slabs %s" % (n_mod, n_par, t, slabs))


# ---- b. every rank ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slabs", [None, "3"])
def test_select_every_rank_in_every_position(slabs, monkeypatch):
    """40 x 65: each of the three rank arguments takes every rank 1 .. 40 once (r, 41 - r, and 7 r mod 40 + 1, a permutation
    since 7 and 40 are coprime), ascending, descending and scattered triples among them"""
    _path(monkeypatch, slabs)
    n = 40
    triples = [(r, n + 1 - r, (7 * r) % n + 1) for r in range(1, n + 1)]
    for pos in range(3):
        assert sorted(t[pos] for t in triples) == list(range(1, n + 1))
    x, _ = _shape_case(n, 65)
    full = qr.select(x, range(1, n + 1))                    # [65][40]: the sorted columns
    for t in triples:
        _same_bits(_quantiles(x, t), full[:, [r - 1 for r in t]], "ranks %s, slabs %s" % (t, slabs))


# ---- c. special values -----------------------------------------------------------------------------------------------------
DBL_MAX = np.finfo(np.float64).max
NANS = np.array([0x7FF8000000000000, 0x7FF8000000000123, 0xFFF8000000000000, 0xFFF8000000000123], dtype=np.uint64).view(np.float64)


@functools.lru_cache(maxsize=None)
def _special_case(n_mod, n_par=65):
    """x [n_mod][n_par] (read-only), one column per pattern, every column in a row order of its own; the patterns' names"""
    rng = np.random.default_rng([7, n_mod])
    u64 = lambda a: np.asarray(a, dtype=np.uint64)
    i = np.arange(n_mod)
    cols, names = [], []

    def add(name, v):
        v = np.asarray(v, dtype=np.float64)
        assert v.shape == (n_mod,), name
        names.append(name)
        cols.append(v)

    add("+-0.0 mixed", np.where(rng.random(n_mod) < 0.5, -0.0, 0.0))
    v = rng.normal(size=n_mod)
    v[i % 5 == 0], v[i % 7 == 1] = np.inf, -np.inf
    add("finite with +-inf", v)
    add("all +inf", np.full(n_mod, np.inf))
    add("all -inf", np.full(n_mod, -np.inf))
    b = rng.integers(1, 1 << 52, size=n_mod, dtype=np.uint64) | (rng.integers(0, 2, size=n_mod, dtype=np.uint64) << np.uint64(63))
    b[:4] = u64([1, 1 | 1 << 63, (1 << 52) - 1, (1 << 52) - 1 | 1 << 63])          # +-5e-324, +- the largest denormal
    add("+-denormals", b.view(np.float64))
    v = np.where(rng.random(n_mod) < 0.5, -DBL_MAX, DBL_MAX)
    v[i % 9 == 2] = rng.normal(size=n_mod)[i % 9 == 2]
    add("+-DBL_MAX", v)
    v = rng.normal(size=n_mod)
    v[i % 3 == 0] = NANS[(i[i % 3 == 0] // 3) % 4]
    add("finite with NaN of both signs and two payloads", v)
    add("all NaN", NANS[rng.integers(0, 4, size=n_mod)])
    add("half tiny negative, half tiny positive", np.where(i % 2 == 0, -1.0, 1.0) * 1e-300 * (1.0 + rng.random(n_mod)))
    for base in (1.0, -1.0, 2.0 ** -1022, 0.0):            # consecutive doubles: the candidates share their top 13 hex digits
        add("ladder from %r" % base, (np.array([base]).view(np.uint64)[0] + u64(i)).view(np.float64))
    k0 = u64(rng.integers(0, 1 << 63, dtype=np.uint64)) | np.uint64(1 << 63)
    for d in range(16):                                    # keys equal except in hex digit d, which takes all 16 values
        k = (k0 & ~np.uint64(15 << 4 * d)) | (u64(i % 16) << np.uint64(4 * d))
        add("keys that differ in hex digit %d alone" % d, qr.unkey(k))
    while len(cols) < n_par:                                # any bit pattern at all: every kind of double, signalling NaN included
        add("random bit patterns", rng.integers(0, 1 << 64, size=n_mod, dtype=np.uint64).view(np.float64))
    assert len(cols) == n_par
    x = np.stack([c[rng.permutation(n_mod)] for c in cols], axis=1)
    # the copies above moved bits, not values: the patterns are still there
    xb = x.view(np.uint64)
    assert sorted(set(xb[:, 7].tolist())) == sorted(NANS.view(np.uint64).tolist()) and np.isnan(x[:, 6]).sum() == (i % 3 == 0).sum()
    assert np.array_equal(np.sort(xb[:, 12]), u64(i)) and {1, 1 | 1 << 63} <= set(xb[:, 4].tolist())
    for d in range(16):
        kd = qr.key(x[:, 13 + d])
        assert ((kd ^ kd[0]) & ~np.uint64(15 << 4 * d) == 0).all() and len(set(((kd >> np.uint64(4 * d)) & np.uint64(15)).tolist())) == min(16, n_mod)
    x.flags.writeable = False
    return x, names


@pytest.mark.parametrize("slabs", [None, "1", "7"])
def test_select_special_values(slabs, monkeypatch):
    """the total order on everything a double can hold, and columns that stay undecided until a late digit"""
    _path(monkeypatch, slabs)
    for n_mod in (257, 40):
        x, names = _special_case(n_mod)
        for t in ((1, (n_mod + 1) // 2, n_mod), st.ranks(n_mod)):
            _same_bits(_quantiles(x, t), qr.select(x, t), "n_mod %d, ranks %s, slabs %s" % (n_mod, t, slabs), names)


def test_python_layer_passes_nan_through_and_takes_a_vector(monkeypatch):
    """statistics.quantiles: NaN and inf are ordered, not refused; a 1-D input is one column"""
    _path(monkeypatch, None)
    x, names = _special_case(40)
    _same_bits(st.quantiles(x), qr.select(x, st.ranks(40)), "statistics.quantiles", names)
    got = st.quantiles(x[:, 6])
    assert got.shape == (1, 3)
    _same_bits(got, qr.select(x[:, 6], st.ranks(40)), "statistics.quantiles of a vector")


# ---- d. the path switches the library makes itself -------------------------------------------------------------------------
@pytest.mark.parametrize("n_mod, n_par, slabs, ranks", [
    (65535, 64, None, (1, 32768, 65535)),       # 2^22 - 64 elements: k_select, one launch
    (65536, 64, None, (65536, 1639, 1)),        # 2^22 exactly: 256 slabs of 256 rows
    (8193, 513, None, (205, 4097, 8193)),       # 9 column groups, 33 slabs of 249 rows, the last of 225
    (40, 131137, None, (1, 20, 40)),            # 2 050 column groups: 2048 / grid.x = 0, back to one slab and k_select
    (70000, 1, "100000", (35000, 70000, 1)),    # clamped to 65 535 slabs of 2 rows, those from 35 000 on empty
])
def test_select_where_the_library_switches_paths(n_mod, n_par, slabs, ranks, monkeypatch):
    _path(monkeypatch, slabs)
    rng = np.random.default_rng([11, n_mod, n_par])
    x = rng.normal(size=(n_mod, n_par))
    x[:, 0] = np.round(3.0 * x[:, 0])           # many duplicates
    _same_bits(_quantiles(x, ranks), qr.select(x, ranks), "n_mod %d, n_par %d, ranks %s" % (n_mod, n_par, ranks))


# ---- e. the _dev form as its callers use it --------------------------------------------------------------------------------
def test_dev_form_on_a_column_window_two_calls_on_one_stream(monkeypatch):
    """As htm_diagnose_rank_dev and htm_hypo_ellipsoid_dev call it: a window of 65 columns that starts at column 37 of a
    300 x 200 matrix (ld = 200, NaN everywhere outside the window: a read outside would win or lose every comparison), a
    stream other than the null stream, the slab workspace taken and released on it, two calls queued back to back with
    htm_diagnose_rank_dev's non-monotone triples and one synchronisation.  Then the same over the first 3 rows, where those
    triples repeat ranks and reach R.  The outputs lie inside larger prefilled buffers that must keep their bits."""
    import torch

    monkeypatch.setenv(ENV, "3")
    lib = _lib.load()
    n_rows, n_cols, c0, n_par, pad = 300, 200, 37, 65, 32
    rng = np.random.default_rng(13)
    win = rng.normal(size=(n_rows, n_par))
    win[:, 0] = np.round(3.0 * win[:, 0])
    win[:, n_par - 1] = -np.abs(win[:, n_par - 1])
    full = np.full((n_rows, n_cols), np.nan)
    full[:, c0:c0 + n_par] = win
    d_x = torch.from_numpy(full).cuda()
    fill = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
    stream = torch.cuda.Stream()
    for R in (n_rows, 3):
        k05, k95 = int(np.floor((R - 1) * 0.05)), int(np.floor((R - 1) * 0.95))
        ra = ((R + 1) // 2, R // 2 + 1, k05 + 1)
        rb = (min(k05 + 2, R), k95 + 1, min(k95 + 2, R))
        assert (ra, rb) == {300: ((150, 151, 15), (16, 285, 286)), 3: ((2, 2, 1), (2, 2, 3))}[R]
        d_out = [torch.from_numpy(np.full(pad + 3 * n_par + pad, fill)).cuda() for _ in range(2)]
        stream.wait_stream(torch.cuda.current_stream())
        for rk, d_o in zip((ra, rb), d_out):
            _lib.check(lib.htm_quantiles_dev(0, C.c_void_p(d_x.data_ptr() + 8 * c0), R, n_par, n_cols, (C.c_int * 3)(*rk),
                                             C.c_void_p(d_o.data_ptr() + 8 * pad), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        for rk, d_o in zip((ra, rb), d_out):
            got = d_o.cpu().numpy()
            edge = np.concatenate([got[:pad], got[pad + 3 * n_par:]]).view(np.uint64)
            assert (edge == fill.view(np.uint64)).all(), "R %d, ranks %s: written outside [n_par][3]" % (R, rk)
            _same_bits(got[pad:pad + 3 * n_par].reshape(n_par, 3), qr.select(win[:R], rk), "R %d, ranks %s" % (R, rk))
    assert np.array_equal(d_x.cpu().numpy().view(np.uint64), full.view(np.uint64))      # the samples are read only
