"""CPU: what makes tests/quantile_restatement.py a reference -- its image of a double is invertible and orders the special
values as documented, its select is np.sort's on NaN-free columns and the compiled reference's step 6 on the golden sample
files -- and the calls both forms of htm_quantiles refuse before any device call."""
import ctypes as C

import numpy as np
import pytest

from tests import quantile_restatement as qr
from tests.helpers import load_case

# ascending in the documented order; as bit patterns, because NaN payloads and signs survive nothing else
SPECIAL_BITS = [
    0xFFFFFFFFFFFFFFFF,     # -NaN, largest payload
    0xFFF8000000000000,     # -NaN, the quiet default
    0xFFF0000000000001,     # -NaN, smallest payload
    0xFFF0000000000000,     # -inf
    0xFFEFFFFFFFFFFFFF,     # -DBL_MAX
    0xC000000000000000,     # -2.0
    0xBFF0000000000001,     # -(1 + 2^-52)
    0xBFF0000000000000,     # -1.0
    0x8010000000000000,     # -DBL_MIN = -2^-1022
    0x800FFFFFFFFFFFFF,     # the largest denormal, negative
    0x8000000000000001,     # -5e-324
    0x8000000000000000,     # -0.0
    0x0000000000000000,     # +0.0
    0x0000000000000001,     # 5e-324
    0x000FFFFFFFFFFFFF,     # the largest denormal
    0x0010000000000000,     # DBL_MIN
    0x3FF0000000000000,     # 1.0
    0x3FF0000000000001,     # 1 + 2^-52
    0x4000000000000000,     # 2.0
    0x7FEFFFFFFFFFFFFF,     # DBL_MAX
    0x7FF0000000000000,     # +inf
    0x7FF0000000000001,     # +NaN, smallest payload
    0x7FF8000000000000,     # +NaN, the quiet default
    0x7FFFFFFFFFFFFFFF,     # +NaN, largest payload
]


def _special():
    return np.array(SPECIAL_BITS, dtype=np.uint64).view(np.float64)


def test_special_list_is_what_its_comments_say():
    x = _special()
    assert np.isnan(x[:3]).all() and np.signbit(x[:3]).all() and np.isnan(x[-3:]).all() and not np.signbit(x[-3:]).any()
    assert x[3] == -np.inf and x[-4] == np.inf and x[4] == -np.finfo(np.float64).max and x[-5] == np.finfo(np.float64).max
    assert x[8] == -2.0 ** -1022 and x[10] == -5e-324 and x[13] == 5e-324 and x[15] == 2.0 ** -1022
    assert x[11] == 0.0 and np.signbit(x[11]) and x[12] == 0.0 and not np.signbit(x[12])
    assert np.array_equal(x[3:-3], np.sort(x[3:-3]))        # numpy's own order agrees wherever it has one


def test_unkey_inverts_key_bit_for_bit():
    x = _special()
    k = qr.key(x)
    assert k.dtype == np.uint64 and np.array_equal(qr.unkey(k).view(np.uint64), x.view(np.uint64))
    rng = np.random.default_rng(1)
    b = rng.integers(0, 2 ** 64, size=4096, dtype=np.uint64)           # every kind of double, NaN included
    assert np.array_equal(qr.key(qr.unkey(b)), b)
    assert np.array_equal(qr.unkey(qr.key(b.view(np.float64))).view(np.uint64), b)
    # the image stated once more in Python integers
    for v, kv in zip(SPECIAL_BITS, k.tolist()):
        assert kv == (v ^ 0xFFFFFFFFFFFFFFFF if v >> 63 else v | 1 << 63)


def test_key_orders_the_special_values_as_documented():
    k = qr.key(_special()).tolist()
    assert all(a < b for a, b in zip(k, k[1:])), [hex(v) for v in k]
    # and select returns them in that order whatever the row order
    x = _special()
    perm = np.random.default_rng(2).permutation(len(x))
    got = qr.select(x[perm], range(1, len(x) + 1))
    assert got.shape == (1, len(x)) and np.array_equal(got[0].view(np.uint64), x.view(np.uint64))


def test_select_is_np_sort_on_nan_free_columns():
    rng = np.random.default_rng(3)
    for n_mod, n_par in ((1, 1), (2, 3), (5, 4), (40, 7), (257, 65), (1000, 9)):
        x = rng.normal(size=(n_mod, n_par)) * rng.choice([1e-300, 1e-3, 1.0, 1e6, 1e300], size=n_par)
        x[:, 0] = np.round(x[:, 0])                 # duplicates; -0.0 and +0.0 mix here
        if n_par > 2:
            x[rng.integers(n_mod, size=n_mod // 3 + 1), 1] = np.inf
            x[rng.integers(n_mod, size=n_mod // 3 + 1), 2] = -np.inf
        r = sorted({1, n_mod, (n_mod + 1) // 2, n_mod // 2 + 1, min(n_mod, 7)})
        got, ref = qr.select(x, r), np.sort(x, axis=0)[[v - 1 for v in r]].T
        assert got.shape == ref.shape and np.array_equal(got, ref), (n_mod, n_par)          # by value
        zeros = (x == 0.0)
        mixed = (zeros & np.signbit(x)).any(axis=0) & (zeros & ~np.signbit(x)).any(axis=0)
        assert np.array_equal(got[~mixed].view(np.uint64), ref[~mixed].view(np.uint64)), (n_mod, n_par)    # by bits
    # the refinement itself: -0.0 orders before +0.0
    z = np.array([0.0, -0.0, 0.0, -0.0, -0.0])
    assert np.signbit(qr.select(z, (1, 2, 3, 4, 5))[0]).tolist() == [True, True, True, False, False]
    # ranks come back in the order asked for, repeats included; a 1-D input is one column
    assert qr.select(np.array([3.0, 1.0, 2.0]), (3, 1, 3)).tolist() == [[3.0, 1.0, 3.0]]
    for bad in ((0, 1, 1), (1, 4, 1)):
        with pytest.raises(ValueError):
            qr.select(np.zeros(3), bad)


@pytest.mark.parametrize("name", ["c1", "fixedcorr"])
def test_select_is_the_oracle_on_the_golden_samples(name):
    """oracle.stats_oracle.quantiles is pinned on the .stat files the compiled reference wrote from these records"""
    from oracle import stats_oracle as so

    fx, _, params = load_case(name)
    n_procs = int(params["n_procs"])
    for nm in ("vs", "qs", "t_corr", "a_corr", "hypo"):
        x = np.concatenate([fx[f"{nm}_{r}"] for r in range(n_procs)], axis=0)
        x = x.reshape(len(x), -1)
        assert len(x) == int(fx["stat_n_mod"]) and np.isfinite(x).all()
        got, ref = qr.select(x, so.ranks(len(x))), so.quantiles(x)
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), nm


# ---- refusals: before any device call (device -1: past the guards the call would fail in the device selection) -------------
def test_both_forms_refuse_bad_ranks_and_shapes_before_any_device_call():
    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    buf, out = np.zeros(64), np.full(64, -7.0)
    hp, ho = _lib.ptr(buf), _lib.ptr(out)
    dp, do = C.c_void_p(buf.ctypes.data), C.c_void_p(out.ctypes.data)
    rk = lambda *r: (C.c_int * 3)(*r)
    calls = {
        "rank 0, host": (lambda: lib.htm_quantiles(-1, hp, 8, 2, rk(0, 4, 8), ho), "rank 0 outside 1..8"),
        "rank 0 last, host": (lambda: lib.htm_quantiles(-1, hp, 8, 2, rk(1, 4, 0), ho), "rank 0 outside 1..8"),
        "rank n_mod + 1, host": (lambda: lib.htm_quantiles(-1, hp, 8, 2, rk(1, 9, 8), ho), "rank 9 outside 1..8"),
        "negative rank, host": (lambda: lib.htm_quantiles(-1, hp, 8, 2, rk(1, 4, -1), ho), "rank -1 outside 1..8"),
        "n_mod 0, host": (lambda: lib.htm_quantiles(-1, hp, 0, 2, rk(1, 1, 1), ho), "bad shape"),
        "n_par 0, host": (lambda: lib.htm_quantiles(-1, hp, 8, 0, rk(1, 4, 8), ho), "bad shape"),
        "NULL ranks, host": (lambda: lib.htm_quantiles(-1, hp, 8, 2, None, ho), "NULL argument"),
        "rank 0, dev": (lambda: lib.htm_quantiles_dev(-1, dp, 8, 2, 2, rk(0, 4, 8), do, None), "rank 0 outside 1..8"),
        "rank n_mod + 1, dev": (lambda: lib.htm_quantiles_dev(-1, dp, 8, 2, 2, rk(8, 1, 9), do, None), "rank 9 outside 1..8"),
        "ld < n_par, dev": (lambda: lib.htm_quantiles_dev(-1, dp, 8, 2, 1, rk(1, 4, 8), do, None), "bad shape (n_mod 8, n_par 2, ld 1)"),
        "n_mod 0, dev": (lambda: lib.htm_quantiles_dev(-1, dp, 0, 2, 2, rk(1, 1, 1), do, None), "bad shape"),
        "n_par 0, dev": (lambda: lib.htm_quantiles_dev(-1, dp, 8, 0, 2, rk(1, 4, 8), do, None), "bad shape"),
        "NULL ranks, dev": (lambda: lib.htm_quantiles_dev(-1, dp, 8, 2, 2, None, do, None), "NULL argument"),
    }
    for name, (call, msg) in calls.items():
        assert call() == -1, name                   # HTM_EINVAL
        assert msg in lib.htm_last_error().decode(), (name, lib.htm_last_error())
    # the same shapes with valid ranks pass the guards and stop at device -1: the guards refused nothing else
    assert lib.htm_quantiles(-1, hp, 8, 2, rk(8, 1, 8), ho) != 0
    last = lib.htm_last_error().decode().lower()
    assert "device" in last and "rank" not in last and "shape" not in last
    assert lib.htm_quantiles_dev(-1, dp, 8, 2, 3, rk(4, 4, 4), do, None) != 0
    assert "device" in lib.htm_last_error().decode().lower()
    assert (out == -7.0).all()


def test_python_layer_refuses_ranks_beyond_the_rows():
    """ranks(n_mod) of more models than rows, and of fewer than 40 (il = 0): the library's refusal, raised"""
    from hypotremormcmc_amd import _lib, statistics

    with pytest.raises(_lib.HtmError, match=r"rank 500 outside 1\.\.10|rank 975 outside 1\.\.10|rank 25 outside 1\.\.10"):
        statistics.quantiles(np.zeros((10, 2)), n_mod=1000, device=-1)
    with pytest.raises(_lib.HtmError, match=r"rank 0 outside 1\.\.39"):
        statistics.quantiles(np.zeros((39, 2)), device=-1)
    x, n = statistics.sample_matrix(np.arange(5.0), "htm_quantiles selects over", n_seq=None, finite=False)
    assert x.shape == (5, 1) and n == 5             # a 1-D input is one column
