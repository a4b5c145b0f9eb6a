"""CPU: the parts of the location error ellipsoids that need no device -- the numpy restatement against
np.cov / eigh and on a cloud of known axes, the chi-square quantiles, the rank rule, what htm_hypo_ellipsoid[_dev] refuses
before any device call, and the text layer of `python -m hypotremormcmc_amd.ellipsoid`."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import ellipsoid_restatement as er


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_restatement_equals_numpy_cov_and_eigh():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(50, 6)) @ np.kron(np.eye(2), rng.normal(size=(3, 3))) + rng.normal(size=6)
    piv = (x[:, 2] + rng.normal(size=50))[:, None]
    ref = er.ellipsoid(x, piv, rank=34, want_d2=True)
    for w in range(2):
        xs = x[:, 3 * w:3 * w + 3]
        cov = np.cov(xs, rowvar=False)
        assert np.allclose(ref["mean"][w], xs.mean(axis=0), rtol=0, atol=1e-14)
        assert np.allclose(ref["cov"][w], cov, rtol=1e-13, atol=0)
        lam = np.linalg.eigvalsh(cov)[::-1]
        assert np.allclose(ref["lam"][w], lam, rtol=1e-12)
        V = ref["axes"][w]
        assert np.allclose(V @ np.diag(ref["lam"][w]) @ V.T, cov, rtol=0, atol=1e-13 * lam[0])
        assert np.allclose(V.T @ V, np.eye(3), atol=1e-14)
        assert all(V[np.argmax(np.abs(V[:, k])), k] > 0 for k in range(3))
        d = xs - xs.mean(axis=0)
        d2 = np.einsum("ia,ab,ib->i", d, np.linalg.inv(cov), d)
        assert np.allclose(ref["d2"][:, w], d2, rtol=1e-10)
        assert ref["q"][w] == np.sort(ref["d2"][:, w])[33]
        assert np.sum(ref["d2"][:, w] <= ref["q"][w]) == 34
        assert np.allclose(ref["piv_corr"][w, :, 0], [np.corrcoef(xs[:, a], piv[:, 0])[0, 1] for a in range(3)], atol=1e-13)
    assert np.isclose(np.mean(ref["d2"]), 3.0 * 49 / 50)          # the mean of d2 is 3 (n - 1) / n whatever the cloud


def test_restatement_gives_back_the_axes_of_a_rotated_gaussian_cloud():
    rng = np.random.default_rng(6)
    th, ph = 0.7, 0.4
    R = (np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]])
         @ np.array([[1, 0, 0], [0, math.cos(ph), -math.sin(ph)], [0, math.sin(ph), math.cos(ph)]]))
    sig = np.array([10.0, 2.0, 0.5])
    n = 200000
    x = (rng.normal(size=(n, 3)) * sig) @ R.T + [3.0, -2.0, 30.0]
    ref = er.ellipsoid(x, rank=math.ceil(0.68 * n))
    assert np.allclose(np.sqrt(ref["lam"][0]), sig, rtol=0.01)
    assert np.all(np.abs(np.abs(np.sum(ref["axes"][0] * R, axis=0)) - 1) < 1e-3)       # |v_k . r_k| = 1
    assert abs(ref["q"][0] / 3.5058823558 - 1) < 0.01              # a Gaussian cloud: q is the chi-square quantile


def test_restatement_marks_degenerate_windows():
    rng = np.random.default_rng(7)
    x = rng.normal(size=(30, 6))
    x[:, 5] = 1.25
    piv = np.stack([rng.normal(size=30), np.full(30, 4.0)], axis=1)
    ref = er.ellipsoid(x, piv, rank=10)
    assert np.all(np.isnan(ref["lam"][1])) and np.all(np.isnan(ref["axes"][1])) and np.isnan(ref["q"][1])
    assert np.all(ref["cov"][1][2] == 0) and np.all(ref["cov"][1][:, 2] == 0) and ref["mean"][1][2] == 1.25
    assert np.all(np.isfinite(ref["lam"][0])) and np.isfinite(ref["q"][0])
    assert np.all(np.isnan(ref["piv_corr"][:, :, 1])) and np.all(np.isnan(ref["piv_corr"][1, 2]))
    assert np.all(np.isfinite(ref["piv_corr"][0, :, 0])) and np.all(np.isfinite(ref["piv_corr"][1, :2, 0]))


# ---- chi-square quantiles and the rank rule --------------------------------------------------------------------------
def test_chi2_quantile():
    from hypotremormcmc_amd.ellipsoid import chi2_quantile

    for lv in (0.1, 0.5, 0.68, 0.95):
        assert chi2_quantile(lv, 2) == pytest.approx(-2.0 * math.log(1.0 - lv), rel=1e-14)
    assert abs(chi2_quantile(0.68, 3) - 3.5058823558) < 1e-9
    assert abs(chi2_quantile(0.95, 3) - 7.8147) < 1e-4
    for dof in (2, 3):
        v = [chi2_quantile(lv, dof) for lv in np.linspace(0.0, 0.999, 101)]
        assert v[0] == 0.0 and np.all(np.diff(v) > 0)
    with pytest.raises(ValueError):
        chi2_quantile(0.5, 4)
    with pytest.raises(ValueError):
        chi2_quantile(1.0, 3)


def test_rank_rule_at_the_edges():
    from hypotremormcmc_amd.ellipsoid import level_rank

    assert level_rank(1e-300, 1000) == 1             # level -> 0: the nearest sample
    assert level_rank(1.0, 1000) == 1000             # level = 1: the farthest
    assert level_rank(0.5, 1000) == 500              # level * n_mod integral: that sample, not the next
    assert level_rank(0.25, 4) == 1 and level_rank(0.26, 4) == 2
    assert level_rank(0.68, 7) == 5 and level_rank(0.75, 80000) == 60000
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            level_rank(bad, 10)


# ---- what the library refuses before any device call -----------------------------------------------------------------
def _dev_call(lib, hypo=1, ld=6, piv=1, ld_piv=2, n_mod=10, n_win=2, n_piv=2, rank=5, out=1, corr=1, device=-1):
    """htm_hypo_ellipsoid_dev with stand-in addresses (1 = some address that is never followed, 0 = NULL)"""
    p = lambda a: C.c_void_p(4096 if a else None)
    return lib.htm_hypo_ellipsoid_dev(device, p(hypo), ld, p(piv), ld_piv, n_mod, n_win, n_piv, rank, p(out), p(corr), None)


def test_arguments_are_checked_before_any_device_call(monkeypatch):
    """device = -1 would fail in hipSetDevice: each of these returns HTM_EINVAL with its own message first"""
    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    last = lambda: lib.htm_last_error().decode()
    monkeypatch.delenv("HTM_ELLIPSOID_MB", raising=False)
    monkeypatch.delenv("HTM_ELL_SLABS", raising=False)
    assert _dev_call(lib, n_mod=3, rank=1) == -1 and "need n_mod >= 4" in last()
    assert _dev_call(lib, n_piv=5, ld_piv=5) == -1 and "0 <= n_piv <= 4" in last()
    assert _dev_call(lib, n_win=0) == -1 and "n_win >= 1" in last()
    assert _dev_call(lib, rank=0) == -1 and "rank 0 outside 1..10" in last()
    assert _dev_call(lib, rank=11) == -1 and "rank 11 outside 1..10" in last()
    assert _dev_call(lib, ld=5) == -1 and "ld 5 < 3 n_win = 6" in last()
    assert _dev_call(lib, ld_piv=1) == -1 and "ld_piv 1 < n_piv = 2" in last()
    for null in ("hypo", "out", "piv", "corr"):
        assert _dev_call(lib, **{null: 0}) == -1 and last() == "NULL argument", null
    assert _dev_call(lib, n_mod=2 ** 31, rank=1) == -1 and "exceeds 2147483647 rows" in last()
    assert _dev_call(lib, n_win=2 ** 31, ld=2 ** 33) == -1 and "2^32 - 1 work-items" in last()
    monkeypatch.setenv("HTM_ELLIPSOID_MB", "lots")
    assert _dev_call(lib) == -1 and "HTM_ELLIPSOID_MB = lots" in last()
    monkeypatch.setenv("HTM_ELLIPSOID_MB", "-3")
    assert _dev_call(lib) == -1 and "HTM_ELLIPSOID_MB = -3" in last()
    # the host form: the same rules, pivots and piv_corr may be NULL without pivots
    x = np.zeros((10, 6))
    out = np.zeros((2, 22))
    dp = _lib.dp
    assert lib.htm_hypo_ellipsoid(-1, x.ctypes.data_as(dp), None, 3, 2, 0, 1, out.ctypes.data_as(dp), None) == -1 and "need n_mod >= 4" in last()
    assert lib.htm_hypo_ellipsoid(-1, x.ctypes.data_as(dp), None, 10, 2, 1, 1, out.ctypes.data_as(dp), None) == -1 and last() == "NULL argument"
    assert lib.htm_hypo_ellipsoid(-1, None, None, 10, 2, 0, 1, out.ctypes.data_as(dp), None) == -1 and last() == "NULL argument"
    assert lib.htm_hypo_ellipsoid(-1, x.ctypes.data_as(dp), None, 10, 2, 0, 11, out.ctypes.data_as(dp), None) == -1 and "outside 1..10" in last()


def test_no_device_is_an_error_not_a_fallback(monkeypatch):
    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    n = C.c_int(-1)
    if lib.htm_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present; the no-device behaviour is exercised on the CPU-only container")
    monkeypatch.delenv("HTM_ELLIPSOID_MB", raising=False)
    x = np.random.default_rng(0).normal(size=(10, 6))
    out = np.zeros((2, 22))
    assert lib.htm_hypo_ellipsoid(0, x.ctypes.data_as(_lib.dp), None, 10, 2, 0, 5, out.ctypes.data_as(_lib.dp), None) == -2
    assert "no HIP device" in lib.htm_last_error().decode()
    assert _dev_call(lib, device=0) == -2 and "no HIP device" in lib.htm_last_error().decode()
    from hypotremormcmc_amd.ellipsoid import ellipsoid

    with pytest.raises(_lib.HtmError, match="no HIP device"):
        ellipsoid(x)


def test_python_entry_checks_its_input():
    from hypotremormcmc_amd.ellipsoid import ellipsoid

    x = np.random.default_rng(1).normal(size=(10, 6))
    for bad, piv, lv in ((x[:, :5], None, 0.68), (x[:3], None, 0.68), (x, np.zeros((9, 1)), 0.68), (x, np.zeros((10, 5)), 0.68),
                         (x, None, 0.0), (np.where(x > 2, np.nan, x) * np.inf, None, 0.68), (x.reshape(10, 2, 3), None, 0.68)):
        with pytest.raises(ValueError):
            ellipsoid(bad, piv, level=lv)


# ---- the text layer --------------------------------------------------------------------------------------------------
def test_writer_on_hand_made_arrays():
    from hypotremormcmc_amd import ellipsoid as el

    res = {"mean": np.array([[1.0, 2.0, 30.0], [-4.5, 0.25, 12.0]]),
           "cov": np.array([np.diag([4.0, 1.0, 9.0]), [[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.0]]]),
           "lam": np.array([[9.0, 4.0, 1.0], [np.nan] * 3]),
           "axes": np.array([[[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], np.full((3, 3), np.nan)]),
           "q": np.array([4.0, np.nan]), "piv_corr": np.array([[[0.1, 0.2], [0.3, 0.4], [0.5, np.nan]], [[0.0, 0.0], [0.0, 0.0], [np.nan, np.nan]]]),
           "rank": 3}
    rows = el.stat_rows(res, 0.68)
    k2, k3 = el.chi2_quantile(0.68, 2), el.chi2_quantile(0.68, 3)
    assert np.allclose(rows[0], [1, 2, 30, 6, 0, 0, 1, 4, 1, 0, 0, 2, 0, 1, 0, 4 / k3, math.sqrt(4 * k2), math.sqrt(k2), 0.0, 0.5, np.nan],
                       equal_nan=True)
    assert np.all(np.isnan(rows[1, 3:16])) and np.allclose(rows[1, 16:19], [math.sqrt(3 * k2), math.sqrt(k2), 45.0])
    text = el.stat_text([7, 12], rows).split("\n")
    assert text[0].startswith("#") and text[-1] == "" and len(text) == 4
    assert len(text[1]) == len(text[2]) == 8 + sum(w for w, _ in el._FIELDS)
    f1, f2 = text[1].split(), text[2].split()
    assert f1[0] == "7" and f2[0] == "12" and len(f1) == len(f2) == 22
    assert f1[1:5] == ["1.000000", "2.000000", "30.000000", "6.000000"] and f1[-1] == "NaN" and f1[-2] == "0.500000" and f1[-3] == "0.000"
    assert f2[4:17] == ["NaN"] * 13 and f2[19] == "45.000" and f2[1] == "-4.500000"
    s = el.summary_text([7, 12], rows).split("\n")
    assert s[0].startswith("largest semi-axis  6.000000  (window 7)") and "(window 7)" in s[1] and s[2] == "median |corr(z, vs)|  0.500000"
    assert "no ellipsoid" in el.summary_text([12], rows[1:])


def test_horizontal_ellipse_angle():
    from hypotremormcmc_amd.ellipsoid import horizontal_ellipse

    c = lambda a, b, xy: np.array([[[a, xy, 0.0], [xy, b, 0.0], [0.0, 0.0, 1.0]]])
    assert horizontal_ellipse(c(4.0, 1.0, 0.0), 0.5)[0, 2] == 0.0
    assert horizontal_ellipse(c(1.0, 4.0, 0.0), 0.5)[0, 2] == 90.0
    assert horizontal_ellipse(c(2.0, 2.0, -1.0), 0.5)[0, 2] == pytest.approx(135.0)
    h = horizontal_ellipse(c(4.0, 1.0, -1e-300), 0.5)[0]
    assert 0.0 <= h[2] < 180.0

