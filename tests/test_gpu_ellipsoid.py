"""Location error ellipsoids on the device (hypotremormcmc_amd/csrc/htm_ellipsoid.hpp) against the numpy restatement
(tests/ellipsoid_restatement.py) at the smallest shapes where the kernels can go wrong, and end to end on the files of a
small step-5 run.

Tolerances, with u = 2^-53, n = n_mod, sigma_a the restatement's standard deviation of column a, C a window's covariance:
mean 4 n u (|mean| + sigma); any summation order of n centred products is within n u (n - 1) sigma_a sigma_b of the exact
sum, so |cov_dev - cov_ref| <= 4 n u sigma_a sigma_b; correlations 8 n u absolute.  The axes are not compared vector by
vector: V Lambda V^T against C_dev (Frobenius, relative to |C_dev|) and V^T V against I, each within 8 x the larger of
numpy.linalg.eigh's own residual on the same C_dev and 8 u; descending order; the sign convention; eigenvalues against
eigh(C_ref) within 4 n u tr(C) + the reconstruction bound (Weyl).  A relative change eps of C moves a squared Mahalanobis
distance by at most cond(C) eps and an order statistic by no more than the largest change of its inputs, so
|q_dev - q_ref| <= 4 cond(C) n u q_ref; d2 itself is not exposed, so q is compared at the ranks 1, ceil(n / 2) and n, which pin
the smallest, the middle and the largest distance.

The inputs are checked for what these bounds assume (condition number <= 1e4, relative eigenvalue gaps >= 1e-3, an
unambiguous sign, |mean| <= the largest column standard deviation of the window): a window that misses one is drawn again,
and the fixture asserts them all.

Observed maxima on an MI355X, as fractions of these bounds: DESIGN.md §3.8."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from tests import ellipsoid_restatement as er
from tests.helpers import load_case, write_run_dir

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# (n_mod, n_win, n_piv)
SHAPES = [
    (4, 1, 0),          # least n_mod, one window, no pivots
    (5, 1, 1),          # one pivot
    (40, 21, 2),        # 63 columns
    (41, 22, 0),        # 66 columns: window 21 straddles the 64-lane boundary of the first load
    (7, 64, 1),         # exactly one wave's 192 columns
    (9, 65, 2),         # one window past a wave
    (33, 43, 4),        # most pivots; windows straddling both lane boundaries
    (1001, 43, 2),      # rows not a multiple of anything
    (4100, 130, 2),     # several row slabs by default
]
_ids = lambda s: "x".join(map(str, s))


def _conditions(r):
    """what the bounds assume of one window (r = its restatement): cond, smallest relative gap, sign margin, |mean| / sigma_max"""
    lam, V = r["lam"][0], r["axes"][0]
    a = np.sort(np.abs(V), axis=0)
    sig = np.sqrt(np.diag(r["cov"][0]))
    return lam[0] / lam[2], min(lam[0] - lam[1], lam[1] - lam[2]) / lam[0], np.min(a[2] - a[1]), np.max(np.abs(r["mean"][0])) / sig.max()


def _good(c):
    return c[0] <= 1e4 and c[1] >= 1e-3 and c[2] >= 1e-6 and c[3] <= 1.0


@functools.lru_cache(maxsize=None)
def _inputs(n_mod, n_win, n_piv):
    """per window A z + offset: z standard normal, A a random 3 x 3 times 1e-3, 1 or 1e3, the offset within the window's
    own spread; pivot k follows z of window k (mod n_win) with noise of its own.  Made once."""
    rng = np.random.default_rng(100000 * n_mod + 10 * n_win + n_piv)
    x = np.empty((n_mod, 3 * n_win))
    for w in range(n_win):
        for _ in range(200):
            A = rng.normal(size=(3, 3)) * rng.choice([1e-3, 1.0, 1e3])
            xw = rng.normal(size=(n_mod, 3)) @ A.T
            xw += rng.uniform(-0.4, 0.4, size=3) * xw.std(axis=0).max() - xw.mean(axis=0)
            if _good(_conditions(er.ellipsoid(xw))):
                break
        assert _good(_conditions(er.ellipsoid(xw))), ("change the seed", (n_mod, n_win, n_piv), w)
        x[:, 3 * w:3 * w + 3] = xw
    piv = None
    if n_piv:
        piv = np.empty((n_mod, n_piv))
        for k in range(n_piv):
            z = x[:, 3 * (k % n_win) + 2]
            piv[:, k] = (z - z.mean()) / z.std() * rng.choice([1e-2, 1.0, 1e2]) + rng.normal(size=n_mod)
            piv[:, k] += 0.3 * piv[:, k].std() - piv[:, k].mean()
        piv.setflags(write=False)
    x.setflags(write=False)
    return x, piv


def _ranks(n_mod):
    return [1, (n_mod + 1) // 2, n_mod]


@functools.lru_cache(maxsize=None)
def _case(n_mod, n_win, n_piv):
    """input and restatement (q at the three ranks) of a shape, made once"""
    x, piv = _inputs(n_mod, n_win, n_piv)
    ref = er.ellipsoid(x, piv, rank=_ranks(n_mod))
    for a in ref.values():
        a.setflags(write=False)
    assert not ref["const"].any() and np.all(np.isfinite(ref["q"]))
    return x, piv, ref


def _run(x, piv, rank):
    """htm_hypo_ellipsoid: out [n_win][22], piv_corr [n_win][3][n_piv]"""
    from hypotremormcmc_amd import _lib

    n_mod, n_win = x.shape[0], x.shape[1] // 3
    n_piv = 0 if piv is None else piv.shape[1]
    out = np.full((n_win, 22), -7.0)
    corr = np.full((n_win, 3, n_piv), -7.0)
    xc = np.ascontiguousarray(x)
    pc = np.ascontiguousarray(piv) if n_piv else None
    _lib.check(_lib.load().htm_hypo_ellipsoid(0, xc.ctypes.data_as(_lib.dp), pc.ctypes.data_as(_lib.dp) if n_piv else None, n_mod, n_win,
                                               n_piv, rank, out.ctypes.data_as(_lib.dp), corr.ctypes.data_as(_lib.dp) if n_piv else None))
    return out, corr


def _cov3(out):
    c = out[:, 3:9]
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)


def _compare(shape, ref, out, corr, i_rank, what=""):
    """all of a call's numbers against the restatement; ref["q"][:, i_rank] is the call's rank.  Prints and returns the
    largest fraction of each bound."""
    n, n_win, n_piv = shape
    sig = np.sqrt(np.stack([np.diag(c) for c in ref["cov"]]))                 # [n_win][3]
    f = {}
    f["mean"] = np.max(np.abs(out[:, 0:3] - ref["mean"]) / (4 * n * U * (np.abs(ref["mean"]) + sig)))
    cov = _cov3(out)
    f["cov"] = np.max(np.abs(cov - ref["cov"]) / (4 * n * U * sig[:, :, None] * sig[:, None, :]))
    f["corr"] = np.max(np.abs(corr - ref["piv_corr"]) / (8 * n * U)) if n_piv else 0.0
    lam, V = out[:, 9:12], out[:, 12:21].reshape(n_win, 3, 3)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(corr))
    f["rec"] = f["orth"] = f["lam"] = f["q"] = 0.0
    for w in range(n_win):
        nc = np.linalg.norm(cov[w])
        le, Ve = np.linalg.eigh(cov[w])
        b_rec = 8 * max(np.linalg.norm(Ve @ np.diag(le) @ Ve.T - cov[w]) / nc, 8 * U)
        b_orth = 8 * max(np.linalg.norm(Ve.T @ Ve - np.eye(3)), 8 * U)
        f["rec"] = max(f["rec"], np.linalg.norm(V[w] @ np.diag(lam[w]) @ V[w].T - cov[w]) / nc / b_rec)
        f["orth"] = max(f["orth"], np.linalg.norm(V[w].T @ V[w] - np.eye(3)) / b_orth)
        assert lam[w, 0] >= lam[w, 1] >= lam[w, 2] > 0, (w, lam[w])
        assert all(V[w, np.argmax(np.abs(V[w, :, k])), k] > 0 for k in range(3)), (w, V[w])
        lr = np.linalg.eigvalsh(ref["cov"][w])[::-1]
        f["lam"] = max(f["lam"], np.max(np.abs(lam[w] - lr)) / (4 * n * U * np.trace(ref["cov"][w]) + b_rec * nc))
        q_ref = ref["q"][w, i_rank]
        f["q"] = max(f["q"], abs(out[w, 21] - q_ref) / (4 * (lr[0] / lr[2]) * n * U * q_ref))
    print("ELL %s %s rank#%d: " % (_ids(shape), what, i_rank) + ", ".join("%s %.3f" % kv for kv in f.items()) + " (fractions of the bounds)")
    for k, v in f.items():
        assert v <= 1.0, (k, v)
    return f


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_device_equals_restatement(shape, monkeypatch):
    monkeypatch.delenv("HTM_ELL_SLABS", raising=False)
    monkeypatch.delenv("HTM_ELLIPSOID_MB", raising=False)
    x, piv, ref = _case(*shape)
    first = None
    for i, rank in enumerate(_ranks(shape[0])):
        out, corr = _run(x, piv, rank)
        _compare(shape, ref, out, corr, i)
        if first is None:
            first = out
        assert np.array_equal(out[:, :21], first[:, :21]), "the rank changes q alone"


@pytest.mark.parametrize("slabs", ["1", "2", "3", "7"])
@pytest.mark.parametrize("shape", [(1001, 43, 2), (4100, 130, 2)], ids=_ids)
def test_row_slabs(shape, slabs, monkeypatch):
    """the rows in one slab (a thread adds them all), in two, in three ragged ones, in seven"""
    monkeypatch.setenv("HTM_ELL_SLABS", slabs)
    x, piv, ref = _case(*shape)
    out, corr = _run(x, piv, _ranks(shape[0])[1])
    _compare(shape, ref, out, corr, 1, "slabs=%s" % slabs)


def test_window_batches_give_the_same_bits(monkeypatch):
    """HTM_ELLIPSOID_MB=1 at 2100 rows: 62 windows' worth, so batches of one wave's 64 windows -- three of them for 130"""
    x, _ = _inputs(2100, 130, 0)
    monkeypatch.delenv("HTM_ELLIPSOID_MB", raising=False)
    a, _ = _run(x, None, 1428)
    monkeypatch.setenv("HTM_ELLIPSOID_MB", "1")
    b, _ = _run(x, None, 1428)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    ref = er.ellipsoid(x[:, 3 * 129:], rank=1428)             # the last window: alone in the third batch
    assert abs(b[129, 21] - ref["q"][0]) <= 4 * (ref["lam"][0, 0] / ref["lam"][0, 2]) * 2100 * U * ref["q"][0]


def test_two_calls_give_the_same_bits():
    x, piv, _ = _case(1001, 43, 2)
    a, b = _run(x, piv, 681), _run(x, piv, 681)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_dev_form_with_row_strides():
    """device pointers, ld = 3 n_win + 5 and ld_piv = n_piv + 3 with NaN beyond the columns (never read), on a stream of its
    own: the host form's bits"""
    import torch

    from hypotremormcmc_amd import _lib

    shape = (33, 43, 4)
    n_mod, n_win, n_piv = shape
    x, piv, ref = _case(*shape)
    rank = _ranks(n_mod)[1]
    d_x = torch.full((n_mod, 3 * n_win + 5), float("nan"), dtype=torch.float64, device="cuda")
    d_x[:, :3 * n_win] = torch.from_numpy(np.array(x)).cuda()
    d_p = torch.full((n_mod, n_piv + 3), float("nan"), dtype=torch.float64, device="cuda")
    d_p[:, :n_piv] = torch.from_numpy(np.array(piv)).cuda()
    d_out = torch.full((n_win, 22), -7.0, dtype=torch.float64, device="cuda")
    d_corr = torch.full((n_win, 3, n_piv), -7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    _lib.check(_lib.load().htm_hypo_ellipsoid_dev(0, C.c_void_p(d_x.data_ptr()), 3 * n_win + 5, C.c_void_p(d_p.data_ptr()), n_piv + 3, n_mod,
                                                   n_win, n_piv, rank, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_corr.data_ptr()),
                                                   C.c_void_p(st.cuda_stream)))
    st.synchronize()
    out, corr = d_out.cpu().numpy(), d_corr.cpu().numpy()
    _compare(shape, ref, out, corr, 1, "dev form")
    h_out, h_corr = _run(x, piv, rank)
    assert np.array_equal(out, h_out) and np.array_equal(corr, h_corr)


def test_degenerate_windows():
    """(40, 5, 2): window 1 with a constant z; window 3 with y a copy of x -- equal columns give equal moments bit for bit, the
    first Jacobi rotation (theta = 0, t = 1) then annihilates one eigenvalue exactly and every later rotation about it is
    skipped, so lambda_3 = 0 is no matter of rounding; pivot 1 constant.  The other windows do not notice."""
    x, piv, _ = _case(40, 5, 2)
    rank = 28
    base, base_corr = _run(x, piv, rank)
    y, p = np.array(x), np.array(piv)
    y[:, 3 * 1 + 2] = -3.75
    y[:, 3 * 3 + 1] = y[:, 3 * 3]
    p[:, 1] = 0.1
    out, corr = _run(y, p, rank)
    ref = er.ellipsoid(y, p, rank=rank)
    assert np.all(np.isnan(ref["lam"][1])) and np.all(np.isnan(ref["piv_corr"][:, :, 1]))
    sig = np.sqrt(np.stack([np.diag(c) for c in ref["cov"]]))
    assert np.all(np.abs(out[:, 0:3] - ref["mean"]) <= 4 * 40 * U * (np.abs(ref["mean"]) + sig))
    assert np.all(np.abs(_cov3(out) - ref["cov"]) <= 4 * 40 * U * sig[:, :, None] * sig[:, None, :])
    # window 1: the constant coordinate's mean is the constant, its covariances are exact zeros; no axes
    assert out[1, 2] == -3.75 and np.all(out[1, [5, 7, 8]] == 0.0) and np.all(out[1, [3, 4, 6]] != 0.0)
    assert np.all(np.isnan(out[1, 9:22])) and np.all(np.isnan(corr[1, 2, :])) and np.all(np.isfinite(corr[1, :2, 0]))
    # window 3: a plane
    assert np.all(np.isnan(out[3, 9:22])) and np.all(np.isfinite(out[3, 0:9]))
    assert out[3, 3] == out[3, 4] == out[3, 6] and out[3, 5] == out[3, 7]
    # pivot 1: NaN in its column only
    assert np.all(np.isnan(corr[:, :, 1]))
    live = np.ones((5, 3), bool)
    live[1, 2] = False
    assert np.all(np.isfinite(corr[:, :, 0][live]))
    assert np.all(np.abs(corr[:, :, 0][live] - ref["piv_corr"][:, :, 0][live]) <= 8 * 40 * U)
    for w in (0, 2, 4):
        assert np.array_equal(out[w], base[w]) and np.array_equal(corr[w, :, 0], base_corr[w, :, 0]), w
        assert np.all(np.isfinite(out[w]))


# ---- end to end: the files of a small step-5 run -------------------------------------------------------------------
def _read(path, n_val):
    a = np.fromfile(path, dtype=np.dtype([("it", "<i4"), ("v", "<f8", (n_val,))]))
    return a["it"], a["v"].reshape(len(a), n_val)


def _expected_rows(work, n_procs, n_ev, level):
    """per window the 21 numbers of a line and the tolerance of each: the restatement on the same files, read here, with
    this test's own formulas for what the program derives; tolerance = the bounds above carried to each number"""
    hyp = np.vstack([_read(os.path.join(work, "hypo.%02d.out" % r), 3 * n_ev)[1] for r in range(n_procs)])
    piv = np.vstack([np.hstack([_read(os.path.join(work, "%s.%02d.out" % (nm, r)), 1)[1] for nm in ("vs", "qs")]) for r in range(n_procs)])
    n = len(hyp)
    rank = min(n, max(1, math.ceil(level * n)))
    ref = er.ellipsoid(hyp, piv, rank=rank)
    assert not ref["const"].any() and np.all(np.isfinite(ref["lam"]))
    k2, k3 = -2.0 * math.log(1.0 - level), 3.5058823558
    assert level == 0.68
    rows, tols = np.empty((n_ev, 21)), np.empty((n_ev, 21))
    for w in range(n_ev):
        C3, lam, V, q = ref["cov"][w], ref["lam"][w], ref["axes"][w], ref["q"][w]
        sig = np.sqrt(np.diag(C3))
        # samples of a real run lie far from the origin in units of their spread: x - mean carries u |mean| / sigma
        far = 1.0 + np.max(np.abs(ref["mean"][w])) / sig.min()
        E = 4 * (lam[0] / lam[2]) * n * U * far
        gap = min(lam[0] - lam[1], lam[1] - lam[2])
        mu = np.linalg.eigvalsh(C3[:2, :2])[::-1]
        ang = math.degrees(0.5 * math.atan2(2 * C3[0, 1], C3[0, 0] - C3[1, 1])) % 180.0
        rows[w] = np.concatenate([ref["mean"][w], *[[math.sqrt(q * lam[k]), *V[:, k]] for k in range(3)], [q / k3],
                                  np.sqrt(k2 * mu), [ang], ref["piv_corr"][w, 2]])
        t_axis = 8 * n * U * np.linalg.norm(C3) / gap + 64 * U
        tols[w] = np.concatenate([4 * n * U * (np.abs(ref["mean"][w]) + sig),
                                  *[[(2 * E + 32 * U) * math.sqrt(q * lam[k]), t_axis, t_axis, t_axis] for k in range(3)], [E * q / k3 + 1e-10],
                                  4 * n * U * mu.sum() / mu[1] * np.sqrt(k2 * mu), [math.degrees(4 * n * U * mu.sum() / (mu[0] - mu[1]))],
                                  [8 * n * U, 8 * n * U]])
    return rows, tols


@pytest.mark.parametrize("n_procs", [1, 2])
def test_program_writes_hypo_ellipsoid_stat(n_procs, tmp_path, monkeypatch, capsys):
    """step 5 on the GPU at fixture fixedcorr's shape (7 events, vs fixed, 2 cold chains per rank), its files written as the
    driver writes them, then the program: every number of hypo_ellipsoid.stat is the restatement's to half a unit of its
    last printed digit plus the bounds; NaN exactly in the vs column"""
    from hypotremormcmc_amd import driver, ellipsoid as el
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.parallel import LocalWorld

    _, data, params = load_case("fixedcorr")
    params = dict(params, n_procs=str(n_procs), n_iter="1500", n_burn="300", n_interval="10")
    obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
    fwd, sets = None, []
    for r in range(n_procs):
        fwd, cs = driver.build_rank(params, data.sta_x, data.sta_y, data.sta_z, obs, r, n_procs=n_procs, fwd=fwd)
        sets.append(cs)
    LocalWorld(sets).run(1500)
    for r, cs in enumerate(sets):
        driver.write_outputs(str(tmp_path), r, cs, endian="little")
    win_id = [3 * j + 2 for j in range(data.n_events)]
    param_file, _ = write_run_dir(tmp_path, data, params, win_id)
    monkeypatch.delenv("HTM_SAMPLE_ENDIAN", raising=False)
    monkeypatch.delenv("HTM_ELL_SLABS", raising=False)
    monkeypatch.delenv("HTM_ELLIPSOID_MB", raising=False)
    el.main([param_file, "--level", "0.68"])
    got = (tmp_path / "hypo_ellipsoid.stat").read_text().split("\n")
    assert got[0].startswith("#") and got[-1] == "" and len(got) == data.n_events + 2
    rows, tols = _expected_rows(str(tmp_path), n_procs, data.n_events, 0.68)
    digits = np.array([6] * 18 + [3] + [6] * 2)
    worst = 0.0
    for w, line in enumerate(got[1:-1]):
        fld = line.split()
        assert len(fld) == 22 and int(fld[0]) == win_id[w]
        assert [j for j, s in enumerate(fld) if s == "NaN"] == [20], "NaN in the vs column and nowhere else"
        assert np.isnan(rows[w, 19])
        for j in range(21):
            if j == 19:
                continue
            v = float(fld[1 + j])
            err = abs(v - rows[w, j])
            if j == 18:
                err = min(err, 180.0 - err)         # an angle at the ends of [0, 180)
            lim = 0.5 * 10.0 ** -digits[j] + tols[w, j]
            worst = max(worst, err / lim)
            assert err <= lim * (1 + 1e-9), (w, j, v, rows[w, j], lim)
    s = capsys.readouterr().out
    print("ELL program n_procs=%d: worst %.3f of half a printed unit plus the bound" % (n_procs, worst))
    assert "largest semi-axis" in s and "farthest from 1" in s and "median |corr(z, vs)|  NaN" in s
