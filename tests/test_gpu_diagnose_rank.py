"""Rank-normalised diagnostics on the device (hypotremormcmc_amd/csrc/htm_rank.hpp) against the numpy restatement
(tests/diagnose_rank_restatement.py) at the smallest shapes where the kernels can go wrong, and end to end on the files of a
small step-5 run.

Ranks are exact half-integers: equality.  z: the device evaluates the same rational approximation (AS 241) as the
restatement's statistics.NormalDist, so the two differ by the rounding of log, sqrt and the Horner steps only; the bound is
4 x the largest difference observed on an MI355X over the shapes below (Z_MAX_OBSERVED; profiles/diagnose_rank_tolerances.txt),
and that bound must itself be <= 1e-12, beyond which the transform would be wrong, not rounded.  The final numbers: the
bounds tests/test_gpu_diagnose.py derives (u = 2^-53, S = 2M split sequences of n = N // 2 draws): R-hat relative 16 S n u,
ESS relative 16 (lags_used + 2) S n u / tau, here for the restatement's §3.6 of the DEVICE's z and zf, so that only the
composition is compared (z's own rounding is the check above); the tail-ESS end to end, the indicators being exact; it is
the smaller of two ESS, each within its bound, so it is within the larger of the two relative bounds."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import diagnose_rank_restatement as rr
from tests import diagnose_restatement as dr
from tests.helpers import load_case, write_run_dir

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TILE = 1024                     # kRankTile of htm_rank.hpp: the elements per scatter tile of k_rank_sort
Z_MAX_OBSERVED = 8.881784e-16   # MI355X, the largest |z_dev - z_restatement| over RANK_SHAPES, plain and folded (at 70001 x 3, |z| up to 4.5)
Z_BOUND = 4 * Z_MAX_OBSERVED

# (n_rows, n_par)
RANK_SHAPES = [(2, 1), (8, 1), (1023, 63), (1024, 64), (1025, 65), (4097, 130), (70001, 3),
               (TILE - 1, 12), (TILE, 12), (TILE + 1, 12), (3 * TILE + 1, 12)]


@functools.lru_cache(maxsize=None)
def _rank_case(n_rows, n_par):
    """unit normals scaled by 1e-3, 1 or 1e6, and from column 1 on, where n_par has them: a normal + 1e3, an all-equal column,
    round(2 normal), -0.0 / +0.0 among positives and negatives, subnormals with +-1e300, values that differ in the lowest
    mantissa byte only, values that differ in the exponent's top byte, random bit patterns (every one of the 8 digit passes
    decides), a sorted and a reversed column; with the restatement's ranks and z, plain and folded"""
    rng = np.random.default_rng(77 * n_rows + n_par)
    x = rng.normal(size=(n_rows, n_par)) * rng.choice([1e-3, 1.0, 1e6], size=n_par)
    special = [
        lambda: rng.normal(size=n_rows) + 1e3,
        lambda: np.full(n_rows, -2.5),
        lambda: np.round(2.0 * rng.normal(size=n_rows)),
        lambda: rng.choice([-0.0, 0.0, -0.0, 0.0, 1.5, -1.5, 5e-324, -5e-324], size=n_rows),
        lambda: rng.choice([5e-324, -5e-324, 1e-310, -1e-310, 2e-310, 1e300, -1e300, 0.0], size=n_rows),
        lambda: 1.0 + rng.integers(0, 200, size=n_rows) * 2.0 ** -52,
        lambda: rng.choice([-1.0, 1.0], size=n_rows) * 2.0 ** (16.0 * rng.integers(-60, 61, size=n_rows)),
        lambda: np.nan_to_num(rng.integers(0, 2 ** 64, size=n_rows, dtype=np.uint64).view(np.float64), nan=0.0, posinf=1.0, neginf=-1.0),
        lambda: np.sort(rng.normal(size=n_rows)),
        lambda: np.sort(rng.normal(size=n_rows))[::-1],
    ]
    for c, make in enumerate(special, start=1):
        if c < n_par:
            x[:, c] = make()
    assert np.isfinite(x).all()
    x.setflags(write=False)
    ref = {}
    for fold in (False, True):
        r = rr.ranks(rr.folded(x) if fold else x)
        z = rr.z_of_ranks(r)
        r.setflags(write=False)
        z.setflags(write=False)
        ref[fold] = (r, z)
    return x, ref


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "folded"])
@pytest.mark.parametrize("shape", RANK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ranks_are_exact_and_z_is_close(shape, fold):
    from hypotremormcmc_amd.diagnose import rank_normalize

    x, ref = _rank_case(*shape)
    r_ref, z_ref = ref[fold]
    z, r = rank_normalize(x, fold=fold, return_ranks=True)
    assert np.array_equal(r, r_ref)
    assert r.sum(axis=0).tolist() == [shape[0] * (shape[0] + 1) / 2] * shape[1]
    err = float(np.max(np.abs(z - z_ref)))
    print("RANKZ %s fold=%d: max |z_dev - z_ref| = %.3e (max |z| %.3f)" % (shape, fold, err, np.abs(z_ref).max()))
    assert np.array_equal(rank_normalize(x, fold=fold), z), "without ranks the same z"
    assert Z_BOUND <= 1e-12
    assert err <= Z_BOUND


# ---- the final numbers ------------------------------------------------------------------------------------------------
# (N, M, n_par, max_lag)
SHAPES = [(4, 1, 1, 1000), (5, 1, 3, 1000), (9, 3, 65, 1000), (35, 2, 130, 16), (34, 2, 63, 16), (36, 2, 64, 17),
          (132, 1, 5, 32), (1023, 1, 2, 64), (1025, 2, 66, 64), (4100, 2, 70, 1000)]


@functools.lru_cache(maxsize=None)
def _case(N, M, n_par, max_lag):
    """the input recipe of tests/test_gpu_diagnose.py (columns of unit normals scaled by 1e-3, 1 or 1e6; column 1 offset by
    1e3, column 2 AR(1) at 0.95, column 3 constant) and column 4 round(2 normal), where n_par has them; with the restatement"""
    rng = np.random.default_rng(1000 * N + 10 * M + n_par)
    x = rng.normal(size=(N * M, n_par)) * rng.choice([1e-3, 1.0, 1e6], size=n_par)
    if n_par > 1:
        x[:, 1] = rng.normal(size=N * M) + 1e3
    if n_par > 2:
        e = rng.normal(size=N * M)
        for i in range(1, N * M):
            e[i] = 0.95 * e[i - 1] + np.sqrt(1 - 0.95 ** 2) * e[i]
        x[:, 2] = e
    if n_par > 3:
        x[:, 3] = -2.5
    if n_par > 4:
        x[:, 4] = np.round(2.0 * rng.normal(size=N * M))
    x.setflags(write=False)
    out, parts, refs = rr.diagnose_rank(x, M, max_lag)
    for k, ref in enumerate(refs):
        _assert_no_marginal_pair_sum(ref, "zf" if k == 1 else ("z", "", "I05", "I95")[k])
    return x, out, refs


def _assert_no_marginal_pair_sum(ref, what):
    """a condition on the inputs: no pair sum of a live column so close to zero that rounding could move the Geyer stop"""
    live = ~np.isnan(ref[0][:, 0])
    assert np.all(ref[2][live] > 1e-6), (what, ref[2][live].min())


def _ess_tol(ref, S, n, L):
    """relative bound of the ESS per column (inf where the column is not live)"""
    out, _, _, used = ref
    used = np.where(out[:, 3] < 0, L, used)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(out[:, 0]), np.inf, 16 * (used + 2) * S * n * U / out[:, 2])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_restatement(shape):
    from hypotremormcmc_amd.diagnose import diagnose_rank, rank_normalize

    N, M, n_par, max_lag = shape
    x, r_out, refs = _case(*shape)
    n, S = N // 2, 2 * M
    L = min(n - 1, max_lag)
    out = diagnose_rank(x, M, max_lag=max_lag)
    assert out.shape == (n_par, 4)
    assert np.array_equal(np.isnan(out), np.isnan(r_out)), "the same entries are NaN"
    print("DIAGRANK %s: NaN per column %s" % (shape, np.isnan(r_out).sum(axis=0).tolist()))
    # the restatement's §3.6 of the device's own z and zf
    for col_rhat, col_ess, fold in ((0, 2, False), (1, None, True)):
        ref = dr.diagnose(rank_normalize(x, fold=fold), M, max_lag)
        _assert_no_marginal_pair_sum(ref, "device z, fold=%d" % fold)
        live = ~np.isnan(ref[0][:, 0])
        assert np.array_equal(live, ~np.isnan(out[:, col_rhat]))
        if not live.any():
            continue
        e_rhat = np.max(np.abs(out[live, col_rhat] / ref[0][live, 0] - 1) / (S * n * U))
        print("DIAGRANK %s fold=%d: rhat %.3f of 16 (units of S n u)" % (shape, fold, e_rhat))
        assert e_rhat <= 16
        if col_ess is not None:
            e_ess = np.max(np.abs(out[live, col_ess] / ref[0][live, 1] - 1) / (_ess_tol(ref, S, n, L)[live] / 16))
            print("DIAGRANK %s: ess_bulk %.3f of 16 (units of (lags + 2) S n u / tau)" % (shape, e_ess))
            assert e_ess <= 16
    # the tail-ESS end to end
    live = ~np.isnan(r_out[:, 3])
    if live.any():
        tol = np.maximum(_ess_tol(refs[2], S, n, L), _ess_tol(refs[3], S, n, L))[live]
        e_tail = np.max(np.abs(out[live, 3] / r_out[live, 3] - 1) / (tol / 16))
        print("DIAGRANK %s: ess_tail %.3f of 16" % (shape, e_tail))
        assert e_tail <= 16


def test_batches_do_not_change_the_result(monkeypatch):
    """HTM_RANK_MB=1 at 4097 rows: 16 columns per batch, 130 columns in 9 batches, the last of 2"""
    from hypotremormcmc_amd.diagnose import diagnose_rank, rank_normalize

    x, _ = _rank_case(4097, 130)
    a = [rank_normalize(x, fold=f, return_ranks=True) for f in (False, True)]
    a_out = diagnose_rank(x[:4096], 2, max_lag=64)
    monkeypatch.setenv("HTM_RANK_MB", "1")
    b = [rank_normalize(x, fold=f, return_ranks=True) for f in (False, True)]
    b_out = diagnose_rank(x[:4096], 2, max_lag=64)
    for (za, ra), (zb, rb) in zip(a, b):
        assert np.array_equal(za, zb) and np.array_equal(ra, rb)
    assert np.array_equal(a_out, b_out, equal_nan=True)


def test_two_runs_give_the_same_bits():
    from hypotremormcmc_amd.diagnose import diagnose_rank

    x, _, _ = _case(4100, 2, 70, 1000)
    assert np.array_equal(diagnose_rank(x, 2), diagnose_rank(x, 2), equal_nan=True)


def test_dev_forms_with_row_strides():
    """device pointers, ld = n_par + 3 and ld_z = n_par + 5, on a stream: the host forms' bits, the padding untouched"""
    import torch

    from hypotremormcmc_amd import _lib
    from hypotremormcmc_amd.diagnose import diagnose_rank, rank_normalize

    N, M, n_par, max_lag = 35, 2, 130, 16
    x, _, _ = _case(N, M, n_par, max_lag)
    ld, ld_z = n_par + 3, n_par + 5
    d_x = torch.full((N * M, ld), float("nan"), dtype=torch.float64, device="cuda")
    d_x[:, :n_par] = torch.from_numpy(np.array(x)).cuda()
    d_out = torch.empty((n_par, 4), dtype=torch.float64, device="cuda")
    lib = _lib.load()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    got = {}
    for fold in (0, 1):
        d_z = torch.full((N * M, ld_z), 777.0, dtype=torch.float64, device="cuda")
        d_r = torch.full((N * M, ld_z), 777.0, dtype=torch.float64, device="cuda")
        st.wait_stream(torch.cuda.current_stream())
        _lib.check(lib.htm_rank_normalize_dev(0, C.c_void_p(d_x.data_ptr()), N * M, n_par, ld, fold, C.c_void_p(d_z.data_ptr()), ld_z,
                                              C.c_void_p(d_r.data_ptr()), C.c_void_p(st.cuda_stream)))
        st.synchronize()
        got[fold] = (d_z.cpu().numpy(), d_r.cpu().numpy())
    _lib.check(lib.htm_diagnose_rank_dev(0, C.c_void_p(d_x.data_ptr()), M, N, n_par, ld, max_lag, C.c_void_p(d_out.data_ptr()),
                                         C.c_void_p(st.cuda_stream)))
    st.synchronize()
    for fold in (0, 1):
        z, r = got[fold]
        h_z, h_r = rank_normalize(x, fold=bool(fold), return_ranks=True)
        assert np.array_equal(z[:, :n_par], h_z) and np.array_equal(r[:, :n_par], h_r)
        assert np.all(z[:, n_par:] == 777.0) and np.all(r[:, n_par:] == 777.0)
    assert np.array_equal(d_out.cpu().numpy(), diagnose_rank(x, M, max_lag=max_lag), equal_nan=True)


def test_monotone_invariance_on_the_device():
    from hypotremormcmc_amd.diagnose import diagnose_rank

    x = np.random.default_rng(11).normal(size=(2000, 3))
    a, b = diagnose_rank(x, 4), diagnose_rank(np.exp(x), 4)
    assert np.array_equal(a[:, [0, 2]], b[:, [0, 2]])


# ---- end to end: the files of a small step-5 run -------------------------------------------------------------------
def _read(path, n_val):
    a = np.fromfile(path, dtype=np.dtype([("it", "<i4"), ("v", "<f8", (n_val,))]))
    return a["it"], a["v"].reshape(len(a), n_val)


def _expected_text(work, k, n_burn, names, n_sta, n_ev, max_lag):
    """convergence_rank.stat from the files of rank 0 by the restatement, with its own reading, ordering and formatting"""
    parts = [_read(os.path.join(work, "%s.00.out" % nm), nv) for nm, nv in
             (("vs", 1), ("qs", 1), ("t_corr", n_sta), ("a_corr", n_sta), ("hypo", 3 * n_ev))]
    it, lk = _read(os.path.join(work, "likelihood00.out"), 1)
    vals = np.hstack([p[1] for p in parts] + [lk[it > n_burn]])
    rows = [(int(i), j, v) for j, (i, v) in enumerate(zip(parts[0][0], vals))]
    rows.sort(key=lambda t: t[:2])                          # by iteration, then record order
    n_it = len(rows) // k
    x = np.array([rows[i * k + j][2] for j in range(k) for i in range(n_it)])
    out = rr.diagnose_rank(x, k, max_lag)[0]
    fmt = lambda v: "NaN".rjust(13) if np.isnan(v) else ("%.6f" % v).rjust(13)
    return [name.ljust(24) + fmt(np.fmax(o[0], o[1])) + "".join(fmt(v) for v in o) for name, o in zip(names, out)]


def test_program_writes_convergence_rank_stat(tmp_path, monkeypatch, capsys):
    """the small step-5 run of tests/test_gpu_diagnose.py (fixture fixedcorr's shape, 1 rank, 2 cold chains), then the program
    without and with --rank: without it, convergence.stat and the output are what they are with it minus the rank lines;
    convergence_rank.stat is the restatement's, to the printed digits, with NaN for the fixed parameters"""
    from hypotremormcmc_amd import diagnose as dg, driver
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.parallel import LocalWorld

    _, data, params = load_case("fixedcorr")
    params = dict(params, n_procs="1", n_iter="1500", n_burn="300", n_interval="10")
    obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
    _, cs = driver.build_rank(params, data.sta_x, data.sta_y, data.sta_z, obs, 0, n_procs=1, fwd=None)
    LocalWorld([cs]).run(1500)
    driver.write_outputs(str(tmp_path), 0, cs, endian="little")
    win_id = [3 * j + 2 for j in range(data.n_events)]
    param_file, stations = write_run_dir(tmp_path, data, params, win_id)
    monkeypatch.delenv("HTM_SAMPLE_ENDIAN", raising=False)
    dg.main([param_file, "--max-lag", "40"])
    plain_stat, plain_out = (tmp_path / "convergence.stat").read_text(), capsys.readouterr().out
    assert not (tmp_path / "convergence_rank.stat").exists()
    assert len(plain_out.split("\n")) == 6 and plain_out.startswith("%d parameters (%d constant)\nlargest R-hat  " % (
        1 + data.n_sta + 3 * data.n_events + 1, 1 + data.n_sta))
    dg.main([param_file, "--max-lag", "40", "--rank"])
    rank_out = capsys.readouterr().out
    assert (tmp_path / "convergence.stat").read_text() == plain_stat
    assert rank_out.startswith(plain_out)
    extra = rank_out[len(plain_out):].split("\n")
    assert len(extra) == 4 and extra[3] == "" and extra[0].startswith("largest rank-normalised R-hat  ")
    assert extra[1].startswith("smallest bulk-ESS  ") and "smallest tail-ESS  " in extra[1]
    assert extra[2].startswith("rank-normalised R-hat > 1.01: ")
    got = (tmp_path / "convergence_rank.stat").read_text().split("\n")
    names = (["vs", "qs"] + ["t_corr " + s for s in stations] + ["a_corr " + s for s in stations]
             + ["%s %d" % (c, w) for w in win_id for c in "xyz"] + ["log_likelihood"])
    want = _expected_text(str(tmp_path), 2, 300, names, data.n_sta, data.n_events, 40)
    assert got[0].startswith("#") and got[-1] == "" and len(got) == len(want) + 2
    assert got[1:-1] == want
    assert want[0].split()[1:] == ["NaN"] * 5 and all(w.split()[2:] == ["NaN"] * 5 for w in want[2:2 + data.n_sta])
    assert "NaN" not in want[1] and "NaN" not in want[-1]
