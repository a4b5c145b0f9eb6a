"""Convergence diagnostics on the device (hypotremormcmc_amd/csrc/htm_diag.hpp) against the numpy restatement
(tests/diagnose_restatement.py) at the smallest shapes where the kernels can go wrong, and end to end on the files of
a small step-5 run.

Tolerances, with u = 2^-53, S = 2M split sequences of n = N // 2 draws: any order of a lag's S n products is within
S n u acov[0] of the exact sum, so |acov_dev - acov_ref| <= 4 S n u acov_ref[0]; R-hat relative 16 S n u; tau and
ESS relative 16 (lags_used + 2) S n u / tau (lags_used = the lags the Geyer scan looked at, L when it did not
terminate); lags equal.  The Geyer stop is discrete, so every input is first checked to have no pair sum within 1e-6
of zero: no rounding can then move the stop.

Observed maxima on an MI355X, as fractions of these bounds: DESIGN.md §3.6."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import diagnose_restatement as dr
from tests.helpers import load_case, write_run_dir

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# (N, M, n_par, max_lag)
SHAPES = [
    (4, 1, 1, 1000),        # n = 2, L = 1
    (5, 1, 3, 1000),        # odd N, the middle draw dropped
    (9, 3, 65, 1000),       # one lane past a wave
    (35, 2, 130, 16),       # L = n - 1 = 16 exactly
    (34, 2, 63, 16),        # the same, 63 columns
    (36, 2, 64, 17),        # lag count one past a block of 16
    (67, 1, 2, 15),         # lag count one short of a block
    (66, 1, 2, 31),         # 32 lags: one block of 32 exactly
    (68, 2, 3, 1000),       # 34 lags: past a block of 32, n - 1 = L
    (132, 1, 5, 32),        # 33 lags, L = max_lag < n - 1
    (2001, 4, 257, 1000),   # L = 999 = n - 1
    (4100, 2, 70, 1000),    # L = max_lag < n - 1
]


@functools.lru_cache(maxsize=None)
def _case(N, M, n_par, max_lag):
    """input and restatement of a shape, made once: columns of unit normals scaled by 1e-3, 1 or 1e6; column 1 offset by
    1e3, column 2 AR(1) at 0.95, column 3 constant (where n_par has them)"""
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
    x.setflags(write=False)
    ref = dr.diagnose(x, M, max_lag)
    for a in ref:
        a.setflags(write=False)
    const = np.zeros(n_par, bool)
    if n_par > 3:
        const[3] = True
    assert np.array_equal(np.isnan(ref[0][:, 0]), const)
    # a condition on the inputs: no pair sum so close to zero that rounding could move the Geyer stop
    assert np.all(ref[2][~const] > 1e-6), ("change the seed", ref[2][~const].min())
    return x, ref, const


def _compare(shape, out, acov, what=""):
    N, M, n_par, max_lag = shape
    _, (r_out, r_acov, _, r_used), const = _case(*shape)
    n, S = N // 2, 2 * M
    L = min(n - 1, max_lag)
    assert acov.shape == r_acov.shape == (L + 1, n_par)
    assert np.all(np.isnan(out[const])), "a constant column gives four NaN"
    live = ~const
    e_acov = np.max(np.abs(acov - r_acov)[:, live] / (S * n * U * r_acov[0, live]))
    e_rhat = np.max(np.abs(out[live, 0] / r_out[live, 0] - 1) / (S * n * U))
    used = np.where(r_out[live, 3] < 0, L, r_used[live])
    tol_tau = (used + 2) * S * n * U / r_out[live, 2]
    e_tau = max(np.max(np.abs(out[live, 2] / r_out[live, 2] - 1) / tol_tau), np.max(np.abs(out[live, 1] / r_out[live, 1] - 1) / tol_tau))
    print("DIAG %s %s: acov %.3f of 4, rhat %.3f of 16, tau/ess %.3f of 16 (units of S n u ...)" % (shape, what, e_acov, e_rhat, e_tau))
    assert e_acov <= 4
    assert e_rhat <= 16
    assert e_tau <= 16
    assert np.array_equal(out[live, 3], r_out[live, 3])


@pytest.mark.parametrize("lags", [None, "16", "32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_equals_restatement(shape, lags, monkeypatch):
    """lags: the library's own lag block, and both instantiations forced"""
    from hypotremormcmc_amd.diagnose import diagnose

    if lags is not None:
        monkeypatch.setenv("HTM_DIAG_LAGS", lags)
    x, _, _ = _case(*shape)
    out, acov = diagnose(x, shape[1], max_lag=shape[3], return_acov=True)
    _compare(shape, out, acov, "lags=%s" % lags)
    assert np.array_equal(diagnose(x, shape[1], max_lag=shape[3]), out, equal_nan=True), "without acov the same out"


@pytest.mark.parametrize("shape,slabs", [((9, 3, 65, 1000), "1"), ((9, 3, 65, 1000), "4"), ((9, 3, 65, 1000), "64"),
                                         ((2001, 4, 257, 1000), "1"), ((2001, 4, 257, 1000), "3")])
def test_sequence_slabs(shape, slabs, monkeypatch):
    """the split sequences cut into slabs: all in one (a thread adds them all), 6 in 3 slabs of 2 (4 asked for), one
    per slab (more slabs asked for than there are sequences), 8 in ragged slabs of 3, 3, 2"""
    from hypotremormcmc_amd.diagnose import diagnose

    monkeypatch.setenv("HTM_DIAG_SLABS", slabs)
    x, _, _ = _case(*shape)
    out, acov = diagnose(x, shape[1], max_lag=shape[3], return_acov=True)
    _compare(shape, out, acov, "slabs=%s" % slabs)


def test_two_runs_give_the_same_bits():
    from hypotremormcmc_amd.diagnose import diagnose

    shape = (2001, 4, 257, 1000)
    x, _, _ = _case(*shape)
    a = diagnose(x, 4, max_lag=1000, return_acov=True)
    b = diagnose(x, 4, max_lag=1000, return_acov=True)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


def test_dev_form_with_a_row_stride():
    """device pointers, ld = n_par + 3 > n_par, on a stream: the host form's bits"""
    import torch

    from hypotremormcmc_amd import _lib
    from hypotremormcmc_amd.diagnose import diagnose

    shape = (35, 2, 130, 16)
    N, M, n_par, max_lag = shape
    x, _, _ = _case(*shape)
    ld = n_par + 3
    d_x = torch.full((N * M, ld), float("nan"), dtype=torch.float64, device="cuda")
    d_x[:, :n_par] = torch.from_numpy(np.array(x)).cuda()
    d_out = torch.empty((n_par, 4), dtype=torch.float64, device="cuda")
    d_acov = torch.empty((17, n_par), dtype=torch.float64, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    _lib.check(_lib.load().htm_diagnose_dev(0, C.c_void_p(d_x.data_ptr()), M, N, n_par, ld, max_lag, C.c_void_p(d_out.data_ptr()),
                                            C.c_void_p(d_acov.data_ptr()), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    out, acov = d_out.cpu().numpy(), d_acov.cpu().numpy()
    _compare(shape, out, acov, "dev form")
    h_out, h_acov = diagnose(x, M, max_lag=max_lag, return_acov=True)
    assert np.array_equal(out, h_out, equal_nan=True) and np.array_equal(acov, h_acov)


# ---- end to end: the files of a small step-5 run -------------------------------------------------------------------
def _read(path, n_val):
    a = np.fromfile(path, dtype=np.dtype([("it", "<i4"), ("v", "<f8", (n_val,))]))
    return a["it"], a["v"].reshape(len(a), n_val)


def _expected_text(work, n_procs, k, n_burn, names, n_sta, n_ev, max_lag):
    """convergence.stat from the same files by the restatement, with its own reading, ordering and formatting"""
    rows = []
    for r in range(n_procs):
        parts = [_read(os.path.join(work, "%s.%02d.out" % (nm, r)), nv) for nm, nv in
                 (("vs", 1), ("qs", 1), ("t_corr", n_sta), ("a_corr", n_sta), ("hypo", 3 * n_ev))]
        it, lk = _read(os.path.join(work, "likelihood%02d.out" % r), 1)
        vals = np.hstack([p[1] for p in parts] + [lk[it > n_burn]])
        rows += [(int(i), r, j, v) for j, (i, v) in enumerate(zip(parts[0][0], vals))]
    rows.sort(key=lambda t: t[:3])                          # by iteration, then rank, then record order
    n_it = len(rows) // k
    assert all(rows[i * k + j][0] == rows[i * k][0] for i in range(n_it) for j in range(k))
    x = np.array([rows[i * k + j][3] for j in range(k) for i in range(n_it)])
    out = dr.diagnose(x, k, max_lag)[0]
    lines = []
    for name, o in zip(names, out):
        if np.isnan(o[0]):
            lines.append(name.ljust(24) + "NaN".rjust(13) * 3 + "NaN".rjust(7))
        else:
            lines.append(name.ljust(24) + "".join(("%.6f" % v).rjust(13) for v in o[:3]) + str(int(o[3])).rjust(7))
    return lines


@pytest.mark.parametrize("n_procs", [1, 2])
def test_program_writes_convergence_stat(n_procs, tmp_path, monkeypatch, capsys):
    """step 5 on the GPU at fixture fixedcorr's shape (7 events, 9 stations, vs and t_corr fixed, 2 cold chains per rank),
    its files written as the driver writes them, then the program: convergence.stat is the restatement's, to the printed
    digits, with NaN for the fixed parameters"""
    from hypotremormcmc_amd import diagnose as dg, driver
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
    param_file, stations = write_run_dir(tmp_path, data, params, win_id)
    monkeypatch.delenv("HTM_SAMPLE_ENDIAN", raising=False)
    dg.main([param_file, "--max-lag", "40"])
    got = (tmp_path / "convergence.stat").read_text().split("\n")
    names = (["vs", "qs"] + ["t_corr " + s for s in stations] + ["a_corr " + s for s in stations]
             + ["%s %d" % (c, w) for w in win_id for c in "xyz"] + ["log_likelihood"])
    k = 2 * n_procs
    want = _expected_text(str(tmp_path), n_procs, k, 300, names, data.n_sta, data.n_events, 40)
    assert got[0].startswith("#") and got[-1] == "" and len(got) == len(want) + 2
    assert got[1:-1] == want
    assert want[0].split()[1:] == ["NaN"] * 4 and all(w.split()[2] == "NaN" for w in want[2:2 + data.n_sta])
    assert "NaN" not in want[1] and "NaN" not in want[-1]
    s = capsys.readouterr().out
    assert "largest R-hat" in s and "smallest ESS" in s and "%d constant" % (1 + data.n_sta) in s
