"""GPU parity of 33..64 chains on a rank (HTM_MAX_CHAINS): the loop with workgroup barriers in its wide instantiations
(k_mcmc_wide, csrc/htm_mcmc.hpp, and k_step_wide, csrc/htm_step.hpp: step_body at kMaxWideChains).  Criteria as in tests/test_gpu_chains.py: the oracle step by
step, bit-equality between launch shapes of the same job."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_chains import RTOL_TRACE, _build_world

pytestmark = [pytest.mark.gpu]

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _job(E, S, nc, seed, sz, n_iter, n_procs=1, **kw):
    from hypotremormcmc_amd import synth

    data = synth.make_synthetic(E, S, 200 + seed)
    params = dict(synth.DEFAULT_PARAMS, n_procs=n_procs, n_chains=nc, n_cool=2, n_iter=n_iter, n_burn=n_iter // 2, n_interval=3,
                  step_size_z=sz, step_size_vs=0.4)
    params.update(kw)
    return data, params


def _same_as_oracle(cs, job, rank, n_iter):
    it, lk = job.likelihood_trace(rank)
    gi, _, gl = cs.likelihood_trace()
    assert len(gi) == len(it) > 0 and np.array_equal(gi, it), "recorded iterations differ"
    np.testing.assert_allclose(gl, lk, rtol=RTOL_TRACE)
    assert cs.rng_state() == job.rng_state(rank)
    s, o = cs.samples(), job.samples(rank)
    assert np.array_equal(s["iter"], o["iter"])
    np.testing.assert_allclose(s["vs"], o["vs"], rtol=1e-12)
    np.testing.assert_allclose(s["qs"], o["qs"], rtol=1e-12)
    np.testing.assert_allclose(s["hypo"], o["hypo"], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(s["t_corr"], o["t_corr"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(s["a_corr"], o["a_corr"], rtol=1e-11, atol=1e-13)


def _bits(cs):
    return (cs.likelihood_trace(), cs.rng_state(), cs.counts(), cs.samples()["hypo"].copy(),
            [cs.state(c).log_likelihood for c in range(cs.n_chains)])


def _assert_same_bits(a, b):
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    assert a[1] == b[1]
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    assert np.array_equal(a[3], b[3])
    assert a[4] == b[4]


# (100, 64, 40): rejection-heavy (depth steps of 20 km: many Rayleigh-prior rejections, every one a repeated pass)
@pytest.mark.parametrize("E,S,nc,seed,sz,n_iter", [(64, 64, 33, 1, 12.0, 3000), (100, 64, 40, 2, 20.0, 3000),
                                                  (300, 128, 64, 3, 6.0, 2000), (1000, 64, 64, 4, 0.4, 1500)])
def test_wide_chain_sets_against_oracle(E, S, nc, seed, sz, n_iter):
    from oracle import oracle

    data, params = _job(E, S, nc, seed, sz, n_iter)
    job = oracle.Job(params, data); job.run(n_iter)
    _, sets = _build_world(data, params)
    assert sets[0].master_stats()["single_rank_loop"] == 0, "33..64 chains run the loop with barriers"
    sets[0].run(n_iter)
    _same_as_oracle(sets[0], job, 0, n_iter)
    a, b = sets[0].counts(); oa, ob = job.counts()
    assert np.array_equal(a, oa) and np.array_equal(b, ob)


def test_wide_step_log_against_oracle():
    """every step of every one of 64 chains, rejection-heavy: proposal, decision, proposed and running log-likelihood,
    temperature (as tests/test_gpu_chains.py::test_final_state_rng_and_steps_vs_oracle)"""
    from oracle import oracle

    n_iter, nc = 800, 64
    data, params = _job(100, 64, nc, 5, 20.0, n_iter)
    job = oracle.Job(params, data)
    job.enable_steplog(n_iter * nc)
    job.run(n_iter)
    _, sets = _build_world(data, params)
    cs = sets[0]
    cs.enable_steplog(n_iter * nc)
    cs.run(n_iter)
    assert cs.rng_state() == job.rng_state(0)
    oi, od = job.steplog()
    gi, gd = cs.steplog()
    assert len(gi) == len(oi) == n_iter * nc
    assert np.array_equal(gi[:, 0], oi[:, 0]) and np.array_equal(gi[:, 1], oi[:, 2])
    assert np.array_equal(gi[:, 2:7], oi[:, 3:8])
    assert (oi[:, 5] == 0).sum() > n_iter, "not the rejection-heavy regime this test is about"
    ok = oi[:, 5] == 1
    np.testing.assert_allclose(gd[:, 0], od[:, 0], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(gd[ok, 1], od[ok, 1], rtol=RTOL_TRACE)
    np.testing.assert_allclose(gd[:, 2], od[:, 2], rtol=RTOL_TRACE)
    assert np.array_equal(gd[:, 3], od[:, 3])


def test_wide_launch_boundaries_and_checkpoint():
    """48 chains: a run cut into launches of odd lengths with tiny record buffers, and a run resumed from a checkpoint, give the
    bits of the uninterrupted run"""
    n_iter, nc = 1200, 48
    data, params = _job(300, 64, nc, 6, 6.0, n_iter)
    _, a = _build_world(data, params)
    a[0].run(n_iter)
    ref = _bits(a[0])
    _, b = _build_world(data, params, lik_capacity=5 * nc, sample_capacity=5 * nc)
    done = 0
    for n in (1, 7, 400, 13):
        b[0].run(n); done += n
    b[0].run(n_iter - done)
    _assert_same_bits(ref, _bits(b[0]))
    _, c = _build_world(data, params)
    c[0].run(500)
    blob = c[0].checkpoint()
    _, d = _build_world(data, params)
    d[0].restore(blob)
    assert d[0].iterations_done == 500 and d[0].rng_state() == c[0].rng_state()
    d[0].run(n_iter - 500)
    assert d[0].rng_state() == ref[1]
    ia, ca, la = ref[0]; id_, cd, ld = d[0].likelihood_trace()
    keep = ia > 500
    assert np.array_equal(ia[keep], id_) and np.array_equal(ca[keep], cd) and np.array_equal(la[keep], ld)
    assert [d[0].state(k).log_likelihood for k in range(nc)] == ref[4]


def test_wide_two_kernel_path_takes_the_persistent_steps(monkeypatch):
    """HTM_PERSIST=0 (k_step_wide + k_full) at 48 chains: every step, decision, record and random draw of the persistent launch.
    (The log-likelihoods agree to RTOL_TRACE, not bit for bit: k_full sums a full evaluation over its own event tiles, the
    persistent launch over its worker blocks -- as at <= 32 chains, tests/test_gpu_chains.py)"""
    from oracle import oracle

    n_iter, nc = 600, 48
    data, params = _job(300, 64, nc, 7, 6.0, n_iter)
    _, a = _build_world(data, params)
    a[0].enable_steplog(n_iter * nc)
    a[0].run(n_iter)
    monkeypatch.setenv("HTM_PERSIST", "0")
    _, b = _build_world(data, params)
    assert b[0].master_stats()["single_rank_loop"] == -1
    b[0].enable_steplog(n_iter * nc)
    b[0].run(n_iter)
    ai, ad = a[0].steplog()
    bi, bd = b[0].steplog()
    assert len(ai) == len(bi) == n_iter * nc and np.array_equal(ai, bi)
    assert np.array_equal(ad[:, 0], bd[:, 0]) and np.array_equal(ad[:, 3], bd[:, 3])
    np.testing.assert_allclose(bd[:, 1:3], ad[:, 1:3], rtol=RTOL_TRACE)
    assert a[0].rng_state() == b[0].rng_state()
    assert all(np.array_equal(x, y) for x, y in zip(a[0].counts(), b[0].counts()))
    job = oracle.Job(params, data); job.run(n_iter)
    _same_as_oracle(b[0], job, 0, n_iter)


@pytest.mark.parametrize("n_procs,nc,E,S,n_iter", [(2, 40, 100, 64, 1500), (4, 64, 64, 32, 600)])
def test_wide_ranks_lockstep_against_oracle(n_procs, nc, E, S, n_iter):
    """several ranks of 40 / 64 chains (records exchanged by device copies).  4 x 64 chains: the gathered records (4 x 132 doubles)
    exceed the kernel's staging area and are read in place"""
    from hypotremormcmc_amd.parallel import LocalWorld
    from oracle import oracle

    data, params = _job(E, S, nc, 8, 6.0, n_iter, n_procs=n_procs)
    job = oracle.Job(params, data); job.run(n_iter)
    _, sets = _build_world(data, params)
    assert n_procs * (4 + 2 * nc) > 512 or n_procs == 2
    LocalWorld(sets).run(n_iter)
    npr = np.zeros(7, np.int64); nac = np.zeros(7, np.int64)
    for r, cs in enumerate(sets):
        _same_as_oracle(cs, job, r, n_iter)
        a, b = cs.counts(); npr += a; nac += b
    oa, ob = job.counts()
    assert np.array_equal(npr, oa) and np.array_equal(nac, ob)


def test_wide_one_rank_torchworld_over_the_in_kernel_exchange(monkeypatch):
    """a one-rank torchrun job at 40 chains takes the in-kernel exchange (persistent lock-step, k_mcmc_wide<.., 2>: 266-granule
    records, wave 0 collecting them ahead of its chain passes); with record buffers of five iterations the launches end every few
    iterations by the rank's own request.  Same iterations, draws, counters and states as the single-rank driver, and the oracle's
    trace"""
    import socket

    import torch
    import torch.distributed as dist

    from hypotremormcmc_amd.parallel import TorchWorld
    from oracle import oracle

    monkeypatch.setenv("HTM_XCHG", "1")
    n_iter, nc = 900, 40
    data, params = _job(100, 64, nc, 12, 20.0, n_iter)
    _, a = _build_world(data, params)
    a[0].run(n_iter)
    _, b = _build_world(data, params, lik_capacity=5 * nc, sample_capacity=5 * nc)
    assert b[0].master_stats()["lockstep_loop"] == 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        tw = TorchWorld(b[0])
        assert tw.direct, "the in-kernel exchange was not set up"
        tw.run(300)
        tw.run(n_iter - 300)
        torch.cuda.synchronize()
        assert tw.direct and tw.fell_back is None
    finally:
        dist.destroy_process_group()
    assert b[0].iterations_done == n_iter
    ia, ca, la = a[0].likelihood_trace(); ib, cb, lb = b[0].likelihood_trace()
    assert np.array_equal(ia, ib) and np.array_equal(ca, cb)
    np.testing.assert_allclose(lb, la, rtol=RTOL_TRACE, atol=0)
    assert a[0].rng_state() == b[0].rng_state()
    assert all(np.array_equal(x, y) for x, y in zip(a[0].counts(), b[0].counts()))
    for c in range(nc):
        assert np.array_equal(a[0].state(c).hypo, b[0].state(c).hypo) and a[0].state(c).temp == b[0].state(c).temp
    job = oracle.Job(params, data); job.run(n_iter)
    it, lk = job.likelihood_trace(0)
    assert np.array_equal(ib, it)
    np.testing.assert_allclose(lb, lk, rtol=RTOL_TRACE, atol=0)


# (tests/test_gpu_chains.py's driver of 2-3 processes sharing the GPU, each a TorchWorld rank; called under another name so that
# its own parameter list is not collected here a second time)
from tests.test_gpu_chains import test_torchworld_across_processes_sharing_the_gpu as _torchworld_processes  # noqa: E402


@pytest.mark.parametrize("name,world,transport", [("synth:100:64:40:2:1500", 2, "direct"), ("synth:100:64:40:5:1200", 2, "direct-stops"),
                                                  ("synth:64:32:64:3:800", 3, "direct")])
def test_wide_ranks_in_processes_over_the_in_kernel_exchange(name, world, transport):
    """2 x 40 and 3 x 64 chains (3 x 132 doubles: the largest staged gather), one process per rank, swap records written into the
    peers' inboxes from inside k_mcmc_wide<.., 2>: per-rank traces and reduced counters against the oracle's lock-step job
    (rejection-heavy, depth steps of 20 km); "direct-stops": launches end every few iterations by some rank's request"""
    _torchworld_processes(name, world, transport)


def test_wide_fp32_forward_checkpoint_and_decisions():
    """fp32 forward at 48 chains: a checkpoint-resumed run gives the uninterrupted run's bits.  Against the fp64 oracle (common
    random numbers) every one of the 400 x 48 logged decisions is the same, and the proposed and running log-likelihoods agree to
    T1's bound of tests/test_gpu_fp32.py (3e-6 relative).  This is burn-in from the initial guess with 6 km depth steps: the
    differences judged are far larger than the fp32 error, so T5's flips (<= 0.2 % of decisions near the posterior) do not occur
    here -- none in four seeds, proposed log-likelihoods within 8e-8 (profiles/r05_wide_chains.txt)"""
    from oracle import oracle

    n_iter, nc = 400, 48
    data, params = _job(300, 64, nc, 9, 6.0, n_iter, forward_precision="fp32")
    _, a = _build_world(data, params)
    assert a[0].fwd.forward_precision == "fp32"
    a[0].enable_steplog(n_iter * nc)
    a[0].run(n_iter)
    _, b = _build_world(data, params)
    b[0].run(150)
    blob = b[0].checkpoint()
    _, c = _build_world(data, params)
    c[0].restore(blob)
    c[0].run(n_iter - 150)
    ia, ca, la = a[0].likelihood_trace(); ic, cc, lc = c[0].likelihood_trace()
    keep = ia > 150
    assert np.array_equal(ia[keep], ic) and np.array_equal(ca[keep], cc) and np.array_equal(la[keep], lc)
    assert c[0].rng_state() == a[0].rng_state()

    p64 = dict(params); p64.pop("forward_precision")
    job = oracle.Job(p64, data)
    job.enable_steplog(n_iter * nc)
    job.run(n_iter)
    oi, od = job.steplog()
    gi, gd = a[0].steplog()
    assert len(gi) == len(oi) == n_iter * nc
    assert np.array_equal(gi[:, 0], oi[:, 0]) and np.array_equal(gi[:, 1], oi[:, 2])
    assert np.array_equal(gi[:, 2:7], oi[:, 3:8]), "a decision differs from the fp64 oracle"
    np.testing.assert_allclose(gd[:, 0], od[:, 0], rtol=1e-12, atol=1e-13)
    assert np.array_equal(gd[:, 3], od[:, 3])
    ok = oi[:, 5] == 1
    np.testing.assert_allclose(gd[ok, 1], od[ok, 1], rtol=3e-6)
    np.testing.assert_allclose(gd[:, 2], od[:, 2], rtol=3e-6)
    assert a[0].rng_state() == job.rng_state(0)


@pytest.mark.parametrize("knob", ["HTM_MB", "HTM_PIPE", "HTM_FLOW"])
def test_wide_loop_selection_and_refusals(knob, monkeypatch):
    """the knobs of the other loops are no error at 40 chains: the loop with barriers runs; 65 chains are refused, by the C ABI too"""
    from hypotremormcmc_amd import _lib
    from hypotremormcmc_amd.chains import ChainSet
    from oracle import oracle

    monkeypatch.setenv(knob, "1")
    n_iter = 300
    data, params = _job(100, 64, 40, 10, 6.0, n_iter)
    fwd, sets = _build_world(data, params)
    st = sets[0].master_stats()
    assert st["single_rank_loop"] == 0 and st["lockstep_loop"] == 2
    sets[0].run(n_iter)
    job = oracle.Job(params, data); job.run(n_iter)
    _same_as_oracle(sets[0], job, 0, n_iter)
    with pytest.raises(ValueError, match="64"):
        ChainSet(fwd, [None] * 65, np.ones(65), (1, 2, 3, 4))
    lib = _lib.load()
    init = _lib.ChainsInit()
    init.n_chains, init.n_procs, init.rank = 65, 1, 0
    h = C.c_void_p()
    assert lib.htm_chains_create(fwd.handle, C.byref(init), C.byref(h)) == -1 and not h.value
    assert b"64" in lib.htm_last_error()


def test_fortran_step5_program_at_40_chains(tmp_path):
    """the Fortran step-5 program with n_chains = 40, n_procs = 1 writes the sample and likelihood files of the Python driver"""
    from hypotremormcmc_amd import synth

    exe = os.path.join(ROOT, "hypotremormcmc_amd", "fortran", "build", "hypo_tremor_mcmc_hip")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run `make -C hypotremormcmc_amd/fortran` (build() does)")
    n_iter, nc = 600, 40
    data, params = _job(100, 32, nc, 11, 6.0, n_iter)
    synth.write_dataset(str(tmp_path), data)
    synth.write_param_file(str(tmp_path / "run.in"), **params)
    subprocess.run([exe, "run.in"], cwd=tmp_path, check=True, timeout=600, stdout=subprocess.DEVNULL,
                   env=dict(os.environ, HTM_SAMPLE_ENDIAN="little"))
    _, sets = _build_world(data, params)
    cs = sets[0]
    cs.run(n_iter)

    def records(name, n_val):
        a = np.fromfile(tmp_path / name, dtype=np.dtype([("iter", "<i4"), ("val", "<f8", (n_val,))]))
        return a["iter"], a["val"].reshape(-1, n_val)

    E, S = data.n_events, data.n_sta
    gi, _, gl = cs.likelihood_trace()
    it, v = records("likelihood00.out", 1)
    assert len(it) > 0 and np.array_equal(it, gi)
    np.testing.assert_allclose(v[:, 0], gl, rtol=RTOL_TRACE, atol=0)
    s = cs.samples()
    for nm, nv in (("vs", 1), ("qs", 1), ("t_corr", S), ("a_corr", S), ("hypo", 3 * E)):
        it, v = records(f"{nm}.00.out", nv)
        assert len(it) > 0 and np.array_equal(it, s["iter"]), nm
        np.testing.assert_allclose(v, s[nm].reshape(len(it), nv), rtol=1e-11, atol=1e-12, err_msg=nm)
