"""The free-running chain master specialised on what a job fixes (k_mcmc<.., 8>: csrc/htm_flow.hpp FlowFixed)
against the generic instantiation (HTM_FAST=0: same source, run-time answers) and against the oracle.

The specialisation removes selects, branches and address arithmetic and changes no rounding, so every comparison between
the two instantiations is numpy.array_equal; the comparisons with the oracle are those of tests/test_gpu_chains.py (fp64)
and of the fp32-forward tests (tests/test_gpu_fp32.py T1's bound, as tests/test_gpu_wide_chains.py uses it)."""
import numpy as np
import pytest

from tests.test_gpu_chains import RTOL_TRACE, _build_world

pytestmark = pytest.mark.gpu

RTOL_FP32 = 3e-6      # tests/test_gpu_fp32.py T1


def _job(E, S, nc, seed, sz, n_iter, **kw):
    """rejection-heavy as test_rejection_heavy_runs_against_oracle builds it (depth steps several times the prior width), with
    records on: n_burn < n_iter and a short n_interval, so the sample-record block runs"""
    from hypotremormcmc_amd import synth

    data = synth.make_synthetic(E, S, 100 + seed)
    params = dict(synth.DEFAULT_PARAMS, n_procs=1, n_chains=nc, n_cool=min(2, nc), n_iter=n_iter, n_burn=n_iter // 2,
                  n_interval=3, step_size_z=sz, step_size_vs=0.4)
    params.update(kw)
    return data, params


def _set(monkeypatch, data, params, fast, **caps):
    if fast:
        monkeypatch.delenv("HTM_FAST", raising=False)
    else:
        monkeypatch.setenv("HTM_FAST", "0")
    _, sets = _build_world(data, params, **caps)
    return sets[0]


def _bits(cs):
    smp = cs.samples()
    out = dict(rng=np.array(cs.rng_state()), n_propose=cs.counts()[0], n_accept=cs.counts()[1])
    out["lik_iter"], out["lik_chain"], out["lik"] = cs.likelihood_trace()
    for k in ("iter", "vs", "qs", "t_corr", "a_corr", "hypo"):
        out["smp_" + k] = np.asarray(smp[k])
    for c in range(cs.n_chains):
        s = cs.state(c)
        out["hypo_%d" % c] = s.hypo; out["t_corr_%d" % c] = s.t_corr
        out["TL_%d" % c] = np.array([s.temp, s.log_likelihood])
    return out


def _assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _assert_oracle(cs, job, n_iter, fp32):
    it, lk = job.likelihood_trace(0)
    gi, _, gl = cs.likelihood_trace()
    # (every n_interval = 3rd iteration each cool chain leaves a record, and there is at least one cool chain)
    assert len(gi) == len(it) >= n_iter // 3 and np.array_equal(gi, it)
    np.testing.assert_allclose(gl, lk, rtol=RTOL_FP32 if fp32 else RTOL_TRACE)
    assert cs.rng_state() == job.rng_state(0)
    a, b = cs.counts(); oa, ob = job.counts()
    assert np.array_equal(a, oa) and np.array_equal(b, ob)


@pytest.mark.parametrize("nc", [1, 5, 8])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("S", [64, 128])
def test_specialised_master_equals_generic_and_oracle(S, prec, nc, monkeypatch):
    """One rejection-heavy job with records, run four ways: specialised in one launch, generic in one launch (the switch),
    specialised cut into launches of odd lengths with tiny record buffers, specialised continued from a checkpoint.  All four
    give the same bits (traces, samples, counters, chain states, RNG state); the specialised run equals the oracle."""
    from oracle import oracle

    n_iter = 1500
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(64, S, nc, 3, 12.0, n_iter, **kw)
    fast = _set(monkeypatch, data, params, True)
    assert fast.master_stats()["single_rank_loop"] == 3
    fast.run(n_iter)
    assert fast.fixed_master(), "the specialised instantiation was not selected"
    ref = _bits(fast)

    gen = _set(monkeypatch, data, params, False)
    assert gen.master_stats()["single_rank_loop"] == 3
    gen.run(n_iter)
    assert not gen.fixed_master(), "HTM_FAST=0 did not force the generic instantiation"
    _assert_same_bits(ref, _bits(gen), "specialised vs generic")

    # (tiny record buffers -- 4 and 3 records per chain, as test_run_in_pieces_and_small_record_buffers has them -- force drains mid-run)
    cut = _set(monkeypatch, data, params, True, lik_capacity=4 * nc, sample_capacity=3 * nc)
    done = 0
    for n in (1, 7, 400, 13):
        cut.run(n); done += n
    cut.run(n_iter - done)
    assert cut.fixed_master()
    _assert_same_bits(ref, _bits(cut), "one launch vs several")

    first = _set(monkeypatch, data, params, True)
    first.run(600)
    blob = first.checkpoint()
    cont = _set(monkeypatch, data, params, True)
    cont.restore(blob)
    cont.run(n_iter - 600)
    assert cont.fixed_master()
    b = _bits(cont)
    keep = ref["lik_iter"] > 600
    assert np.array_equal(ref["lik_iter"][keep], b["lik_iter"]) and np.array_equal(ref["lik_chain"][keep], b["lik_chain"])
    assert np.array_equal(ref["lik"][keep], b["lik"])
    for k in ref:
        if k.startswith(("rng", "n_", "hypo_", "t_corr_", "TL_")):
            assert np.array_equal(ref[k], b[k]), "continued from a checkpoint: %s differs" % k

    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data); job.run(n_iter)
    _assert_oracle(fast, job, n_iter, prec == "fp32")


@pytest.mark.parametrize("case", ["60 stations", "use_amp = F", "9 chains", "step log"])
def test_other_shapes_run_the_generic_master(case, monkeypatch):
    """what the specialisation does not cover runs the generic instantiation, from what the library observes, and equals the oracle"""
    from oracle import oracle

    n_iter = 1200
    S, nc, kw = 64, 8, {}
    if case == "60 stations":
        S = 60
    elif case == "use_amp = F":
        kw = dict(use_amp="F")
    elif case == "9 chains":
        nc = 9
    data, params = _job(64, S, nc, 1, 4.0, n_iter, **kw)
    monkeypatch.setenv("HTM_MB", "0")      # (9 chains on ONE master workgroup: the free-running loop, two chains on a wave)
    cs = _set(monkeypatch, data, params, True)
    assert cs.master_stats()["single_rank_loop"] == 3
    if case == "step log":
        cs.enable_steplog(n_iter * nc)
    cs.run(n_iter)
    assert not cs.fixed_master(), "%s: the specialised instantiation must not run" % case
    job = oracle.Job(params, data); job.run(n_iter)
    _assert_oracle(cs, job, n_iter, False)
    if case == "step log":
        gi, _ = cs.steplog()
        assert len(gi) == n_iter * nc


def test_two_ranks_run_the_generic_lockstep_master(monkeypatch):
    """n_procs = 2: the lock-step loops, never the specialised single-rank instantiation; traces and counters against the oracle"""
    from hypotremormcmc_amd.parallel import LocalWorld
    from oracle import oracle

    n_iter = 1200
    data, params = _job(64, 64, 8, 1, 4.0, n_iter, n_procs=2)
    monkeypatch.delenv("HTM_FAST", raising=False)
    _, sets = _build_world(data, params)
    LocalWorld(sets).run(n_iter)
    job = oracle.Job(params, data); job.run(n_iter)
    npr = np.zeros(7, np.int64); nac = np.zeros(7, np.int64)
    for r in range(2):
        assert not sets[r].fixed_master()
        it, lk = job.likelihood_trace(r)
        gi, _, gl = sets[r].likelihood_trace()
        assert len(gi) == len(it) > 0 and np.array_equal(gi, it)
        np.testing.assert_allclose(gl, lk, rtol=RTOL_TRACE)
        assert sets[r].rng_state() == job.rng_state(r)
        a, b = sets[r].counts()
        npr += a; nac += b
    oa, ob = job.counts()
    assert np.array_equal(npr, oa) and np.array_equal(nac, ob)


def test_more_than_128_worker_blocks(monkeypatch):
    """10 000 events: 250 worker blocks, four rounds of partial-sum granules in a full evaluation.  The specialised master keeps
    the generic sweep of four rounds (two rounds were measured and not kept: DESIGN.md 10), so it runs here too -- and equals
    the oracle"""
    from oracle import oracle

    n_iter = 150
    data, params = _job(10000, 128, 8, 5, 0.4, n_iter, n_burn=50)
    cs = _set(monkeypatch, data, params, True)
    cs.run(n_iter)
    assert cs.n_worker_blocks > 128, "this job was meant to have more than 128 worker blocks"
    assert cs.fixed_master()
    job = oracle.Job(params, data); job.run(n_iter)
    it, lk = job.likelihood_trace(0)
    gi, _, gl = cs.likelihood_trace()
    assert len(gi) > 50 and np.array_equal(gi, it)
    np.testing.assert_allclose(gl, lk, rtol=RTOL_TRACE)
    assert cs.rng_state() == job.rng_state(0)
    a, b = cs.counts(); oa, ob = job.counts()
    assert np.array_equal(a, oa) and np.array_equal(b, ob)
