"""The specialised chain master's own corrections in registers and its tail (csrc/htm_flow.hpp FlowOwn): with
one station per lane a chain wave carries the lane's t_corr and a_corr of its chain from step to step instead of loading the
chain's two correction rows at every step (only the wave's own accepted t_corr / a_corr step changes them); the tail of a step
looks at the two decoded types of its look-ahead before it looks at the order book.

None of it changes a rounding or the order of a sum, so every comparison between the specialised and the generic instantiation
(HTM_FAST=0: same source, every value read where it always was) is numpy.array_equal; against the oracle the bounds of
tests/test_gpu_fast_master.py hold.  The register copies are seeded at every launch, so a job cut into many launches (tiny
record buffers) and a job continued from a checkpoint must give the same bits as one launch.  Three events make consecutive
steps of a chain hit the same event: the wave's own-event path of a full evaluation (which patches the lane's copy with the
proposed correction) and the rule that keeps an order two steps ahead from racing the step in between (o == o_mid) run.
128 stations (two stations per lane) keep the loads: the same grid checks that instantiation's path."""
import numpy as np
import pytest

from tests.test_gpu_fast_master import _assert_oracle, _assert_same_bits, _job, _set
from tests.test_gpu_fast_master import _bits as _bits_fast_master

pytestmark = pytest.mark.gpu

N_ITER = 1500


def _bits(cs):
    """tests/test_gpu_fast_master.py's, and every chain's a_corr row (read from the chain state in memory, which the commit writes
    whatever the registers hold: a stale register copy shows in the likelihoods and decisions that follow, not here)"""
    out = _bits_fast_master(cs)
    for c in range(cs.n_chains):
        out["a_corr_%d" % c] = cs.state(c).a_corr
    return out


def _four_ways(data, params, nc, n_iter, monkeypatch):
    """specialised in one launch (returned with its bits), generic, cut into launches, continued from a checkpoint"""
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

    # (4 and 3 records per chain: the buffers fill mid-run, every launch ends early and the next one reseeds the registers)
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
        if k.startswith(("rng", "n_", "hypo_", "t_corr_", "a_corr_", "TL_")):
            assert np.array_equal(ref[k], b[k]), "continued from a checkpoint: %s differs" % k
    return fast


@pytest.mark.parametrize("nc", [1, 5, 8])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("E", [3, 64])
def test_register_state_equals_generic_and_oracle(E, S, prec, nc, monkeypatch):
    """A rejection-heavy job with records on, run four ways: all four give the same bits (traces, samples, counters, chain
    states, RNG state), and the specialised run equals the oracle."""
    from oracle import oracle

    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(E, S, nc, 3, 12.0, N_ITER, **kw)
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data); job.run(N_ITER)
    _assert_oracle(fast, job, N_ITER, prec == "fp32")


@pytest.mark.parametrize("S", [64, 128])
def test_every_refresh_of_the_register_copies_runs(S, monkeypatch):
    """Small steps in vs, qs and the two corrections: those proposals are accepted often, so the lane's register copies of the
    corrections (types 2, 4; registers at S = 64, loads at S = 128) are patched many times, and the accepted vs / qs steps (types
    1, 3) renew the chain's two reciprocals in LDS, which every later partial update of the chain multiplies by -- at least ten
    accepted steps of every type 1-4 on the cool chains, counted by the oracle on the CPU."""
    from oracle import oracle

    nc = 8
    data, params = _job(3, S, nc, 3, 0.4, N_ITER, step_size_vs=0.02, step_size_qs=1.0, step_size_t_corr=0.003,
                        step_size_a_corr=0.0005)
    job = oracle.Job(params, data); job.run(N_ITER)
    _, n_accept = job.counts()
    assert np.all(np.asarray(n_accept)[:4] >= 10), "a type 1-4 was accepted fewer than ten times: %s" % n_accept
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, False)
