"""The specialised chain master between two steps (csrc/htm_flow.hpp, the loop of flow_body and the two ends of flow_step; DESIGN.md
3.0 and 10): a full evaluation looks ahead as a partial update does -- the step after it starts from FlowNext and the wave's B2
comes from FlowNext::b3 instead of a walk through the hop table and the swap record.

The same words are compared and the same values added and stored as in the generic instantiation (HTM_FAST=0), so every comparison
with it is numpy.array_equal; against the oracle the bounds of tests/test_gpu_fast_master.py hold.

Where this code can go wrong, and the smallest shapes that reach it (about 1 500 iterations):
  3 events x 64 stations, long enough for a hundred full evaluations that follow one another and a hundred followed by a hypocentre
  step -- the new look-ahead, and a step behind a step that had none (iteration 1, a rejected prior, a window that did not cover
  the look-up); 1 event: every hypocentre step hits the event of the one before.
  1, 2, 3 and 8 chains (no swap; the pair is always the two waves; the hop tables at c = 0 .. 7), 64 stations (corrections in
  registers) and 128 (two stations per lane), fp64 and fp32.
  64 events: nearly every step is a partial update -- the start from FlowNext and B2 from FlowNext::b3, as before.
  Priors that reject: epochs change at the loop top and in the turn, and the rare path is entered from both.
  Launches of ONE iteration: the launch's end is seen at the top of every step; the evaluation counters add up over the launches.
  A launch that chain 0's wave ends itself (record buffers full, stop code 1).
  Swaps accepted often: the commit's stores of the temperature rings.
Conditions on a job are asserted on the ORACLE's step log, on the CPU."""
import numpy as np
import pytest

from tests.test_gpu_fast_master import _assert_oracle, _assert_same_bits, _job, _set
from tests.test_gpu_own_state import _bits, _four_ways

pytestmark = pytest.mark.gpu

N_ITER = 1500


def _oracle(data, params, n_iter):
    """the oracle's run with its step log, rows in (iteration, chain) order: (job, ir) with ir = iter, rank, chain, type, index,
    prior ok, accepted, full evaluation"""
    from oracle import oracle

    nc = int(params["n_chains"])
    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data)
    job.enable_steplog(n_iter * nc)
    job.run(n_iter)
    ir, _ = job.steplog()
    assert len(ir) == n_iter * nc and np.array_equal(ir[:nc, 2], np.arange(nc))
    return job, ir


def _followers(ir, n_iter, nc):
    """(full evaluations followed directly -- the same chain's next step -- by another one, ... by a hypocentre step)"""
    full = (ir[:, 7] != 0).reshape(n_iter, nc)
    hyp = (ir[:, 3] >= 5).reshape(n_iter, nc)
    return int(np.sum(full[:-1] & full[1:])), int(np.sum(full[:-1] & hyp[1:]))


# iterations at 3 events x 64 stations, by chains: enough for the oracle to count the followers asked for below (a full evaluation is
# followed by another one of the same chain after one step in a hundred)
N_ITER_FULL = {1: 15000, 2: 6000, 3: 6000, 8: 2500}


# every value of (chains, stations, precision, events) at least twice; 8 x 64 is the shape bench.py runs
@pytest.mark.parametrize("nc,S,prec,E", [(1, 64, "fp64", 3), (2, 64, "fp32", 3), (3, 64, "fp64", 3), (8, 64, "fp64", 3),
                                         (8, 64, "fp32", 1), (1, 128, "fp32", 1), (2, 128, "fp64", 1), (3, 128, "fp32", 3),
                                         (8, 128, "fp64", 3)])
def test_full_evaluations_and_the_steps_behind_them(nc, S, prec, E, monkeypatch):
    """One job with records on, run four ways -- specialised in one launch, generic, cut into launches (1, 7, 400, 13, the rest),
    continued from a checkpoint: the same bits; the specialised run equals the oracle.  At 3 events x 64 stations at least 100 full
    evaluations are followed directly (the chain's next step) by another one and at least 100 by a hypocentre step.

    (The share of full evaluations is not an input: a step perturbs vs, qs or a correction -- a full evaluation -- with probability
    4 x 0.025 whatever the job (cls_mcmc.f90:91-107, :139-165), so one step in ten is one, and every step of iteration 1.  No job of
    1 500 iterations has the oracle run more than half of its steps as full evaluations; the counts below are what a job can give.)"""
    n_iter = N_ITER_FULL[nc] if (E == 3 and S == 64) else N_ITER
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(E, S, nc, 3, 12.0, n_iter, **kw)
    job, ir = _oracle(data, params, n_iter)
    if E == 3 and S == 64:
        ff, fh = _followers(ir, n_iter, nc)
        assert ff >= 100 and fh >= 100, "full evaluations followed by a full evaluation: %d, by a hypocentre step: %d" % (ff, fh)
    fast = _four_ways(data, params, nc, n_iter, monkeypatch)
    _assert_oracle(fast, job, n_iter, prec == "fp32")


@pytest.mark.parametrize("nc,S,prec", [(8, 64, "fp64"), (3, 128, "fp32")])
def test_mostly_partial_updates(nc, S, prec, monkeypatch):
    """64 events: more than half of the oracle's steps are partial updates, and after most of them the next step of the chain is
    one too -- the step starts from what the one before looked up, and so does the base of the iteration after next."""
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(64, S, nc, 3, 12.0, N_ITER, **kw)
    job, ir = _oracle(data, params, N_ITER)
    part = (ir[:, 7] == 0).reshape(N_ITER, nc)
    assert np.mean(part) > 0.5, "the oracle ran %.1f %% of its steps as partial updates" % (100 * np.mean(part))
    assert np.sum(part[:-1] & part[1:]) > 0.5 * np.sum(part[:-1])
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, prec == "fp32")


@pytest.mark.parametrize("nc,E", [(2, 3), (8, 3), (8, 64)])
def test_rejection_heavy_job_takes_the_rare_path(nc, E, monkeypatch):
    """Depth steps several times the prior's width (tools/stress_rejections.py): the oracle counts at least 50 proposals that the
    Rayleigh prior rejects -- each one a new epoch, which the other waves adopt at the top of a step or in their turn, also while a
    full evaluation's look-ahead is in flight (it is dropped: predicted in another epoch); the step behind an adoption starts from the
    hop tables, not from FlowNext."""
    data, params = _job(E, 64, nc, 3, 12.0, N_ITER)
    job, ir = _oracle(data, params, N_ITER)
    rejected = int(np.sum(ir[:, 5] == 0))
    assert rejected >= 50, "the oracle's priors rejected %d proposals" % rejected
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, False)


@pytest.mark.parametrize("nc,S,E", [(2, 64, 3), (8, 64, 3), (8, 128, 64)])
def test_launches_of_one_iteration_and_their_counters(nc, S, E, monkeypatch):
    """40 launches of one iteration each in a row, between longer launches: the bits of one launch, and the evaluation counters of
    last_run_stats(), summed over the launches, equal the single launch's, which equal what the oracle's step log counts."""
    n_iter = 400
    data, params = _job(E, S, nc, 3, 12.0, n_iter)
    one = _set(monkeypatch, data, params, True)
    one.run(n_iter)
    assert one.fixed_master()
    st = one.last_run_stats()
    ref = _bits(one)
    job, ir = _oracle(data, params, n_iter)
    # (a step whose prior rejects is evaluated by nobody; every other step is counted once, as what it was)
    ok = ir[:, 5] != 0
    assert st["full_evals"] == int(np.sum(ok & (ir[:, 7] != 0))) and st["partial_evals"] == int(np.sum(ok & (ir[:, 7] == 0)))

    cut = _set(monkeypatch, data, params, True)
    full = part = 0
    for n in [3] + [1] * 40 + [n_iter - 43]:
        cut.run(n)
        s = cut.last_run_stats()
        full += s["full_evals"]; part += s["partial_evals"]
    assert cut.fixed_master()
    _assert_same_bits(ref, _bits(cut), "one launch vs launches of one iteration")
    assert (full, part) == (st["full_evals"], st["partial_evals"])
    _assert_oracle(cut, job, n_iter, False)


@pytest.mark.parametrize("nc", [2, 8])
def test_launch_ended_by_chain_0s_wave(nc, monkeypatch):
    """A cool chain that leaves a record every other iteration (n_interval = 2: with 1, `iteration mod n_interval == 1` never holds
    and nothing is recorded) and record buffers of 4 and 3 records per chain: chain 0's wave finds the buffers nearly full at the top
    of a step (stop code 1), the launch ends on its own and the next one goes on -- one run() takes more than one launch; records,
    samples and every counter equal the generic run's, and the oracle's."""
    from oracle import oracle
    from tests.test_gpu_chains import RTOL_TRACE

    n_iter = 600
    data, params = _job(3, 64, nc, 3, 12.0, n_iter, n_interval=2, n_cool=1)
    caps = dict(lik_capacity=4 * nc, sample_capacity=3 * nc)
    fast = _set(monkeypatch, data, params, True, **caps)
    fast.run(n_iter)
    assert fast.fixed_master()
    st = fast.last_run_stats()
    assert st["graph_launches"] > 1, "one run() took %d launch(es)" % st["graph_launches"]
    gen = _set(monkeypatch, data, params, False, **caps)
    gen.run(n_iter)
    assert not gen.fixed_master()
    sg = gen.last_run_stats()
    _assert_same_bits(_bits(fast), _bits(gen), "specialised vs generic")
    assert (st["full_evals"], st["partial_evals"]) == (sg["full_evals"], sg["partial_evals"])

    job = oracle.Job(params, data); job.run(n_iter)
    it, lk = job.likelihood_trace(0)
    gi, _, gl = fast.likelihood_trace()
    assert len(gi) == len(it) == n_iter // 2 and np.array_equal(gi, it)      # (one cool chain, a record every other iteration)
    np.testing.assert_allclose(gl, lk, rtol=RTOL_TRACE)
    assert fast.rng_state() == job.rng_state(0)
    a, b = fast.counts(); oa, ob = job.counts()
    assert np.array_equal(a, oa) and np.array_equal(b, ob)


@pytest.mark.parametrize("nc,temp_high", [(2, 1.00001), (8, 1.001)])
def test_swaps_accepted_often(nc, temp_high, monkeypatch):
    """Temperatures close together (tests/test_gpu_turn_batch.py): between 10 % and 90 % of the oracle's iterations end with a pair
    exchanging its temperatures -- what the commit stores into the rings of T, 1 / T and L changes from iteration to iteration."""
    from oracle import oracle

    data, params = _job(3, 64, nc, 3, 12.0, N_ITER, n_cool=1, temp_high=temp_high)
    job = oracle.Job(params, data)
    job.enable_steplog(N_ITER * nc)
    job.run(N_ITER)
    _, dr = job.steplog()
    T = dr[:, 3].reshape(N_ITER, nc)
    exchanged = float(np.mean(np.any(T[1:] != T[:-1], axis=1)))
    assert 0.10 <= exchanged <= 0.90, "the oracle exchanges temperatures after %.1f %% of the iterations" % (100 * exchanged)
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, False)
    for c in range(nc):
        assert fast.state(c).temp == job.chain(0, c)["temp"]
