"""The specialised chain master from its turn to its decision (csrc/htm_flow.hpp FlowTurn): what a step reads
from LDS between its evaluation and its Metropolis decision -- the other chains' checks and the epoch, its own temperature of the
iteration before, the plan of that iteration's swap, every chain's committed key and (T, 1/T, L) -- is requested in one batch with
every poll of the turn; FlowShared::i0 and the launch's target come with the batch at the loop top.  The same words are read and
the same values compared, added and stored as in the generic instantiation (HTM_FAST=0), so every comparison with it is
numpy.array_equal; against the oracle the bounds of tests/test_gpu_fast_master.py hold.

Where this code can go wrong, and the smallest shapes that reach it (1 or 3 events, 1500 iterations):
  1 chain: no swap block at all; 2 chains: every step is one of the pair and the partner is always the other wave (the partner's
  record from the batch, or -- the partner not yet committed -- from the spin); 3 chains: the pair's path two times in three;
  8 chains: the shape bench.py runs.  64 stations (the corrections in registers) and 128 (two stations per lane), fp64 and fp32.
  Launches of ONE iteration: every step is "the first iteration of a launch", which reads the prologue's temperature and no plan.
  Swaps that are accepted often (the select of the partner's temperature, the exchanged pair committed) and almost never.
  Prior rejections: epochs change while turns poll, and batches are dropped with their round.
Conditions on a job (how often temperatures are exchanged, how many priors reject) are asserted on the ORACLE's step log."""
import numpy as np
import pytest

from tests.test_gpu_fast_master import _assert_oracle, _assert_same_bits, _job, _set
from tests.test_gpu_own_state import _bits, _four_ways

pytestmark = pytest.mark.gpu

N_ITER = 1500


def _oracle(data, params, n_iter):
    """the oracle's run with its step log: (job, fraction of iterations after which some chain's temperature differs from the one
    it had the iteration before, number of proposals the prior rejected)"""
    from oracle import oracle

    nc = int(params["n_chains"])
    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data)
    job.enable_steplog(n_iter * nc)
    job.run(n_iter)
    ir, dr = job.steplog()      # rows in (iteration, chain) order: ir = iter, rank, chain, type, index, prior ok, accepted, full; dr[3] = T
    assert len(ir) == n_iter * nc and np.array_equal(ir[:nc, 2], np.arange(nc))
    T = dr[:, 3].reshape(n_iter, nc)
    exchanged = float(np.mean(np.any(T[1:] != T[:-1], axis=1)))
    return job, exchanged, int(np.sum(ir[:, 5] == 0))


# every value of (stations, precision) at 2 and at 8 chains, the bench's shape, and 1 and 3 chains
@pytest.mark.parametrize("nc,S,prec", [(1, 64, "fp64"), (2, 64, "fp64"), (2, 128, "fp32"), (3, 64, "fp32"), (3, 128, "fp64"),
                                       (8, 64, "fp64"), (8, 64, "fp32"), (8, 128, "fp64")])
def test_batched_turn_equals_generic_and_oracle(nc, S, prec, monkeypatch):
    """One job with records on, run four ways -- specialised in one launch, generic, cut into launches (1, 7, 400, 13, the rest),
    continued from a checkpoint: the same bits; the specialised run equals the oracle."""
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(3, S, nc, 3, 12.0, N_ITER, **kw)
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    job, _, _ = _oracle(data, params, N_ITER)
    _assert_oracle(fast, job, N_ITER, prec == "fp32")


@pytest.mark.parametrize("nc,S", [(2, 64), (8, 64), (8, 128)])
def test_launches_of_one_iteration(nc, S, monkeypatch):
    """40 launches of one iteration each in a row (every step: the first iteration of its launch, the swap of the iteration
    before applied by the launch before), between longer launches: the bits of one launch."""
    n_iter = 400
    data, params = _job(3, S, nc, 3, 12.0, n_iter)
    one = _set(monkeypatch, data, params, True)
    one.run(n_iter)
    assert one.fixed_master()
    ref = _bits(one)
    cut = _set(monkeypatch, data, params, True)
    cut.run(3)
    for _ in range(40):
        cut.run(1)
    cut.run(n_iter - 43)
    assert cut.fixed_master()
    _assert_same_bits(ref, _bits(cut), "one launch vs launches of one iteration")
    job, _, _ = _oracle(data, params, n_iter)
    _assert_oracle(cut, job, n_iter, False)


# (one cool chain, so that two chains have two temperatures; the ladder's top chosen on the CPU from the oracle's step log)
@pytest.mark.parametrize("nc,temp_high,often", [(2, 1.00001, True), (8, 1.001, True), (2, 200.0, False), (3, 200.0, False)])
def test_swaps_accepted_often_and_almost_never(nc, temp_high, often, monkeypatch):
    """Temperatures close together: between 10 % and 90 % of the iterations end with a pair exchanging its temperatures (the
    decision's select, and the pair's path that commits the partner's temperature); far apart: under 2 % do (the pair's path
    that keeps its own)."""
    data, params = _job(3, 64, nc, 3, 12.0, N_ITER, n_cool=1, temp_high=temp_high)
    job, exchanged, _ = _oracle(data, params, N_ITER)
    if often:
        assert 0.10 <= exchanged <= 0.90, "the oracle exchanges temperatures after %.1f %% of the iterations" % (100 * exchanged)
    else:
        assert exchanged < 0.02, "the oracle exchanges temperatures after %.1f %% of the iterations" % (100 * exchanged)
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, False)
    # the temperatures every chain ends with (the swap of the last iteration included)
    for c in range(nc):
        assert fast.state(c).temp == job.chain(0, c)["temp"]


@pytest.mark.parametrize("nc", [2, 8])
def test_rejection_heavy_job_drops_batches(nc, monkeypatch):
    """Depth steps several times the prior's width (tools/stress_rejections.py): the oracle counts at least 50 proposals that the
    Rayleigh prior rejects -- each one a new epoch that the other waves adopt at the top of a step or in their turn, where the
    round's batch is dropped and read again."""
    data, params = _job(3, 64, nc, 3, 12.0, N_ITER)
    job, _, rejected = _oracle(data, params, N_ITER)
    assert rejected >= 50, "the oracle's priors rejected %d proposals" % rejected
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, False)
