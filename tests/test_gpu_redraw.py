"""The swap pair's redraw fallback in every chain loop.  select_pair (src/cls_parallel.f90:226-230) redraws i2 until it differs from
i1; the stream service precomputes the pair for up to 12 redraws (k_stream_rec, csrc/htm_chains_kernels.hpp) and every loop
follows the stream itself beyond that -- swap_plan and role P's bet (htm_step.hpp), both branches of flow_swap_at and the
look-ahead (htm_flow.hpp), the pipelined master's front (htm_pipe.hpp) -- each with its own count of the draws the pair took and
of whether the judge draw is this rank's.  A miscount shifts the rank's stream by one position and nothing crashes.

Each test runs a job of tests/redraw_cases.py (two chains in the job, the event at a known iteration, 100 iterations behind it;
tests/test_redraw_cases.py proves the event on the CPU) on the loop it names, asserts that this loop ran, and compares with the
oracle by the criteria of tests/test_gpu_chains.py and tests/test_gpu_fast_master.py.

How the loops are reached: LocalWorld drives step_begin / step_end, one launch per iteration (the k_mcmc instantiation 1, or
k_step + k_full with HTM_PERSIST=0) whatever HTM_FLOW_LOCK / HTM_PIPE_LOCK say; the persistent lock-step loops (2, 4, 6) run only
under htm_chains_run_lockstep_direct, i.e. TorchWorld over the in-kernel exchange.  With one rank that is a process group of one
in this process; with two ranks it takes two processes, which one test starts for all three loops and both two-rank cases.

Out of scope, because the fallback cannot be reached there without a knob that changes product behaviour: two master workgroups
(9-16 chains) and the wide loop (33+ chains) -- with three or more chains in the job the event has probability 3^-12 per
iteration and less; the multi-process transports as such, which only carry records; the ring wrap-around."""
import os
import socket
import sys

import numpy as np
import pytest

from tests import redraw_cases as rc
from tests.test_gpu_chains import RTOL_TRACE, _build_world
from tests.test_gpu_fast_master import RTOL_FP32, _assert_same_bits, _bits, _set

pytestmark = pytest.mark.gpu

TWO_RANK_CASES = ("ranks2_judge0", "ranks2_judge1")
# knob -> the loop htm_chains_run_lockstep_direct then runs (htm_plan.hpp loop_for)
LOCKRUN_LOOPS = ((None, 4), ("HTM_FLOW_LOCK=0", 2), ("HTM_PIPE_LOCK=1", 6))


def _build(name, **kw):
    data, params, n_iter, k = rc.build(name)
    return data, dict(params, **kw), n_iter, k


def _differences(sets, name, fp32=False):
    """what tests/test_gpu_chains.py compares with the oracle, for the ranks in `sets` ({rank: chain set}): a list of findings"""
    job = rc.oracle_run(name)
    bad = []
    for r, cs in sets.items():
        it, lk = job.likelihood_trace(r)
        gi, _, gl = cs.likelihood_trace()
        if not (len(gi) == len(it) > 20 and np.array_equal(gi, it)):
            bad.append("rank %d: recorded iterations differ (%d records, the oracle has %d)" % (r, len(gi), len(it)))
        elif not np.allclose(gl, lk, rtol=RTOL_FP32 if fp32 else RTOL_TRACE, atol=0):
            bad.append("rank %d: log-likelihoods differ, from record %d on" % (r, int(np.argmax(~np.isclose(gl, lk, rtol=RTOL_FP32 if fp32 else RTOL_TRACE, atol=0)))))
        if cs.rng_state() != job.rng_state(r):
            bad.append("rank %d: rng_state differs" % r)
        for c in range(cs.n_chains):
            s, o = cs.state(c), job.chain(r, c)
            if not (np.array_equal(s.n_propose, o["n_propose"]) and np.array_equal(s.n_accept, o["n_accept"])):
                bad.append("rank %d chain %d: proposal / accept counters differ" % (r, c))
            if not np.allclose(s.hypo, o["hypo"], rtol=1e-11, atol=1e-12):
                bad.append("rank %d chain %d: hypo differs" % (r, c))
            if not np.allclose(s.t_corr, o["t_corr"], rtol=1e-11, atol=1e-13):
                bad.append("rank %d chain %d: t_corr differs" % (r, c))
            if s.temp != o["temp"]:
                bad.append("rank %d chain %d: temperature %r, the oracle has %r" % (r, c, s.temp, o["temp"]))
    return bad


def _assert_oracle(sets, name, fp32=False):
    bad = _differences(sets if isinstance(sets, dict) else {0: sets}, name, fp32)
    assert not bad, "%s: %s" % (name, "; ".join(bad))


def _assert_steplog_from_the_event(cs, name, k):
    """step-log columns 2-6 (type, index, prior_ok, accepted, full / partial) and the temperatures, from the event to the end"""
    oi, od = rc.oracle_run(name).steplog()
    gi, gd = cs.steplog()
    assert len(gi) == len(oi) and np.array_equal(gi[:, 0], oi[:, 0]) and np.array_equal(gi[:, 1], oi[:, 2])
    late = oi[:, 0] >= k
    assert late.sum() == 2 * 101
    assert np.array_equal(gi[late, 2:7], oi[late, 3:8])
    assert np.array_equal(gd[late, 3], od[late, 3])


def _one_launch(monkeypatch, name, fast=True, steplog=False, **kw):
    data, params, n_iter, k = _build(name, **kw)
    cs = _set(monkeypatch, data, params, fast)
    if steplog:
        cs.enable_steplog(2 * n_iter)
    cs.run(n_iter)
    return cs


# ---- single rank, one launch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_free_running_master_specialised_and_generic(prec, monkeypatch):
    """64 stations, both data types: the specialised instantiation and the generic one (HTM_FAST=0) pass the event with the same
    bits, and equal the oracle -- with the fp64 and with the fp32 forward"""
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    fast = _one_launch(monkeypatch, "spec64", True, **kw)
    assert fast.master_stats()["single_rank_loop"] == 3 and fast.fixed_master(), "the specialised instantiation was not selected"
    gen = _one_launch(monkeypatch, "spec64", False, **kw)
    assert gen.master_stats()["single_rank_loop"] == 3 and not gen.fixed_master(), "HTM_FAST=0 did not force the generic instantiation"
    _assert_same_bits(_bits(fast), _bits(gen), "specialised vs generic")
    _assert_oracle(fast, "spec64", prec == "fp32")


@pytest.mark.parametrize("name", ["spec64", "ragged70"])
def test_free_running_master_generic_step_by_step(name, monkeypatch):
    """the generic instantiation with the step log on, at 64 stations and at 70 (two per lane, a ragged row)"""
    k = rc.CASES[name][7]
    cs = _one_launch(monkeypatch, name, True, steplog=True)
    assert cs.master_stats()["single_rank_loop"] == 3 and not cs.fixed_master()
    _assert_oracle(cs, name)
    _assert_steplog_from_the_event(cs, name, k)


def test_free_running_master_at_70_stations(monkeypatch):
    cs = _one_launch(monkeypatch, "ragged70", True)
    assert cs.master_stats()["single_rank_loop"] == 3 and not cs.fixed_master()
    _assert_oracle(cs, "ragged70")


@pytest.mark.parametrize("name", ["spec64", "ragged70"])
@pytest.mark.parametrize("knob,loop", [("HTM_FLOW=0", 0), ("HTM_PERSIST=0", -1), ("HTM_PIPE=1", 5)])
def test_other_single_rank_loops(knob, loop, name, monkeypatch):
    """the loop with barriers (swap_plan, role P's bet), the two-kernel path and the pipelined master's front"""
    monkeypatch.setenv(*knob.split("="))
    steplog = loop in (0, 5)
    cs = _one_launch(monkeypatch, name, True, steplog=steplog)
    assert cs.master_stats()["single_rank_loop"] == loop, "%s did not select loop %d" % (knob, loop)
    _assert_oracle(cs, name)
    if steplog:
        _assert_steplog_from_the_event(cs, name, rc.CASES[name][7])


# ---- single rank, the event at a launch boundary ----------------------------------------------------------------------------------

@pytest.mark.parametrize("which,loop", [("specialised", 3), ("generic", 3), ("HTM_FLOW=0", 0), ("HTM_PIPE=1", 5)])
def test_event_at_launch_boundaries(which, loop, monkeypatch):
    """run(k - 2), run(1), run(1), run(1), run(rest): the event's swap is the last thing of one launch and the look-ahead of the
    launches before it.  The same bits as the run in one launch."""
    if "=" in which:
        monkeypatch.setenv(*which.split("="))
    data, params, n_iter, k = _build("spec64")
    fast = which != "generic"
    one = _set(monkeypatch, data, params, fast)
    one.run(n_iter)
    assert one.master_stats()["single_rank_loop"] == loop and one.fixed_master() == (which == "specialised")
    cut = _set(monkeypatch, data, params, fast)
    for n in (k - 2, 1, 1, 1, n_iter - k - 1):
        cut.run(n)
    assert cut.iterations_done == n_iter and cut.fixed_master() == (which == "specialised")
    _assert_same_bits(_bits(one), _bits(cut), "%s: one launch vs launches that end around iteration %d" % (which, k))
    _assert_oracle(cut, "spec64")


def test_checkpoint_right_before_the_event(monkeypatch):
    """a checkpoint saved after iteration k - 1 and loaded into a fresh chain set: the specialised master's first iteration is the event"""
    data, params, n_iter, k = _build("spec64")
    ref = _bits(_one_launch(monkeypatch, "spec64", True))
    first = _set(monkeypatch, data, params, True)
    first.run(k - 1)
    blob = first.checkpoint()
    cont = _set(monkeypatch, data, params, True)
    cont.restore(blob)
    assert cont.iterations_done == k - 1
    cont.run(n_iter - (k - 1))
    assert cont.fixed_master()
    b = _bits(cont)
    keep = ref["lik_iter"] > k - 1
    assert np.array_equal(ref["lik_iter"][keep], b["lik_iter"]) and np.array_equal(ref["lik"][keep], b["lik"])
    for key in ref:
        if key.startswith(("rng", "n_", "hypo_", "t_corr_", "TL_")):
            assert np.array_equal(ref[key], b[key]), "continued from the checkpoint: %s differs" % key


# ---- lock-step, one launch per iteration (step_begin / step_end) -------------------------------------------------------------------

def test_lockstep_driver_of_one_rank_equals_run(monkeypatch):
    """n_procs = 1 through LocalWorld: as test_lockstep_equals_single_rank_driver compares the two, here across the event"""
    from hypotremormcmc_amd.parallel import LocalWorld

    data, params, n_iter, k = _build("spec64")
    a = _one_launch(monkeypatch, "spec64", True)
    _, b = _build_world(data, params)
    LocalWorld(b).run(n_iter)
    ia, ca, la = a.likelihood_trace(); ib, cb, lb = b[0].likelihood_trace()
    assert np.array_equal(ia, ib)
    np.testing.assert_allclose(la, lb, rtol=1e-13, atol=0)
    assert a.rng_state() == b[0].rng_state()
    for c in range(2):
        assert np.array_equal(a.state(c).hypo, b[0].state(c).hypo)
        assert np.array_equal(a.state(c).n_accept, b[0].state(c).n_accept)
        assert a.state(c).temp == b[0].state(c).temp
    _assert_oracle(b[0], "spec64")


@pytest.mark.parametrize("name", TWO_RANK_CASES)
@pytest.mark.parametrize("persist", ["1", "0"])
def test_lockstep_driver_of_two_ranks(persist, name, monkeypatch):
    """two ranks of one chain through LocalWorld: rank 0 draws the pair; the judge draw is rank 0's (i1 = 0) or rank 1's (i1 = 1:
    rank 0 draws nothing else).  One k_mcmc launch per iteration, or k_step + k_full + k_step with HTM_PERSIST=0."""
    from hypotremormcmc_amd.parallel import LocalWorld

    monkeypatch.setenv("HTM_PERSIST", persist)
    data, params, n_iter, k = _build(name)
    _, sets = _build_world(data, params)
    for cs in sets:
        assert (cs.master_stats()["single_rank_loop"] == -1) == (persist == "0")
    LocalWorld(sets).run(n_iter)
    _assert_oracle(dict(enumerate(sets)), name)


# ---- persistent lock-step (htm_chains_run_lockstep_direct) -------------------------------------------------------------------------

@pytest.mark.parametrize("knob,loop", LOCKRUN_LOOPS)
def test_persistent_lockstep_rank_alone(knob, loop, monkeypatch):
    """one rank of two chains through MODE_LOCKRUN (a process group of one, the in-kernel exchange): the lock-step branch of
    flow_swap_at, swap_plan with lockstep set, the pipelined master's lock-step front -- equal to run() as
    test_rccl_lockstep_loop_equals_single_rank_driver compares them, and to the oracle"""
    import torch
    import torch.distributed as dist

    from hypotremormcmc_amd.parallel import TorchWorld

    monkeypatch.setenv("HTM_XCHG", "1")
    a = _one_launch(monkeypatch, "spec64", True)
    if knob:
        monkeypatch.setenv(*knob.split("="))
    data, params, n_iter, k = _build("spec64")
    _, b = _build_world(data, params)
    assert b[0].master_stats()["lockstep_loop"] == loop
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group(backend="nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        tw = TorchWorld(b[0])
        assert tw.direct, "the in-kernel exchange was not set up"
        tw.run(k - 1)           # (the event is the first iteration of the second launch)
        tw.run(n_iter - (k - 1))
        torch.cuda.synchronize()
        assert tw.fell_back is None
    finally:
        dist.destroy_process_group()
    assert b[0].iterations_done == n_iter
    ia, ca, la = a.likelihood_trace(); ib, cb, lb = b[0].likelihood_trace()
    assert np.array_equal(ia, ib)
    np.testing.assert_allclose(la, lb, rtol=1e-12 if loop == 6 else 1e-13, atol=0)      # (tests/test_gpu_pipe.py: 1e-12 for the pipelined master)
    assert a.rng_state() == b[0].rng_state()
    for c in range(2):
        assert np.array_equal(a.state(c).hypo, b[0].state(c).hypo)
        assert a.state(c).temp == b[0].state(c).temp
    _assert_oracle(b[0], "spec64")


def _two_rank_worker(rank, port, q):
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", HTM_XCHG="1")
    import torch.distributed as dist

    from hypotremormcmc_amd import driver
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.parallel import TorchWorld

    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        for knob, loop in LOCKRUN_LOOPS:
            for key in ("HTM_FLOW_LOCK", "HTM_PIPE_LOCK"):
                os.environ.pop(key, None)
            if knob:
                os.environ.update([knob.split("=")])
            for name in TWO_RANK_CASES:
                data, params, n_iter, k = rc.build(name)
                obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
                fwd, cs = driver.build_rank(params, data.sta_x, data.sta_y, data.sta_z, obs, rank, n_procs=2, device=0)
                bad = []
                if cs.master_stats()["lockstep_loop"] != loop:
                    bad.append("loop %d selected" % cs.master_stats()["lockstep_loop"])
                tw = TorchWorld(cs)
                if not tw.direct:
                    bad.append("the in-kernel exchange was not set up")
                tw.run(k - 1)
                tw.run(n_iter - (k - 1))
                if tw.fell_back is not None:
                    bad.append(tw.fell_back)
                bad += _differences({rank: cs}, name)
                q.put((rank, loop, name, bad))
                del tw, cs, fwd
    finally:
        dist.destroy_process_group()


def test_persistent_lockstep_two_ranks_in_two_processes():
    """Two ranks of one chain on the persistent lock-step loops -- the free-running master (4), the loop with barriers (2,
    HTM_FLOW_LOCK=0), the pipelined master (6, HTM_PIPE_LOCK=1) -- on both two-rank cases: the judge draw on rank 0, and on rank 1,
    where rank 0's count of its own draws must leave the judge draw out
    (nd = ... + ((!rg.lock || i1 / n_chains == 0) ? 1 : 0)) and rank 1 loses its bet that the pair's first chain is not its own.
    These loops exchange the swap records inside the launch, so two ranks take two processes (sharing the GPU, as
    test_torchworld_across_processes_sharing_the_gpu arranges them): one pair of processes runs all six jobs."""
    import queue
    import time

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    want = 2 * len(LOCKRUN_LOOPS) * len(TWO_RANK_CASES)
    res, t_end = [], time.time() + 240
    while len(res) < want and time.time() < t_end:
        try:
            res.append(q.get(timeout=2))
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):      # a rank died: do not wait for its answers
                break
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
        assert p.exitcode == 0
    assert len(res) == want, res
    assert not [r for r in res if r[3]], [r for r in res if r[3]]
