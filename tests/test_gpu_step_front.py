"""The front of the specialised chain master's step (csrc/htm_flow.hpp flow_step under FlowFixed): the event's
observations from one packed record (FwdDev::obs_pack), the launch constants from one batch of scalar loads, the perturbed
element's offset by arithmetic on the proposal type, the gather index from the lane id -- at the shapes where that addressing
can go wrong: the first and the last record (1, 2, 3 events), both record strides and element types (64 / 128 stations,
fp64 / fp32 forward), offsets that are no powers of two (5 chains).

None of it changes a rounding, so the specialised run equals the generic instantiation (HTM_FAST=0: same source, run-time
answers) bit for bit; against the oracle the bounds of tests/test_gpu_fast_master.py hold."""
import numpy as np
import pytest

from tests.test_gpu_fast_master import _assert_oracle, _assert_same_bits, _bits, _job, _set

pytestmark = pytest.mark.gpu

N_ITER = 400


def _pack_bytes(E, S, fp32):
    """one record per event: four rows and two doubles, padded to a multiple of 64 bytes"""
    return E * ((4 * S * (4 if fp32 else 8) + 16 + 63) // 64 * 64)


@pytest.mark.parametrize("nc", [1, 5, 8])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("E", [1, 2, 3])
def test_front_addressing_equals_generic_and_oracle(E, S, prec, nc, monkeypatch):
    """A rejection-heavy job with records on, once specialised and once generic: traces, samples, counters, chain states and
    the RNG state are the same bits; the specialised run equals the oracle.  Every proposal type and every coordinate has
    occurred (proposal counters), so the element offset of every type was exercised."""
    from oracle import oracle

    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(E, S, nc, 3, 12.0, N_ITER, **kw)
    fast = _set(monkeypatch, data, params, True)
    assert fast.master_stats()["single_rank_loop"] == 3
    fast.run(N_ITER)
    assert fast.fixed_master(), "the specialised instantiation was not selected"
    assert fast.fwd.obs_pack_bytes() == _pack_bytes(E, S, prec == "fp32")
    ref = _bits(fast)
    n_propose = np.asarray(ref["n_propose"])
    assert n_propose.shape[-1] == 7 and np.all(n_propose.reshape(-1, 7).sum(axis=0) > 0), \
        "a proposal type (vs, t_corr, qs, a_corr, x, y, z) did not occur: %s" % n_propose

    gen = _set(monkeypatch, data, params, False)
    assert gen.master_stats()["single_rank_loop"] == 3
    gen.run(N_ITER)
    assert not gen.fixed_master(), "HTM_FAST=0 did not force the generic instantiation"
    assert gen.fwd.obs_pack_bytes() == 0, "the generic master does not read packed records: none are built for it"
    _assert_same_bits(ref, _bits(gen), "specialised vs generic")

    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data); job.run(N_ITER)
    _assert_oracle(fast, job, N_ITER, prec == "fp32")


@pytest.mark.parametrize("case", ["60 stations", "use_amp = F"])
def test_other_shapes_build_no_packed_records(case, monkeypatch):
    """rows that are not full, or one data type only: the generic master runs, no packed records are allocated, and the run
    equals the oracle"""
    from oracle import oracle

    S, kw = (60, {}) if case == "60 stations" else (64, dict(use_amp="F"))
    data, params = _job(3, S, 5, 1, 12.0, N_ITER, **kw)
    cs = _set(monkeypatch, data, params, True)
    assert cs.master_stats()["single_rank_loop"] == 3
    cs.run(N_ITER)
    assert not cs.fixed_master(), "%s: the specialised instantiation must not run" % case
    assert cs.fwd.obs_pack_bytes() == 0, "%s: packed records were allocated" % case
    job = oracle.Job(params, data); job.run(N_ITER)
    _assert_oracle(cs, job, N_ITER, False)
