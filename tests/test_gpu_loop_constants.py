"""The specialised chain master's loop constants in vector registers (csrc/htm_device.hpp LoopRegs, csrc/htm_flow.hpp flow_body and
flow_step): the ten constants of htm_log and the two lane classes of the transposed wave sum are formed once
per launch and read from registers by the evaluations and by the Rayleigh prior ratio; the proposed position is chosen by scalar
selects.  Every item copies values or performs the same operations on the same operands, so

  the register-constant logarithm equals htm_log bit for bit (self-test mode 7 against mode 0), also where the threshold constant
  decides the branch (the doubles around 2^e sqrt(1/2)), at 0, at the subnormals and at every power of two;
  the class-taking transposed sums equal wave_sum1 value by value (modes 8 and 9 against mode 6);
  a job run specialised, generic (HTM_FAST=0: the literal forms), cut into launches (every launch forms the registers again) and
  from a checkpoint gives the same bits, within the oracle's bounds of tests/test_gpu_fast_master.py.

Shapes, about 1 500 iterations each: 1 event (every hypocentre step hits the event of the step before), 3 events (full evaluations
with an own event: the NPOS = 1 evaluation), 64 events (nearly all partial updates: NPOS = 2); 64 and 128 stations, fp64 and fp32 --
the four kernels k_mcmc<1|2, false|true, 8>; 1, 2, 3 and 8 chains.  Depth steps several times the prior's width run both logarithms
of the Rayleigh prior ratio hundreds of times, and reject.  Conditions on a job are asserted on the ORACLE's step log, on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_fast_master import _assert_oracle, _assert_same_bits, _job, _set  # noqa: F401  (the helpers _four_ways builds on)
from tests.test_gpu_own_state import _bits, _four_ways  # noqa: F401

pytestmark = pytest.mark.gpu

N_ITER = 1500
RT_HALF = 0.70710678118654752      # htm_log's threshold between the two mantissa ranges


def _math(which, x):
    from hypotremormcmc_amd import _lib

    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    _lib.check(_lib.load().htm_selftest_math(0, which, x.ctypes.data_as(_lib.dp), y.ctypes.data_as(_lib.dp), C.c_int(len(x))))
    return y


def _log_arguments():
    tiny = np.finfo(np.float64).tiny
    special = [0.0, 5e-324, float(np.nextafter(tiny, 0.0)), tiny, float(np.finfo(np.float64).max)]
    special += [2.0 ** e for e in range(-1074, 1024)]
    for e in range(-3, 4):
        t = 2.0 ** e * RT_HALF      # (exact: a power of two times the constant)
        special += [float(np.nextafter(t, 0.0)), t, float(np.nextafter(t, np.inf))]
    special = np.array(special)
    rng = np.random.default_rng(20250)
    fill = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), 65536 - len(special)))      # distances, km
    x = np.concatenate([special, fill])
    assert len(x) == 65536
    return x


def test_register_constant_logarithm_equals_htm_log():
    """65 536 arguments: 0, the smallest and the largest subnormal, every power of two, the doubles below, at and above
    2^e sqrt(1/2) for e = -3 .. 3 (where the threshold constant decides the branch), and a seeded log-uniform set over
    [1e-3, 1e4] km.  Bit for bit (-inf at 0 included)."""
    x = _log_arguments()
    ref, got = _math(0, x), _math(7, x)
    assert ref[0] == -np.inf and np.all(np.isfinite(ref[1:]))
    # (the thresholds are really straddled: the mantissa of the value below is under the constant, of the value at it is not)
    m = np.frexp(np.array([np.nextafter(RT_HALF, 0.0), RT_HALF]))[0]
    assert m[0] < RT_HALF <= m[1]
    bad = np.flatnonzero(ref.view(np.int64) != got.view(np.int64))
    assert len(bad) == 0, "%d arguments differ, the first: x = %r: %r (registers) vs %r" % (len(bad), x[bad[0]], got[bad[0]], ref[bad[0]])


@pytest.mark.parametrize("mode", [8, 9])
def test_class_taking_transposed_sums_equal_wave_sum1(mode):
    """1 000 seeded waves, four values per lane, magnitudes from 1e-8 to 1e8 and both signs: wave_sum_transposed<4> (mode 8) and
    wave_sum_transposed<2> on the two pairs (mode 9), lane classes from registers, against wave_sum1 value by value (mode 6)."""
    rng = np.random.default_rng(77)
    n = 4 * 64 * 1000
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-8.0, 8.0, n)
    assert np.mean(x < 0) > 0.4 and np.mean(x > 0) > 0.4
    ref, got = _math(6, x), _math(mode, x)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(ref.view(np.int64), got.view(np.int64))
    # (every lane of a wave holds its wave's sum, and the sum is the values' sum to rounding)
    w = ref[:n // 4].reshape(1000, 64)
    assert np.all(w == w[:, :1])
    xs = x[:n // 4].reshape(1000, 64)
    # (63 additions each way, each within eps / 2 of a partial sum no larger than sum |x|: 64 eps sum |x| covers both sides' error)
    assert np.all(np.abs(w[:, 0] - xs.sum(axis=1)) <= 64 * np.finfo(np.float64).eps * np.abs(xs).sum(axis=1))


def _oracle(data, params, n_iter):
    """the oracle's run with its step log: (job, ir), ir = iter, rank, chain, type, index (1-based), prior ok, accepted, full evaluation"""
    from oracle import oracle

    nc = int(params["n_chains"])
    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data)
    job.enable_steplog(n_iter * nc)
    job.run(n_iter)
    ir, _ = job.steplog()
    assert len(ir) == n_iter * nc
    return job, ir


@pytest.mark.parametrize("nc,S,prec,E", [(1, 64, "fp64", 1), (8, 64, "fp64", 3), (3, 64, "fp32", 3), (2, 128, "fp64", 1),
                                         (8, 128, "fp32", 3), (8, 64, "fp64", 64)])
def test_four_ways_same_bits_and_oracle(nc, S, prec, E, monkeypatch):
    """One job run specialised in one launch, generic, cut into launches (1, 7, 400, 13, the rest) and continued from a checkpoint:
    numpy.array_equal among themselves; the specialised run within the oracle's bounds.  3 events: the oracle runs full evaluations
    behind a hypocentre step of the same chain (the own-event evaluation); 64 events: most steps are partial updates."""
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(E, S, nc, 3, 12.0, N_ITER, **kw)
    job, ir = _oracle(data, params, N_ITER)
    full = (ir[:, 7] != 0).reshape(N_ITER, nc)
    hyp = (ir[:, 3] >= 5).reshape(N_ITER, nc)
    if E == 3:
        own = int(np.sum(hyp[1:-1] & full[2:]))      # (iteration 1 is all full evaluations, the partial updates start at 2)
        assert own >= 50, "full evaluations behind a hypocentre step of their chain: %d" % own
    if E == 64:
        assert np.mean(~full) > 0.5
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, prec == "fp32")


@pytest.mark.parametrize("nc,S,prec", [(8, 64, "fp64"), (2, 128, "fp32")])
def test_wide_depth_steps_run_both_logarithms_of_the_prior_ratio(nc, S, prec, monkeypatch):
    """Depth steps of 20 km against a prior a few km wide (tools/stress_rejections.py's widest): on the oracle's step log at least
    200 depth proposals pass the Rayleigh prior -- each one takes log(x_new - mu) - log(x_old - mu) -- and at least 50 are rejected
    by it.  Four ways as above."""
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(3, S, nc, 4, 20.0, N_ITER, **kw)
    job, ir = _oracle(data, params, N_ITER)
    depth = (ir[:, 3] >= 5) & (ir[:, 4] % 3 == 0)      # (1-based element 3 i of the hypocentre vector: driver.py gives it prior type 1)
    passed, rejected = int(np.sum(depth & (ir[:, 5] != 0))), int(np.sum(depth & (ir[:, 5] == 0)))
    assert int(np.sum(~depth & (ir[:, 5] == 0))) == 0, "only the depth's prior rejects"
    assert passed >= 200 and rejected >= 50, "depth proposals that passed the Rayleigh prior: %d, rejected: %d" % (passed, rejected)
    fast = _four_ways(data, params, nc, N_ITER, monkeypatch)
    _assert_oracle(fast, job, N_ITER, prec == "fp32")
