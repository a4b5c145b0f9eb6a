"""The specialised chain master with the chain count and the stream window's ring as compile-time constants (k_mcmc_sized:
csrc/htm_flow.hpp FlowSized<8, 512>) against the same master with run-time sizes (HTM_SIZED=0), against the
generic instantiation (HTM_FAST=0) and against the oracle.

The constants replace loads, address arithmetic and multiplications by values the job fixes; the arithmetic of the model, the
LDS words and the order of every operation are the same, so every comparison between the three instantiations is
numpy.array_equal.  The comparisons with the oracle are those of tests/test_gpu_fast_master.py, whose job builder and
comparisons are used here.  Which instantiation ran is asserted through ChainSet.sized_master() / fixed_master()."""
import numpy as np
import pytest

from tests.test_gpu_fast_master import _assert_oracle, _assert_same_bits, _bits, _job
from tests.test_gpu_chains import _build_world

SIZED = (8, 512)      # the literals of the one sized instantiation: eight chains on a ring of 512 positions


def _set(monkeypatch, data, params, which, **caps):
    """which: 'sized' (nothing set), 'unsized' (HTM_SIZED=0: k_mcmc<.., 8>), 'generic' (HTM_FAST=0: k_mcmc<.., 3>)"""
    monkeypatch.delenv("HTM_FAST", raising=False)
    monkeypatch.delenv("HTM_SIZED", raising=False)
    if which == "unsized":
        monkeypatch.setenv("HTM_SIZED", "0")
    elif which == "generic":
        monkeypatch.setenv("HTM_FAST", "0")
    else:
        assert which == "sized"
    _, sets = _build_world(data, params, **caps)
    return sets[0]


def _oracle(params, data, n_iter):
    from oracle import oracle

    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data); job.run(n_iter)
    return job


def _three_ways(monkeypatch, data, params, n_iter, fp32):
    """the job on the sized master, on the specialised master with run-time sizes and on the generic one: the same bits, each
    reporting what it ran; the sized run against the oracle step for step (counters, RNG state, every recorded likelihood)"""
    sized = _set(monkeypatch, data, params, "sized")
    assert sized.master_stats()["single_rank_loop"] == 3 and sized.plan()[0]["ring_size"] == 512
    assert sized.sized_master() == (0, 0), "nothing has been launched yet"
    sized.run(n_iter)
    assert sized.sized_master() == SIZED, "the sized instantiation was not selected"
    assert sized.fixed_master(), "fixed_master() is true for both fixed kinds"
    ref = _bits(sized)

    unsized = _set(monkeypatch, data, params, "unsized")
    unsized.run(n_iter)
    assert unsized.sized_master() == (0, 0) and unsized.fixed_master(), "HTM_SIZED=0 did not keep the sized instantiation out"
    _assert_same_bits(ref, _bits(unsized), "sized vs HTM_SIZED=0")

    gen = _set(monkeypatch, data, params, "generic")
    gen.run(n_iter)
    assert gen.sized_master() == (0, 0) and not gen.fixed_master(), "HTM_FAST=0 did not force the generic instantiation"
    _assert_same_bits(ref, _bits(gen), "sized vs HTM_FAST=0")

    _assert_oracle(sized, _oracle(params, data, n_iter), n_iter, fp32)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("E", [3, 64])
def test_sized_master_same_bits_three_ways(E, S, prec, monkeypatch):
    """8 chains; 3 events (every event's step comes round often, full evaluations of a nearly empty worker fleet) and 64; one and
    two stations per lane; both forward precisions.  (The fp32 forward is compared with the fp64 oracle at the bound of
    tests/test_gpu_fp32.py T1, as tests/test_gpu_fast_master.py does.)"""
    n_iter = 4000 if E == 3 else 2000
    kw = dict(forward_precision="fp32") if prec == "fp32" else {}
    data, params = _job(E, S, 8, 3, 12.0, n_iter, **kw)
    _three_ways(monkeypatch, data, params, n_iter, prec == "fp32")


@pytest.mark.gpu
def test_sized_master_rejection_heavy(monkeypatch):
    """Depth steps of five times the prior's width (the stress job's largest, tools/stress_rejections.py): Rayleigh-prior rejections
    every few steps, so the chain waves publish anchors, adopt epochs and void their order books all the time -- the paths on which the
    sized master's one test at the loop top is not hot and the checks behind it run.  3 events: nearly every hypocentre step is a
    depth step of one of them."""
    n_iter = 4000
    data, params = _job(3, 64, 8, 4, 20.0, n_iter)
    _three_ways(monkeypatch, data, params, n_iter, False)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 128])
def test_sized_master_cut_into_launches_and_from_a_checkpoint(S, monkeypatch):
    """one launch, several launches of odd lengths with tiny record buffers (every launch carves the LDS and seeds the window
    again) and a run continued from a checkpoint: the same bits, the sized kernel in every part"""
    n_iter = 2000
    data, params = _job(64, S, 8, 3, 12.0, n_iter)
    one = _set(monkeypatch, data, params, "sized")
    one.run(n_iter)
    assert one.sized_master() == SIZED
    ref = _bits(one)

    nc = 8
    cut = _set(monkeypatch, data, params, "sized", lik_capacity=4 * nc, sample_capacity=3 * nc)
    done = 0
    for n in (1, 7, 400, 13, 2, 900):
        cut.run(n); done += n
        assert cut.sized_master() == SIZED and cut.iterations_done == done
    cut.run(n_iter - done)
    assert cut.sized_master() == SIZED
    _assert_same_bits(ref, _bits(cut), "one launch vs several")

    first = _set(monkeypatch, data, params, "sized")
    first.run(700)
    assert first.sized_master() == SIZED
    blob = first.checkpoint()
    cont = _set(monkeypatch, data, params, "sized")
    cont.restore(blob)
    cont.run(n_iter - 700)
    assert cont.sized_master() == SIZED
    b = _bits(cont)
    keep = ref["lik_iter"] > 700
    assert np.array_equal(ref["lik_iter"][keep], b["lik_iter"]) and np.array_equal(ref["lik_chain"][keep], b["lik_chain"])
    assert np.array_equal(ref["lik"][keep], b["lik"])
    for k in ref:
        if k.startswith(("rng", "n_", "hypo_", "t_corr_", "TL_")):
            assert np.array_equal(ref[k], b[k]), "continued from a checkpoint: %s differs" % k


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["7 chains", "4 chains", "2 chains", "step log", "HTM_FAST=0", "HTM_SIZED=0"])
def test_sized_master_is_not_selected(case, monkeypatch):
    """a launch with other sizes than the literals, a loop other than 8, or the switch: the kernels of before, the oracle's steps.
    7 and 4 chains are planned with the ring of 512 and are not eight chains; 2 chains are planned with a ring of 256."""
    n_iter = 2000
    nc = {"7 chains": 7, "4 chains": 4, "2 chains": 2}.get(case, 8)
    data, params = _job(64, 64, nc, 1, 4.0, n_iter)
    cs = _set(monkeypatch, data, params, {"HTM_FAST=0": "generic", "HTM_SIZED=0": "unsized"}.get(case, "sized"))
    assert cs.master_stats()["single_rank_loop"] == 3
    assert cs.plan()[0]["ring_size"] == (256 if nc == 2 else 512)
    if case == "step log":
        cs.enable_steplog(n_iter * nc)
    cs.run(n_iter)
    assert cs.sized_master() == (0, 0), "%s: the sized instantiation must not run" % case
    assert cs.fixed_master() == (case not in ("step log", "HTM_FAST=0"))
    _assert_oracle(cs, _oracle(params, data, n_iter), n_iter, False)


def test_library_exports_the_sized_master_query():
    """CPU: the library builds with the sized rows and exports htm_chains_sized_master, declared with the signature the binding uses"""
    import ctypes as C

    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "htm_chains_sized_master")
    restype, argtypes = _lib.SIGNATURES["htm_chains_sized_master"]
    assert restype is C.c_int and len(argtypes) == 3
    nc, ring = C.c_int(-1), C.c_int(-1)
    assert lib.htm_chains_sized_master(None, C.byref(nc), C.byref(ring)) == -1      # HTM_EINVAL: no handle
    assert "NULL" in lib.htm_last_error().decode()
