"""The launch plan of a chain set (csrc/htm_plan.hpp; htm_chains_plan, htm_chains_get_plan): which chain-master loop each
mode runs and the launch shape, pinned against tests/golden/launch_plan.json.

The fixture was recorded on an MI355X from the commit BEFORE the planner was separated from htm_chains_create (its header
names that commit): a read-out of the handle's fields, of the device facts the creation saw and of launch_mcmc's if-chain,
over a grid that holds every value at which a rule switches.  The CPU test feeds the recorded device facts to
htm_chains_plan; the GPU test creates every chain set (and runs none)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from hypotremormcmc_amd import _lib, chains

# every environment switch htm_chains_create reads (htm_plan.hpp read_knobs): a case runs with its own ones only
KNOBS = ("HTM_WORKER_CAP", "HTM_MAX_WORKERS", "HTM_RANKS_PER_GPU", "HTM_SLOT_REPLICAS", "HTM_SLOT_STRIDE", "HTM_PGRAN_STRIDE",
         "HTM_NPOLL", "HTM_PERSIST", "HTM_DEBUG_NO_DROP", "HTM_XCHG_TIMEOUT_MS", "HTM_DEBUG_XCHG_FAIL_ITER", "HTM_XOWN",
         "HTM_STREAM_CAP", "HTM_PRIOR_SAME", "HTM_MB", "HTM_RING_SLACK", "HTM_FLOW", "HTM_FAST", "HTM_FLOW_LOCK", "HTM_PIPE",
         "HTM_PIPE_LOCK")
RUN, ADVANCE, LOCKRUN = 0, 1, 2      # rows of htm_launch_plan::loop

with open(os.path.join(os.path.dirname(__file__), "golden", "launch_plan.json")) as _f:
    FIXTURE = json.load(_f)
CASES = FIXTURE["cases"]
IDS = [c["id"] for c in CASES]


def set_env(setter, deleter, case):
    for k in KNOBS:
        deleter(k)
    for k, v in case["env"].items():
        assert k in KNOBS, k
        setter(k, v)


@pytest.fixture
def case_env(monkeypatch, request):
    case = request.param
    set_env(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), case)
    return case


def plan_or_error(job, device):
    """(plan, None) or (None, (code, text)) of htm_chains_plan"""
    lib = _lib.load()
    j = _lib.PlanJob(**job)
    f = _lib.PlanDevice(device["n_cu"], device["blocks_per_cu"], (C.c_int32 * 2)(*device["pipe_blocks_per_cu"]))
    p = _lib.LaunchPlan()
    rc = lib.htm_chains_plan(C.byref(j), C.byref(f), C.byref(p))
    if rc:
        return None, (rc, lib.htm_last_error().decode())
    return chains._plan_dict(p), None


def assert_plan(got, want, what):
    diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not diff, "%s: (got, recorded) differ in %r" % (what, diff)


NO_DEVICE = dict(n_cu=0, blocks_per_cu=0, pipe_blocks_per_cu=[0, 0])


@pytest.mark.parametrize("case_env", CASES, ids=IDS, indirect=True)
def test_plan_equals_the_recorded_one(case_env):
    case = case_env
    plan, err = plan_or_error(case["job"], case["device"] or NO_DEVICE)
    if "error" in case:
        assert err == (case["error_code"], case["error"])
        return
    assert err is None, err
    assert_plan(plan, case["plan"], case["id"])
    # what holds for every plan
    assert plan["step_smem"] <= 156 * 1024
    r = plan["ring_size"]
    assert r >= 256 and r & (r - 1) == 0
    assert plan["n_workers"] >= 1
    if plan["persist"]:
        assert plan["n_workers"] <= plan["blocks_fit"] - max(1, plan["mb_blocks"])
    assert plan["loop"][RUN][1] != 8      # a diagnostic run with a step log takes the generic instantiation
    # every loop a launch can take names a kernel that the library holds for this job (mcmc_kernel)
    assert plan["loop_built"] == [[1, 1], [1, 1], [1, 1]]
    for m, allowed in ((RUN, (0, 3, 5, 7, 8)), (ADVANCE, (1,)), (LOCKRUN, (2, 4, 6))):
        assert plan["loop"][m][0] in allowed and plan["loop"][m][1] in allowed


def test_fixture_holds_the_grid():
    """every value the rules switch at is in the fixture at least once"""
    jobs = [c["job"] for c in CASES]
    assert {j["n_chains"] for j in jobs} >= {1, 2, 4, 5, 8, 9, 12, 16, 17, 27, 32, 33, 64}
    assert {j["n_sta"] for j in jobs} >= {3, 16, 64, 65, 128, 129, 256, 300}
    assert {j["n_events"] for j in jobs} >= {1, 8, 9, 100, 1000, 2001, 10000}
    assert {j["n_procs"] for j in jobs} >= {1, 2, 8, 60, 61}
    assert {j["forward_fp32"] for j in jobs} == {0, 1}
    assert {(j["use_time"], j["use_amp"]) for j in jobs} == {(1, 1), (1, 0), (0, 1)}
    switches = {"%s=%s" % kv for c in CASES for kv in c["env"].items()}
    assert switches >= {"HTM_FLOW=0", "HTM_FAST=0", "HTM_MB=0", "HTM_MB=1", "HTM_PIPE=1", "HTM_PIPE_LOCK=1", "HTM_PERSIST=0",
                        "HTM_RING_SLACK=0", "HTM_DEBUG_NO_DROP=1", "HTM_MAX_WORKERS=3", "HTM_WORKER_CAP=40",
                        "HTM_RANKS_PER_GPU=4", "HTM_RANKS_PER_GPU=5", "HTM_STREAM_CAP=131072"}
    assert {c["share_gpu"] for c in CASES if c.get("share_gpu")} == {2, 4, 5, 8}
    refused = [c for c in CASES if "error" in c]
    assert any(c["job"]["n_chains"] > 32 for c in refused) and any(c["job"]["n_chains"] <= 32 for c in refused)
    assert 150 <= len(CASES) <= 260


# ---- on the device: creation only ------------------------------------------------------------------------------------------------
_FORWARDS = {}


def forward_for(job):
    """a forward handle of the job's shape (the data do not matter to the plan); the latest few are kept"""
    from hypotremormcmc_amd.forward import Forward

    key = (job["n_sta"], job["n_events"], job["use_time"], job["use_amp"], job["forward_fp32"])
    if key not in _FORWARDS:
        while len(_FORWARDS) >= 4:
            _FORWARDS.pop(next(iter(_FORWARDS))).close()
        S, E = job["n_sta"], job["n_events"]
        one = np.ones(S * E)

        class Obs:
            get_t_obs = get_t_stdv = get_a_obs = get_a_stdv = staticmethod(lambda: one)

        _FORWARDS[key] = Forward(S, E, np.arange(S, dtype=float), np.zeros(S), np.zeros(S), Obs, use_amp=job["use_amp"],
                                 use_time=job["use_time"], forward_precision="fp32" if job["forward_fp32"] else "fp64")
    return _FORWARDS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_forwards():
    yield
    while _FORWARDS:
        _FORWARDS.popitem()[1].close()


def create_bare(fwd, job):
    """htm_chains_create with nothing but the shapes: (handle, None) or (None, (code, text))"""
    lib = _lib.load()
    nc, S, E = job["n_chains"], job["n_sta"], job["n_events"]
    init = _lib.ChainsInit()
    init.n_chains, init.n_procs, init.rank = nc, job["n_procs"], 0
    keep = []
    for name, nx, v in (("hypo", 3 * E, 0.0), ("t_corr", S, 0.0), ("vs", 1, 3.5), ("a_corr", S, 0.0), ("qs", 1, 100.0)):
        a = np.full(nx * nc, v)
        keep.append(a)
        mi = _lib.ModelInit()
        mi.x = a.ctypes.data_as(_lib.dp)
        setattr(init, name, mi)
    t = np.ones(nc)
    init.temp = t.ctypes.data_as(_lib.dp)
    init.solve_vs = init.solve_t_corr = init.solve_qs = init.solve_a_corr = 1
    init.n_burn, init.n_interval = 0, 1
    init.lik_capacity = init.sample_capacity = 2 * nc
    h = C.c_void_p()
    rc = lib.htm_chains_create(fwd.handle, C.byref(init), C.byref(h))
    if rc:
        return None, (rc, lib.htm_last_error().decode())
    return h, None


def master_stats_of(handle):
    a = C.c_int(); b = C.c_int()
    _lib.check(_lib.load().htm_chains_master_stats(handle, C.byref(a), C.byref(b), None))
    return a.value, b.value


@pytest.mark.gpu
@pytest.mark.parametrize("case_env", CASES, ids=IDS, indirect=True)
def test_created_chain_set_has_the_recorded_plan(case_env):
    case = case_env
    lib = _lib.load()
    handle, err = create_bare(forward_for(case["job"]), case["job"])
    if "error" in case:
        assert err == (case["error_code"], case["error"])
        assert plan_or_error(case["job"], NO_DEVICE)[1] == err
        return
    assert err is None, err
    try:
        plan, seen = chains.get_plan(handle)
        assert seen == case["device"]
        assert_plan(plan, case["plan"], "htm_chains_get_plan")
        replanned, err = plan_or_error(case["job"], seen)
        assert err is None and replanned == plan
        # master_stats by its mapping: -1 the two-kernel path, the specialised instantiation reported as the free-running master
        want = tuple(-1 if not plan["persist"] else 3 if v == 8 else v for v in (plan["loop"][RUN][0], plan["loop"][LOCKRUN][0]))
        assert master_stats_of(handle) == want
        if case.get("share_gpu"):
            _lib.check(lib.htm_chains_share_gpu(handle, case["share_gpu"]))
            assert_plan(chains.get_plan(handle)[0], case["plan_after_share"], "after htm_chains_share_gpu")
    finally:
        lib.htm_chains_destroy(handle)
