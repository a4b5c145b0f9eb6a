"""CPU: every chain-master loop unit (csrc/htm_loop_*.hip) includes the headers of the ONE loop it builds and nothing of the
others; k_mcmc's header (htm_mcmc.hpp) includes no loop; the forward unit and the locate unit include none either, and only the
locate unit sees the locate kernels; of the chain sets' four host
units only the set-up and the run unit see a loop header, each the ones it takes something from.  Read from the compiler's own
dependency list (hipcc -MM: preprocessing only), so an include that comes in through another header counts."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "hypotremormcmc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # the Makefile's default

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason=f"no hipcc ({HIPCC}): the include graph is read from its -MM output")

LOOP_HEADERS = {"htm_step.hpp", "htm_flow.hpp", "htm_pipe.hpp"}
# what every loop unit may see: the host side of the kernel table, the device basics, the hand-off, the workers, the kernel
COMMON = {"htm_host.hpp", "htm_kernels.hpp", "htm_plan.hpp", "htm_device.hpp", "htm_stream.hpp", "htm_handoff.hpp",
          "htm_worker.hpp", "htm_mcmc.hpp", "htm_loop_rows.hpp"}
ALLOWED = {
    "htm_loop_free": COMMON | {"htm_flow.hpp"},
    "htm_loop_lock": COMMON | {"htm_flow.hpp"},
    "htm_loop_barrier": COMMON | {"htm_step.hpp"},
    "htm_loop_wide": COMMON | {"htm_step.hpp"},
    "htm_loop_pipe": COMMON | {"htm_flow.hpp", "htm_pipe.hpp"},      # (the pipelined loop takes flow_swap_at from htm_flow.hpp)
}


# The chain sets' host units (the map: htm_host.hpp).  What htm_host.hpp itself brings in -- the types of a handle, the plan --
# every one of them sees; beyond that: the set-up unit takes sizes from the loops, the run unit has the small kernels of
# htm_chains_kernels.hpp (which is on htm_flow.hpp), and the state and comm units see nothing else: no edit of the hand-off,
# the workers, k_mcmc or a loop rebuilds them.
HOST = {"htm_host.hpp", "htm_kernels.hpp", "htm_plan.hpp", "htm_device.hpp", "htm_stream.hpp"}
SHARED_BY_LOOPS = {"htm_handoff.hpp", "htm_worker.hpp", "htm_mcmc.hpp"}
CHAIN_UNITS = {
    "htm_chains_setup": HOST | SHARED_BY_LOOPS | {"htm_flow.hpp", "htm_pipe.hpp"},
    "htm_chains_run": HOST | {"htm_handoff.hpp", "htm_flow.hpp", "htm_chains_kernels.hpp"},
    "htm_chains_state": HOST,
    "htm_comm": HOST,
}


def _project_headers(source, as_hip=False):
    """the htm_*.hpp files in the -MM closure of csrc/<source>"""
    cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-MM"]
    cmd += (["-x", "hip"] if as_hip else []) + [source]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return set(re.findall(r"\bhtm_\w+\.hpp\b", r.stdout))


def test_the_loop_units_are_the_ones_listed():
    units = {f[:-4] for f in os.listdir(CSRC) if f.startswith("htm_loop_") and f.endswith(".hip")}
    assert units == set(ALLOWED)


@pytest.mark.parametrize("unit", sorted(ALLOWED))
def test_loop_unit_includes_only_its_own_loop(unit):
    got = _project_headers(unit + ".hip")
    assert got <= ALLOWED[unit], sorted(got - ALLOWED[unit])
    assert got & LOOP_HEADERS, "a loop unit builds a loop"


def test_the_chain_set_host_units_are_the_ones_listed():
    units = {f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip")}
    assert units == set(ALLOWED) | set(CHAIN_UNITS) | {"htm_forward", "htm_locate", "htm_steps"}


@pytest.mark.parametrize("unit", sorted(CHAIN_UNITS))
def test_chain_set_host_unit_includes_only_what_it_may(unit):
    got = _project_headers(unit + ".hip")
    assert got <= CHAIN_UNITS[unit], sorted(got - CHAIN_UNITS[unit])
    assert "htm_host.hpp" in got      # (the closure was really read)
    assert "htm_step.hpp" not in got, "no successor of htm_hip.hip needs the barrier loop's header"


def test_htm_host_brings_in_no_loop_and_nothing_the_loops_share():
    """what the state and comm units are held to is htm_host.hpp's own closure: it must stay free of these"""
    got = _project_headers("htm_host.hpp", as_hip=True)
    assert got | {"htm_host.hpp"} == HOST
    assert not (got & (LOOP_HEADERS | SHARED_BY_LOOPS | {"htm_chains_kernels.hpp"}))


def test_only_the_setup_unit_takes_sizes_from_the_pipelined_loop_and_k_mcmc():
    for unit in CHAIN_UNITS:
        got = _project_headers(unit + ".hip")
        assert (unit == "htm_chains_setup") == bool(got & {"htm_pipe.hpp", "htm_mcmc.hpp"}), (unit, sorted(got))


def test_the_chain_kernels_header_is_included_by_one_unit():
    users = [f for f in sorted(os.listdir(CSRC)) if f.endswith(".hip") and "htm_chains_kernels.hpp" in _project_headers(f)]
    assert users == ["htm_chains_run.hip"]


def test_forward_unit_includes_no_loop():
    got = _project_headers("htm_forward.hip")
    assert not (got & LOOP_HEADERS)
    assert not (got & {"htm_locate.hpp", "htm_locate_plan.hpp", "htm_steps_host.hpp"}), "locate has a unit of its own"


def test_locate_unit_includes_no_loop_and_is_the_one_with_the_locate_kernels():
    got = _project_headers("htm_locate.hip")
    assert {"htm_locate.hpp", "htm_locate_plan.hpp", "htm_host.hpp"} <= got      # (the closure was really read)
    assert not (got & (LOOP_HEADERS | SHARED_BY_LOOPS | {"htm_chains_kernels.hpp", "htm_forward_kernels.hpp"}))
    users = [f for f in sorted(os.listdir(CSRC)) if f.endswith(".hip") and "htm_locate.hpp" in _project_headers(f)]
    assert users == ["htm_locate.hip"]


def test_the_locate_plan_includes_nothing_of_hip():
    """a plain C++ compiler reads it: of the project's headers it sees the map grid and the limits only"""
    got = _project_headers("htm_locate_plan.hpp", as_hip=True)
    assert got | {"htm_locate_plan.hpp"} == {"htm_locate_plan.hpp", "htm_grid.hpp", "htm_limits.hpp"}


def test_mcmc_header_includes_no_loop():
    got = _project_headers("htm_mcmc.hpp", as_hip=True)
    assert "htm_worker.hpp" in got and "htm_handoff.hpp" in got      # (the closure was really read)
    assert not (got & LOOP_HEADERS)
