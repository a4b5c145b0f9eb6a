"""CPU: every chain-master loop unit (csrc/htm_loop_*.hip) includes the headers of the ONE loop it builds and nothing of the
others; k_mcmc's header (htm_mcmc.hpp) includes no loop; the forward unit includes none either.  Read from the compiler's own
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


def test_forward_unit_includes_no_loop():
    assert not (_project_headers("htm_forward.hip") & LOOP_HEADERS)


def test_mcmc_header_includes_no_loop():
    got = _project_headers("htm_mcmc.hpp", as_hip=True)
    assert "htm_worker.hpp" in got and "htm_handoff.hpp" in got      # (the closure was really read)
    assert not (got & LOOP_HEADERS)
