"""CPU: the C-ABI library builds, loads and exports every symbol include/htm_hip.h declares; without a GPU
its entry points fail loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _declared():
    src = open(os.path.join(ROOT, "include", "htm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(htm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    names = _declared()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/htm_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert lib.htm_abi_version() == 1


def test_no_cpu_fallback_without_device():
    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    n = C.c_int(-1)
    rc = lib.htm_device_count(C.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present; the no-device behaviour is exercised on the CPU-only container")
    from hypotremormcmc_amd.forward import Forward
    from hypotremormcmc_amd.obs_data import ObsData

    z = np.zeros((2, 3))
    obs = ObsData.from_arrays(np.zeros(3), np.zeros(3), z, z + 1, z, z + 1)
    with pytest.raises(_lib.HtmError, match="no HIP device|CPU fallback"):
        Forward(n_sta=3, n_events=2, sta_x=np.zeros(3), sta_y=np.zeros(3), sta_z=np.zeros(3), obs=obs)
    assert lib.htm_selftest(0) == -2       # HTM_ENODEVICE
    # The library is built from several translation units with ONE last-error string behind htm_last_error(): a failure raised
    # in each host unit (forward with the self-test, steps, chains) is what it returns next, whichever unit failed before.
    last = lambda: lib.htm_last_error().decode()
    assert "no HIP device" in last()                                   # the self-test, just above
    assert lib.htm_device_count(None) == -1 and last() == "n is NULL"  # HTM_EINVAL from a forward-unit entry point
    x = np.zeros(64, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(64).ctypes.data_as(C.POINTER(C.c_double))
    assert lib.htm_convert(0, x, x, 64, 16, 1, 2, None, 1.0, 1.0, 0, 0, out) == -1      # step 1 with a NULL band
    assert last() == "NULL argument"
    assert lib.htm_chains_run(None, 1) == -1 and last() == "NULL handle"
    assert lib.htm_selftest(0) == -2 and "no HIP device" in last()


@pytest.mark.gpu
def test_device_ordinal_past_the_last_is_einval():
    """one entry point of each family of the steps' unit, smallest valid shapes, device = htm_device_count(): HTM_EINVAL with
    "out of range" from the shared device selection, before anything is allocated or launched"""
    from hypotremormcmc_amd import _lib

    lib = _lib.load()
    n = C.c_int(-1)
    assert lib.htm_device_count(C.byref(n)) == 0 and n.value >= 1
    bad = n.value
    x, out = np.arange(16.0), np.zeros(32)
    px, po = _lib.ptr(x), _lib.ptr(out)
    calls = {
        "htm_quantiles": lambda: lib.htm_quantiles(bad, px, 4, 1, (C.c_int * 3)(1, 2, 4), po),
        "htm_diagnose": lambda: lib.htm_diagnose(bad, px, 1, 4, 1, 1, po, None),
        "htm_rank_normalize": lambda: lib.htm_rank_normalize(bad, px, 4, 1, 0, po, None),
        "htm_hypo_ellipsoid": lambda: lib.htm_hypo_ellipsoid(bad, px, None, 4, 1, 0, 3, po, None),
        "htm_xcorr": lambda: lib.htm_xcorr(bad, px, 2, 2, 2, 1, 1, 0, 1, po, po),
        "htm_fft": lambda: lib.htm_fft(bad, px, 2, po, 2, 2, 1, -1),
    }
    for name, call in calls.items():
        assert call() == -1, name                   # HTM_EINVAL
        assert "out of range" in lib.htm_last_error().decode(), name


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "hypotremormcmc_amd")
    for dp_, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".f90", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(dp_, f), errors="ignore").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "liboracle" not in txt and "htm_oracle" not in txt, f
