"""CPU: the restatement's side of the single-precision forward of locate (tests/locate_fp32_restatement.py): the U table, that the
documented arithmetic is within the bound on every case the GPU tests run, that the bound separates two wrong arithmetics from
it, and the new entry point's presence in the library, the signatures and the program's options."""
import ctypes

import numpy as np
import pytest

from hypotremormcmc_amd import _lib
from hypotremormcmc_amd import locate as lc
from tests import locate_fp32_restatement as l32
from tests.fp32_restatement import NUDGES, ULPS32


def test_u_table_and_emulate_is_within_the_bound():
    """U of the bound: the worst |ell_emulate - ell_reference| / (2^-24 D32) over the GPU tests' cases and the four nudges; the
    next power of two above it is locate_fp32_restatement.U, and emulate is within the bound on every case"""
    rows, worst_of_bound = {}, 0.0
    for key in l32.volume_cases():
        c, ref = l32.case(key), l32.references(key)
        fin = np.isfinite(ref.ell)
        for n, nudge in enumerate(NUDGES):
            ell = l32.emulate(c["sta"], c["obs"], c["use"], c["structure"], c["grid"], nudge=nudge, seed=n)
            assert np.array_equal(np.isnan(ell), np.isnan(ref.ell)), (key, nudge)
            err = np.abs(ell[fin].astype(l32.LD) - ref.ell[fin]).astype(np.float64)
            row = rows.setdefault(l32.group(key), [0.0] * len(NUDGES))
            row[n] = max(row[n], float(np.max(l32.units(err, ref.D32[fin]))))
            b = l32.bound(ref.D32[fin], c["abs"][fin])
            worst_of_bound = max(worst_of_bound, float(np.max(err / b)))
            assert np.all(err <= b), (key, nudge, float(np.max(err / b)))
    print("    nudge            " + "".join("%-8s" % (n if isinstance(n, str) else "%+d" % n if n else "0") for n in NUDGES))
    for name, row in rows.items():
        print("    %-17s" % name + "".join("%-8.2f" % v for v in row))
    worst = max(max(r) for r in rows.values())
    print(f"    worst {worst:.2f}; U = {l32.U}; fp32_restatement.ULPS32 = {ULPS32}; emulate's worst share of the bound {worst_of_bound:.3f}")
    assert l32.U / 2 < worst <= l32.U            # the next power of two above the worst


@pytest.mark.parametrize("mutant", ["f32_coords", "next_corr"])
def test_the_bound_separates_a_wrong_arithmetic(mutant):
    """on the case shifted by 2^12 km the documented arithmetic is within the bound in every cell under every nudge; each mutant
    is beyond it, at its worst cell by more than a factor of two and in more than a quarter of the cells"""
    c = l32.shifted_case()
    ell_ref, D32, _ = c["ref"]
    fin = np.isfinite(ell_ref)
    b = l32.bound(D32[fin], c["abs"][fin])
    for n, nudge in enumerate(NUDGES):
        good = l32.emulate(c["sta"], c["obs"], c["use"], c["structure"], c["grid"], nudge=nudge, seed=n)
        assert np.all(np.abs(good[fin].astype(l32.LD) - ell_ref[fin]).astype(np.float64) <= b), nudge
    bad = l32.emulate(c["sta"], c["obs"], c["use"], c["structure"], c["grid"], **{mutant: True})
    err = np.abs(bad[fin].astype(l32.LD) - ell_ref[fin]).astype(np.float64)
    u = l32.units(err, D32[fin])
    print(f"{mutant}: |ell - ell_ref| = {u.min():.3g} .. {u.max():.3g} x 2^-24 D32 (the bound: {l32.U}); {int((err > b).sum())} of {err.size} cells "
          f"beyond the bound, the worst at {float(np.max(err / b)):.3g} of it")
    # (a cell's error is a signed sum over six stations and can vanish at a cell: the volume as a whole is what a test judges)
    assert np.max(err / b) > 2.0 and (err > b).sum() > err.size // 4, (mutant, float(np.max(err / b)))


def test_the_symbol_is_declared_and_exported():
    assert _lib.SIGNATURES["htm_forward_locate_set_precision"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    lib = _lib.load()
    assert lib.htm_forward_locate_set_precision is not None and lib.htm_abi_version() == 1
    # a NULL handle is refused with a message, without a device
    assert lib.htm_forward_locate_set_precision(None, 1) == -1 and lib.htm_last_error().decode() == "NULL handle"


def test_the_program_refuses_an_unknown_precision(capsys):
    with pytest.raises(SystemExit) as exc:
        lc.main(["hypo.in", "--cell", "1", "--precision", "fp16"])
    assert exc.value.code == 2 and "--precision" in capsys.readouterr().err
