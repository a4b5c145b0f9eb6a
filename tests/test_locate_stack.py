"""CPU: the restatement's side of every precondition of tests/test_gpu_locate_stack.py (the rule of htm_forward_locate_stack,
tests/locate_stack_restatement.py), and the host helpers of `locate --stack`: the regions of a map of floats, the text of the
map files, the program's argument errors and --stack-resolved's layers."""
import math

import numpy as np
import pytest

from hypotremormcmc_amd import density as dn
from hypotremormcmc_amd import locate as lc
from tests import locate_stack_cases as sc
from tests import locate_stack_restatement as sr

EPS = 2.0 ** -53


@pytest.mark.parametrize("which", list(sc.LAYERINGS))
@pytest.mark.parametrize("name", list(sc.CASES))
def test_every_layer_holds_one_unit_of_mass_per_window(name, which):
    """the restatement's stack of a layer sums to tally[L][0] within cells 2^-53 relative (a window's masses are roundings of
    numbers that sum to 1), and so does each of its maps; nothing is NaN; a window without an included cell is in tally[L][1]"""
    c = sc.case(name)
    layer, n_layer = sc.layering(name, which)
    ref = sr.stack_rule(c["lp_prior"], layer, n_layer)
    cells = ref["stack"][0].size
    E = c["lp_prior"].shape[0]
    assert ref["tally"].sum() == (E if layer is None else ((layer >= 0) & (layer < n_layer)).sum())
    for L in range(n_layer):
        n = ref["tally"][L, 0]
        for key in ("stack", "xy", "xz", "yz"):
            assert not np.isnan(ref[key][L]).any() and (ref[key][L] >= 0.0).all()
            assert abs(math.fsum(ref[key][L].reshape(-1)) - n) <= cells * EPS * n, (L, key)
    if name == "1x1x1":
        assert np.array_equal(ref["stack"].reshape(-1), ref["tally"][:, 0])
    if name == "excluded":
        assert ref["tally"][:, 1].sum() == 1 and ref["m"][2].sum() == 0.0 and ref["stack"][:, 0, 1, 1].sum() == 0.0
    if which == "three":
        assert ref["tally"][1].sum() == 0 and not ref["stack"][1].any()          # the empty layer


@pytest.mark.parametrize("which", list(sc.LAYERINGS))
@pytest.mark.parametrize("name", sc.INDEPENDENT)
def test_cells_held_against_the_independent_restatement_carry_the_mass(name, which):
    """the cells whose stack is at least 1e-200 of the layer's largest carry more than 1 - 1e-12 of every layer's mass"""
    c = sc.case(name)
    layer, n_layer = sc.layering(name, which)
    ref = sr.stack_rule(c["lp_prior"], layer, n_layer)
    for L in range(n_layer):
        s = ref["stack"][L].reshape(-1)
        if ref["tally"][L, 0] == 0:
            continue
        judged = s >= 1e-200 * s.max()
        assert math.fsum(s[~judged]) < 1e-12 * math.fsum(s), (L, math.fsum(s[~judged]))


def test_masses_take_the_given_best_lp():
    """with lp_best given the masses are formed against it (the library's loc[4]); the volume's own maximum gives the same"""
    c = sc.case("5x3x2")
    best = np.array([v[~np.isnan(v)].max() for v in c["lp_prior"]])
    a, b = sr.masses(c["lp_prior"]), sr.masses(c["lp_prior"], best)
    assert np.array_equal(a[0], b[0]) and a[1].all()


# ---- the regions of a map of floats ------------------------------------------------------------------------------------------
def test_float_regions_agree_with_the_integer_ones():
    rng = np.random.default_rng(5)
    for shape, top in (((4, 5), 3), ((3, 7, 2), 50), ((30,), 1), ((6, 6), 1000)):
        counts = rng.integers(0, top + 1, shape).astype(np.uint64)
        for levels in ([0.68, 0.95], [0.5], [1.0, 0.1, 0.9]):
            assert np.array_equal(lc.hpd_levels_mass(counts.astype(np.float64), levels), dn.hpd_levels(counts, levels)), (shape, top, levels)
    assert not lc.hpd_levels_mass(np.zeros((3, 3)), [0.68]).any()
    # scaling the masses changes nothing
    counts = rng.integers(0, 9, (5, 5)).astype(np.float64)
    assert np.array_equal(lc.hpd_levels_mass(counts * 0.125, [0.68, 0.95]), lc.hpd_levels_mass(counts, [0.68, 0.95]))


def test_float_regions_take_ties_together_and_leave_empty_cells_out():
    m = np.array([0.25, 0.25, 0.25, 0.125, 0.125, 0.0])
    # the three largest tie: they enter the 0.5 region together although two of them reach it
    assert list(lc.hpd_levels_mass(m, [0.5, 0.9])) == [0.5, 0.5, 0.5, 0.9, 0.9, 0.0]
    assert list(lc.hpd_levels_mass(m, [0.75])) == [0.75, 0.75, 0.75, 0.0, 0.0, 0.0]
    assert list(lc.hpd_levels_mass(m, [1.0])) == [1.0] * 5 + [0.0]
    with pytest.raises(ValueError):
        lc.hpd_levels_mass(m, [0.0])
    with pytest.raises(ValueError):
        lc.hpd_levels_mass(np.array([0.5, -0.1]), [0.5])
    with pytest.raises(ValueError):
        lc.hpd_levels_mass(np.array([0.5, np.nan]), [0.5])


# ---- the text of the map files -------------------------------------------------------------------------------------------------
def test_map_text_layout():
    grid = [10.0, 2.0, 3, -5.0, 0.5, 2, 0.0, 1.0, 2]
    xy = np.zeros((2, 2, 3))
    xy[0, 1, 2], xy[0, 0, 0], xy[1, 0, 1] = 1.5, 0.5, 2.0e-7
    lines = lc.stack_map_text("xy", xy, grid, [0.68, 0.95]).split("\n")
    assert lines[0] == lc.STACK_HEADERS["xy"] and lines[0].startswith("# layer, cell ix iy, centre x y, expected windows") and "no sample" in lines[0]
    assert len(lines) == 1 + 2 * 6 + 1 and lines[-1] == ""
    # density's order (ix fastest) and formats, without the sample count
    assert lines[1] == "%5d%6d%6d%14.6f%14.6f%14.6e%8.4f" % (0, 0, 0, 11.0, -4.75, 0.5, 0.95)
    assert lines[2] == "%5d%6d%6d%14.6f%14.6f%14.6e%8.4f" % (0, 1, 0, 13.0, -4.75, 0.0, 0.0)
    assert lines[6] == "%5d%6d%6d%14.6f%14.6f%14.6e%8.4f" % (0, 2, 1, 15.0, -4.25, 1.5, 0.68)
    assert lines[8] == "%5d%6d%6d%14.6f%14.6f%14.6e%8.4f" % (1, 1, 0, 13.0, -4.75, 2.0e-7, 0.68)
    # the same columns as tremor_density.xy.dat up to the centre, and one column fewer
    counts = np.zeros((2, 2, 3), dtype=np.uint64)
    counts[0, 1, 2] = 3
    dens = dn.map_text("xy", counts, grid, 2, [0.68, 0.95]).split("\n")
    assert [ln[:45] for ln in dens[1:]] == [ln[:45] for ln in lines[1:]]
    assert all(len(a.split()) == len(b.split()) + 1 for a, b in zip(dens[1:-1], lines[1:-1]))
    vol = lc.stack_map_text("vol", np.ones((1, 2, 2, 3)), grid, [0.5]).split("\n")
    assert vol[0].startswith("# layer, cell ix iy iz, centre x y z") and len(vol) == 14 and len(vol[1].split()) == 9
    yz = lc.stack_map_text("yz", np.ones((1, 2, 2)), grid, [0.5]).split("\n")
    assert yz[0].startswith("# layer, cell iy iz, centre y z") and yz[2].split()[:5] == ["0", "1", "0", "-4.250000", "0.500000"]


def test_summary_lines():
    text = lc.stack_summary_text(np.array([[5.0, 1.0], [0.0, 0.0]]), np.array([0.125, np.nan]), 3)
    assert text.split("\n") == ["3 windows left out of the stack: their best cell lies on a face of the box",
                                "layer 0: 5 windows stacked, 1 without an included cell, 12.50 % of the mass on the faces of the box",
                                "layer 1: 0 windows stacked, 0 without an included cell, NaN of the mass on the faces of the box", ""]
    assert len(lc.stack_summary_text(np.array([[5.0, 1.0]]), np.array([0.0])).split("\n")) == 2
    s = np.zeros((2, 3, 3, 3))
    s[0, 1, 1, 1], s[0, 0, 1, 1] = 3.0, 1.0
    share = lc.face_share(s)
    assert share[0] == 0.25 and np.isnan(share[1])
    assert lc.face_share(np.ones((1, 2, 5, 5)))[0] == 1.0            # two layers in z: every cell is on a face


# ---- the program's arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,name", [(["--time-bins", "2"], "--time-bins"), (["--stack-volume"], "--stack-volume"),
                                        (["--stack-resolved"], "--stack-resolved"), (["--level", "0.5"], "--level")])
def test_stack_options_need_stack(extra, name, capsys):
    with pytest.raises(SystemExit) as err:
        lc.main(["no_such_file.in", "--cell", "1"] + extra)
    assert err.value.code == 2
    assert f"{name} needs --stack" in capsys.readouterr().err


@pytest.mark.parametrize("extra,msg", [(["--time-bins", "0"], "--time-bins must be at least 1"), (["--level", "0.5", "1.5"], "--level must lie in (0, 1]"),
                                       (["--level", "0"], "--level must lie in (0, 1]")])
def test_stack_option_values_are_checked(extra, msg, capsys):
    with pytest.raises(SystemExit) as err:
        lc.main(["no_such_file.in", "--cell", "1", "--stack"] + extra)
    assert err.value.code == 2
    assert msg in capsys.readouterr().err


def test_resolved_layer_switches_off_the_windows_on_a_face():
    grid = [0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 3]
    cell = lambda ix, iy, iz: ix + 4 * (iy + 3 * iz)
    #        inside         x low          x high         y high         z low          z high         no cell
    index = [cell(1, 1, 1), cell(0, 1, 1), cell(3, 1, 1), cell(2, 2, 1), cell(1, 1, 0), cell(2, 1, 2), -1, cell(2, 1, 1)]
    layer = np.array([0, 1, 2, 0, 1, 2, 1, -1], dtype=np.int32)
    got = lc.resolved_layer(layer, index, grid)
    assert got.dtype == np.int32 and list(got) == [0, -1, -1, -1, -1, -1, 1, -1]
    assert list(layer) == [0, 1, 2, 0, 1, 2, 1, -1]                 # the input is left alone
