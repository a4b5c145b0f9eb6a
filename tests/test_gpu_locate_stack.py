"""GPU: htm_forward_locate_stack (k_locate_stack, k_locate_stack_project: hypotremormcmc_amd/csrc/htm_locate.hpp; DESIGN.md
§3.14) at the smallest shapes at which the kernels can go wrong, against the numpy restatement of its rule
(tests/locate_stack_restatement.py).

The stack is pinned to the restatement applied to the device's OWN volume and loc[4] (locate.locate(..., volume=True)), which
separates the stacking from the evaluation: per stacked cell |stack - ref| <= (2e-12 + E 2^-53) ref, E the windows of the
case -- W is held to 1e-12 relative by the existing contract of the weight sums, the subtraction's rounding is at most
745 * 2^-53 = 8e-14 in the exponent, exp, the reciprocal and the product are a few ulp, and a sequential sum of E non-negative
terms adds E 2^-53.  Where ref is subnormal the difference must be 0 or below 1e-300.  On two cases the stack is also held
against the independent restatement's volumes: (2e-12 + 2e-12 A_e) relative per contributing window, A_e the window's largest
sum of absolute terms over its included cells (a cell's lp and the window's evidence are each good to 1e-12 A), on the cells
that carry the mass (tests/test_locate_stack.py).  The maps are pinned to the device's own stack: n 2^-53 relative of
math.fsum along the summed axis of length n."""
import math
import os

import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from hypotremormcmc_amd.forward import Forward, ObsArrays
from tests import locate_cases as cases
from tests import locate_marginal_cases as mcases
from tests import locate_stack_cases as sc
from tests import locate_stack_restatement as sr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
TINY = np.finfo(float).tiny
KEYS = ("xy", "xz", "yz", "stack", "tally")


def forward_of(c):
    E, S = c["obs"][0].shape
    return Forward(S, E, c["sta"][0], c["sta"][1], c["sta"][2], ObsArrays(*c["obs"]), use_time=c["use"][0], use_amp=c["use"][1])


def run(c, layer=None, n_layer=1, structure=None, volume=True, also=None, **kw):
    """lc.stack of the case under its prior; with `also` ("locate" or "locate_marginal") that call's result on the same
    Forward comes second"""
    fwd = forward_of(c)
    try:
        tc, vs, ac, qs = c["structure"] if structure is None else structure
        res = lc.stack(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], layer=layer, n_layer=n_layer, volume=volume, **kw)
        if also is None:
            return res
        return res, getattr(lc, also)(fwd, tc, vs, ac, qs, c["grid"], prior=c["prior"], volume=True, **kw)
    finally:
        fwd.close()


def same(a, b):
    for key in KEYS + ("loc", "marg_x", "marg_y", "marg_z"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def check_loc(res, own):
    """check 1: loc and the marginals are the other entry point's, bit for bit"""
    for key in ("loc", "marg_x", "marg_y", "marg_z"):
        assert np.array_equal(res[key], own[key], equal_nan=True), key
    assert res["vol"] is None


def check_stack(res, own, layer, n_layer, what):
    """check 2: the stack and the tally against the rule applied to the device's own volume and loc[4]"""
    E = own["vol"].shape[0]
    ref = sr.stack_rule(own["vol"], layer, n_layer, lp_best=own["loc"][:, 4])
    assert np.array_equal(res["tally"], ref["tally"]), what
    got, want = res["stack"], ref["stack"]
    assert got.shape == want.shape and not np.isnan(got).any() and (got >= 0.0).all(), what
    assert not got[want == 0.0].any(), what
    sub = (want > 0.0) & (want < TINY)
    diff = np.abs(got - want)
    assert np.all((diff[sub] == 0.0) | (diff[sub] < 1e-300)), what
    norm = want >= TINY
    bound = 2e-12 + E * EPS
    ratio = diff[norm] / (bound * want[norm])
    print(f"{what}: {norm.sum()} stacked cells ({sub.sum()} subnormal), worst |stack - ref| / ((2e-12 + {E} 2^-53) ref) = "
          f"{ratio.max() if ratio.size else 0.0:.3e}")
    assert np.all(ratio <= 1.0), (what, ratio.max())
    return ref


def check_maps(res, what):
    """check 4: the maps against the device's own stack, and every layer's unit of mass per window"""
    stack = res["stack"]
    cells = stack[0].size
    for key, axis, want in zip(("xy", "xz", "yz"), (1, 2, 3), sr.project(stack)):
        n = stack.shape[axis]
        got = res[key]
        assert got.shape == want.shape and not np.isnan(got).any(), (what, key)
        err = np.abs(got - want)
        big = want >= TINY                      # (sums of subnormal numbers are exact: the assertion below holds them to 0)
        worst = float(np.max(err[big] / (n * EPS * want[big]))) if big.any() else 0.0
        print(f"{what}: {key}, worst |map - fsum| / ({n} 2^-53 fsum) = {worst:.3e}")
        assert np.all(err <= n * EPS * want), (what, key, worst)
    for L in range(stack.shape[0]):
        n_in = res["tally"][L, 0]
        for key in KEYS[:4]:
            total = math.fsum(res[key][L].reshape(-1))
            assert abs(total - n_in) <= (2e-12 + cells * EPS) * n_in, (what, L, key, total, n_in)


# ---- the stack, the maps, loc and the marginals at every shape, under both layerings ------------------------------------------
@pytest.mark.parametrize("which", list(sc.LAYERINGS))
@pytest.mark.parametrize("name", list(sc.CASES))
def test_stack_and_maps_follow_the_rule(name, which):
    c = sc.case(name)
    layer, n_layer = sc.layering(name, which)
    what = f"{name}, {which}"
    res, own = run(c, layer, n_layer, also="locate")
    check_loc(res, own)
    check_stack(res, own, layer, n_layer, what)
    check_maps(res, what)
    if name == "1x1x1":          # one cell, which holds every window's whole mass
        assert np.array_equal(res["stack"].reshape(-1), res["tally"][:, 0])
    if name == "excluded":       # a NaN cell, a window that loses a z-layer, a window with no cell left
        assert res["tally"][:, 1].sum() == 1 and res["tally"][-1, 1] == 1 and res["index"][2] == -1
        assert not res["stack"][:, 0, 1, 1].any()
        assert all(not np.isnan(res[key]).any() for key in KEYS)
    if which == "three":
        assert not res["tally"][1].any() and not res["stack"][1].any() and not res["xy"][1].any()


def test_single_precision_forward():
    """the fp32 forward changes lp, and the stack consumes lp: the same checks against the fp32 volume"""
    c = sc.case("67x3x5")
    layer, n_layer = sc.layering("67x3x5", "three")
    res, own = run(c, layer, n_layer, also="locate", precision="fp32")
    fp64 = run(c, layer, n_layer)
    assert not np.array_equal(res["stack"], fp64["stack"])
    check_loc(res, own)
    check_stack(res, own, layer, n_layer, "67x3x5, fp32")
    check_maps(res, "67x3x5, fp32")


@pytest.mark.parametrize("which", list(sc.LAYERINGS))
@pytest.mark.parametrize("name", sc.INDEPENDENT)
def test_stack_against_the_independent_restatement(name, which):
    """check 3: volumes that the device had no part in"""
    c = sc.case(name)
    layer, n_layer = sc.layering(name, which)
    ref = sr.stack_rule(c["lp_prior"], layer, n_layer)
    res = run(c, layer, n_layer)
    assert np.array_equal(res["tally"], ref["tally"])
    E = c["lp_prior"].shape[0]
    inc = [~np.isnan(c["lp_prior"][e]) & (c["lp_prior"][e] != -np.inf) for e in range(E)]
    A = np.array([c["abs_prior"][e][inc[e]].max() for e in range(E)])
    bound_of = (2e-12 + 2e-12 * A)[:, None, None, None] * ref["m"]            # per contributing window
    for L in range(n_layer):
        want = ref["stack"][L]
        if ref["tally"][L, 0] == 0:
            assert not res["stack"][L].any()
            continue
        judged = want >= 1e-200 * want.max()
        assert math.fsum(want[~judged]) < 1e-12 * math.fsum(want.reshape(-1))
        bound = bound_of[ref["layer"] == L].sum(axis=0)
        ratio = np.abs(res["stack"][L] - want)[judged] / bound[judged]
        print(f"{name}, {which}, layer {L}: {judged.sum()} cells, worst |stack - ref| / bound = {ratio.max():.3e}")
        assert np.all(ratio <= 1.0), (L, ratio.max())


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_every_batching_give_the_same_bits(monkeypatch):
    """check 5: a cell's running total goes through memory unchanged from batch to batch.  HTM_LOCATE_MB between the workspace
    of one and of two events per batch (include/htm_hip.h's formula): seven batches of one window, the layer changing from batch
    to batch; half an event less is refused"""
    name = "67x3x5"
    c = sc.case(name)
    layer, n_layer = sc.layering(name, "three")
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    first = run(c, layer, n_layer)
    same(first, run(c, layer, n_layer))
    fixed, per_event = sc.workspace_bytes(c["grid"], sc.N_STA, sc.N_EVENTS, n_layer, True)
    monkeypatch.setenv("HTM_LOCATE_MB", repr((fixed + 1.5 * per_event) / 1048576.0))
    same(first, run(c, layer, n_layer))
    monkeypatch.setenv("HTM_LOCATE_MB", repr((fixed + 3.5 * per_event) / 1048576.0))         # batches of 3, 3, 1
    same(first, run(c, layer, n_layer))
    monkeypatch.setenv("HTM_LOCATE_MB", repr((fixed + 0.5 * per_event) / 1048576.0))
    with pytest.raises(lc._lib.HtmError, match="HTM_LOCATE_MB"):
        run(c, layer, n_layer)


def test_one_draw_and_equal_draws_give_the_fixed_structure_bits():
    name = "5x3x2"
    c = sc.case(name)
    layer, n_layer = sc.layering(name, "three")
    tc, vs, ac, qs = c["structure"]
    fixed = run(c, layer, n_layer)
    for K in (1, 9):             # 9: more than one block of 8 draws
        draws = (np.tile(tc, (K, 1)), np.full(K, vs), np.tile(ac, (K, 1)), np.full(K, qs))
        same(fixed, run(c, layer, n_layer, structure=draws))


def test_marginal_form_with_distinct_draws():
    """check 6: K = 7 draws, against the rule applied to locate_marginal's own volume"""
    name = "5x3x2"
    c = sc.case(name)
    layer, n_layer = sc.layering(name, "three")
    draws = mcases.draws(sc.N_STA, 7 * sc.N_STA + sc.N_EVENTS, "tight", 7)
    res, own = run(c, layer, n_layer, structure=draws, also="locate_marginal")
    assert not np.array_equal(res["stack"], run(c, layer, n_layer)["stack"])
    check_loc(res, own)
    check_stack(res, own, layer, n_layer, "5x3x2, 7 draws")
    check_maps(res, "5x3x2, 7 draws")


def test_outputs_that_are_not_asked_for():
    """loc, marg and stack may be NULL: the maps and the tally are the same"""
    c = sc.case("5x3x2")
    layer, n_layer = sc.layering("5x3x2", "three")
    full = run(c, layer, n_layer)
    assert run(c, layer, n_layer, volume=False)["stack"] is None
    fwd = forward_of(c)
    try:
        tc, vs, ac, qs = c["structure"]
        out = {k: np.empty_like(full[k]) for k in ("xy", "xz", "yz", "tally")}
        fwd.locate_stack(0, tc, np.array([vs]), ac, np.array([qs]), np.asarray(c["grid"], dtype=np.float64), np.ascontiguousarray(c["prior"]), layer,
                         n_layer, None, None, out["xy"], out["xz"], out["yz"], None, out["tally"])
    finally:
        fwd.close()
    for k, v in out.items():
        assert np.array_equal(v, full[k]), k


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(monkeypatch):
    """check 7: HTM_EINVAL with a message, before any device call"""
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    c = sc.case("5x3x2")
    E, S = sc.N_EVENTS, sc.N_STA
    fwd = forward_of(c)
    lib, p = lc._lib.load(), lc._lib.ptr
    tc, vs, ac, qs = c["structure"]
    good = {"n_draws": 0, "tc": tc, "vs": np.array([vs]), "ac": ac, "qs": np.array([qs]), "grid": np.asarray(c["grid"], dtype=np.float64),
            "prior": np.ascontiguousarray(c["prior"]), "layer": np.array(sc.LAYERS3, dtype=np.int32), "n_layer": 3}
    SENT = -12345.0
    names = ("loc", "marg", "xy", "xz", "yz", "stack", "tally")
    shapes = {"loc": E * 16, "marg": E * 10, "xy": 3 * 15, "xz": 3 * 10, "yz": 3 * 6, "stack": 3 * 30, "tally": 6}

    def call(drop=(), **kw):
        a = dict(good, **kw)
        out = {k: np.full(shapes[k], SENT) for k in names}
        ptrs = [None if k in drop else p(out[k]) for k in names]
        rc = lib.htm_forward_locate_stack(fwd.handle, a["n_draws"], p(a["tc"]), p(a["vs"]), p(a["ac"]), p(a["qs"]), p(a["grid"]), p(a["prior"]),
                                          None if a["layer"] is None else a["layer"].ctypes.data_as(lc._lib.ip), a["n_layer"], *ptrs)
        return rc, lib.htm_last_error().decode(), out

    def refused(msg, **kw):
        rc, text, out = call(**kw)
        assert rc == -1 and msg in text, (kw.keys(), rc, text)
        assert all((v == SENT).all() for v in out.values()), kw.keys()

    try:
        rc, _, out = call()
        assert rc == 0 and all(not (v == SENT).any() for v in out.values())
        for key in ("tc", "vs", "ac", "qs", "grid"):
            refused("NULL argument", **{key: None})
        assert lib.htm_forward_locate_stack(None, 0, *([None] * 7), 1, *([None] * 7)) == -1 and "NULL handle" in lib.htm_last_error().decode()
        # whatever htm_forward_locate and htm_forward_locate_marginal refuse
        for vs_bad in (0.0, -1.0, float("nan"), float("inf")):
            refused("need finite values > 0", vs=np.array([vs_bad]))
        refused("need finite values > 0", qs=np.array([0.0]))
        refused("n_draws = -1", n_draws=-1)
        refused("n_draws = 4097", n_draws=4097)
        two = {"n_draws": 2, "tc": np.tile(tc, (2, 1)), "ac": np.tile(ac, (2, 1))}
        assert call(vs=np.array([vs, vs]), qs=np.array([qs, qs]), **two)[0] == 0
        refused("draw 1", vs=np.array([vs, float("nan")]), qs=np.array([qs, qs]), **two)
        bad = lambda i, val: np.array([val if k == i else g for k, g in enumerate(good["grid"])])
        for i, val, msg in ((1, 0.0, "cell size"), (0, float("inf"), "origin"), (2, 0.0, "cells"), (5, 2.5, "cells"), (8, 4097.0, "cells")):
            refused(msg, grid=bad(i, val))
        refused("more than 2^31 - 1", grid=np.array([0.0, 1.0, 4096, 0.0, 1.0, 4096, 0.0, 1.0, 128]))
        prior = good["prior"].copy()
        prior[3, 2] = 0.0
        refused("event 3: prior widths", prior=prior)
        # the stack's own
        refused("n_layer = 0", n_layer=0)
        refused("n_layer = -2", n_layer=-2)
        refused("without a layer per window", layer=None, n_layer=2)
        assert call(layer=None, n_layer=1, drop=("loc", "marg", "stack"))[0] == 0
        for key in ("xy", "xz", "yz", "tally"):
            refused("NULL output", drop=(key,))
        # 2^29 cells, which one layer may have, in four layers: more than 2^31 - 1 doubles over all layers' outputs
        refused("more than 2^31 - 1 doubles", grid=np.array([0.0, 1.0, 4096, 0.0, 1.0, 4096, 0.0, 1.0, 32]), n_layer=4, prior=None)
        fixed, per_event = sc.workspace_bytes(c["grid"], S, E, 3, True)
        monkeypatch.setenv("HTM_LOCATE_MB", repr((fixed + 0.9 * per_event) / 1048576.0))
        refused("HTM_LOCATE_MB")
        monkeypatch.setenv("HTM_LOCATE_MB", repr((fixed + 1.01 * per_event) / 1048576.0))
        assert call()[0] == 0
    finally:
        fwd.close()


def test_python_arguments_are_checked():
    c = sc.case("5x3x2")
    fwd = forward_of(c)
    tc, vs, ac, qs = c["structure"]
    try:
        with pytest.raises(ValueError, match="n_layer"):
            lc.stack(fwd, tc, vs, ac, qs, c["grid"], n_layer=0)
        with pytest.raises(ValueError, match="without a layer"):
            lc.stack(fwd, tc, vs, ac, qs, c["grid"], n_layer=2)
        with pytest.raises(ValueError, match="one per window"):
            lc.stack(fwd, tc, vs, ac, qs, c["grid"], layer=[0, 1], n_layer=2)
        with pytest.raises(ValueError, match="one per station"):
            lc.stack(fwd, tc[:-1], vs, ac, qs, c["grid"])
    finally:
        fwd.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_program_end_to_end(tmp_path, capsys):
    """check 8: --stack writes the three maps from the evaluation that hypo_grid.stat comes from, and changes nothing else"""
    from hypotremormcmc_amd.density import time_layers
    from hypotremormcmc_amd.grid import make_grid
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.run_files import Step5Run

    data = cases.e2e_data()
    d = str(tmp_path)
    synth.write_dataset(d, data)
    synth.write_param_file(os.path.join(d, "hypo.in"))
    cases.write_structure(d, ["S%03d" % (j + 1) for j in range(16)], np.zeros(16), np.zeros(16), vs=3.0, qs=250.0)
    base = [os.path.join(d, "hypo.in"), "--cell"] + [str(v) for v in cases.E2E_CELL] + ["--bounds"] + [str(v) for v in cases.E2E_BOUNDS]
    lc.main(base)
    plain = {nm: open(os.path.join(d, nm), "rb").read() for nm in ("hypo_grid.stat", "hypo_grid.best.dat")}
    plain_out = capsys.readouterr().out
    assert not any(nm.startswith("hypo_grid.density") for nm in os.listdir(d))
    lc.main(base + ["--stack", "--time-bins", "2", "--level", "0.68", "0.95"])
    for nm, text in plain.items():
        assert open(os.path.join(d, nm), "rb").read() == text, nm
    assert sorted(nm for nm in os.listdir(d) if nm.startswith("hypo_grid.density")) == ["hypo_grid.density.%s.dat" % m for m in ("xy", "xz", "yz")]
    # the library call with the same inputs, read from the same files
    r5 = Step5Run.open(os.path.join(d, "hypo.in"))
    par = r5.par
    grid = make_grid(cases.E2E_BOUNDS, cases.E2E_CELL)
    obs = ObsData(r5.win_id, par.n_stations, par.sta_x, par.sta_y, directory=r5.work)
    vs, qs, t_corr, a_corr = lc.read_structure(d, par.stations)
    layer = time_layers(r5.win_id, 2)
    fwd = Forward(par.n_stations, len(r5.win_id), par.sta_x, par.sta_y, par.sta_z, obs, use_amp=par.get_use_amp(), use_time=par.get_use_time())
    try:
        res = lc.stack(fwd, t_corr, vs, a_corr, qs, grid, prior=lc.step5_prior(par, obs), layer=layer, n_layer=2, volume=True)
    finally:
        fwd.close()
    assert res["tally"][:, 0].sum() == 8 and (res["tally"][:, 0] > 0).all()
    for nm in ("xy", "xz", "yz"):
        lines = open(os.path.join(d, "hypo_grid.density.%s.dat" % nm)).read().split("\n")
        assert lines[0] == lc.STACK_HEADERS[nm] and lines[-1] == "" and len(lines) == res[nm].size + 2
        assert lines[1:-1] == lc.stack_map_text(nm, res[nm], grid, [0.68, 0.95]).split("\n")[1:-1]
        mass = np.array([float(ln.split()[5]) for ln in lines[1:-1]]).reshape(res[nm].shape)
        assert np.all(np.abs(mass - res[nm]) <= 0.5000001e-6 * res[nm] + 1e-300)          # %14.6e: seven significant digits
        level = np.array([float(ln.split()[6]) for ln in lines[1:-1]]).reshape(res[nm].shape)
        assert set(np.unique(level)) <= {0.0, 0.68, 0.95} and (level[res[nm] == 0.0] == 0.0).all()
    out = capsys.readouterr().out
    assert out.startswith(plain_out)
    extra = out[len(plain_out):].split("\n")
    assert len(extra) == 3 and extra[2] == ""
    for L in range(2):
        assert extra[L].startswith(f"layer {L}: {int(res['tally'][L, 0])} windows stacked, 0 without an included cell, ")
        assert extra[L].endswith("of the mass on the faces of the box")
