"""Step 4 (`hypo_tremor_select`): the regressions of src/cls_selector.f90:75-132 / src/mod_regress.f90.

CPU: the oracle restatement against what the COMPILED REFERENCE step 4 wrote (regress.dat, selected_win.dat of
tests/golden/select*.npz, produced under mpiexec by tests/golden/make_golden.py): bit-identical, NaN in place.
select_edges and select_min are constructed windows: rows of NaN and -inf, ties of the largest amplitude, +-0, a
station at depth z_guess, zero errors, +inf; they also record the nearest station the reference chose (maxloc).
GPU: `htm_select_regress` through the C ABI against the same files (1e-10 relative: wave-tree sums instead of serial
ones; NaN and infinities in place), the same windows selected, and the drop-in program
`python -m hypotremormcmc_amd.select` on the reference's input files; k_regress at edge shapes against exact sums."""
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from hypotremormcmc_amd import synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ["select", "select_wide"]
EDGE_CASES = ["select_edges", "select_min"]


def _load(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    pv = dict(zip(fx["param_keys"].tolist(), (float(v) for v in fx["param_vals"])))
    if "in_t" in fx:                    # constructed inputs, stored with the fixture
        data = SimpleNamespace(sta_x=fx["in_sta_x"], sta_y=fx["in_sta_y"], sta_z=fx["in_sta_z"], t_obs=fx["in_t"],
                               t_stdv=fx["in_t_err"], a_obs=fx["in_a"], a_stdv=fx["in_a_err"])
        data.n_events, data.n_sta = data.t_obs.shape
        return fx, data, pv
    E, S = (int(v) for v in fx["in_shape"])
    data = synth.make_synthetic(E, S, int(fx["in_seed"]), 0)
    return fx, data, pv


def _assert_same_nan_and_inf(out, ref):
    """NaN at the same places, the same infinities (sign included) at the same places"""
    assert np.array_equal(np.isnan(out), np.isnan(ref)), np.argwhere(np.isnan(out) != np.isnan(ref))
    assert np.array_equal(np.isinf(out), np.isinf(ref)), np.argwhere(np.isinf(out) != np.isinf(ref))
    assert np.array_equal(out[np.isinf(out)], ref[np.isinf(ref)])


@pytest.mark.parametrize("name", CASES + EDGE_CASES)
def test_oracle_equals_reference_regress_file(name):
    from oracle import oracle

    fx, data, pv = _load(name)
    out = oracle.select_regress(data.sta_x, data.sta_y, data.sta_z, pv["z_guess"], data.t_obs, data.t_stdv, data.a_obs,
                                data.a_stdv)
    assert np.array_equal(fx["regress"][:, 0].astype(int), np.arange(1, data.n_events + 1))
    # bit-exact: same operation order, same libm; NaN where the reference has NaN
    assert np.array_equal(out, fx["regress"][:, 1:], equal_nan=True)
    _assert_same_nan_and_inf(out, fx["regress"][:, 1:])
    from hypotremormcmc_amd.select import select

    keep = select(out, pv["vs_min"], pv["vs_max"], pv["b_min"], pv["b_max"])
    assert np.array_equal(np.flatnonzero(keep) + 1, fx["selected"])


def test_edge_fixtures_cover_the_degenerate_rows():
    """what the fixtures are for: NaN reaches the outputs, and no window with a NaN vs or b is selected"""
    for name in EDGE_CASES:
        fx, data, pv = _load(name)
        reg = fx["regress"][:, 1:]
        assert np.isnan(data.a_obs).all(axis=1).any() and np.isneginf(data.a_obs).all(axis=1).any()
        bad = np.isnan(reg[:, 0]) | np.isnan(reg[:, 1])
        assert bad.any() and not set(np.flatnonzero(bad) + 1) & set(fx["selected"].tolist())
        assert 0 < len(fx["selected"]) < data.n_events


@pytest.mark.parametrize("name", EDGE_CASES)
def test_maxloc_and_initial_guess_take_the_reference_station(name):
    from hypotremormcmc_amd.obs_data import ObsData, maxloc
    from oracle import oracle

    fx, data, pv = _load(name)
    near = fx["nearest"]
    assert np.array_equal(maxloc(data.a_obs), near)
    obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
    x_mu, y_mu = obs.make_initial_guess()
    assert np.array_equal(x_mu, data.sta_x[near]) and np.array_equal(y_mu, data.sta_y[near])
    # the oracle's step-5 set-up centres the hypocentre prior on the same stations (src/cls_obs_data.f90:120-134)
    params = dict(synth.DEFAULT_PARAMS, n_procs=1, n_chains=1)
    job = oracle.Job(params, data)
    mu = job.hypo_priors(0, 0)[0].reshape(-1, 3)
    assert np.array_equal(mu[:, 0], data.sta_x[near]) and np.array_equal(mu[:, 1], data.sta_y[near])


def test_maxloc_rule_rows():
    """the rows probed with the reference's compiler (1-based there, 0-based here), and a few more"""
    from hypotremormcmc_amd.obs_data import maxloc

    nan, inf = float("nan"), float("inf")
    rows = {(nan, 1, 3, 3): 2, (nan, nan, nan, nan): 0, (-inf, -inf, -inf, -inf): 0, (-inf, nan, -1e301, -inf): 2,
            (0, 0, 0, 0): 0, (nan, -inf, -inf): 1, (-0.0, 0.0, -1.0): 0, (0.0, -0.0): 0, (1.0, inf, nan, inf): 1}
    for row, k in rows.items():
        assert maxloc(np.array(row)) == k, row
    assert np.array_equal(maxloc(np.array(list(rows)[:5], dtype=float)), [2, 0, 0, 2, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES + EDGE_CASES)
def test_device_regressions_equal_reference(name):
    from hypotremormcmc_amd.select import regress, select

    fx, data, pv = _load(name)
    out = regress(data.sta_x, data.sta_y, data.sta_z, pv["z_guess"], data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
    _assert_same_nan_and_inf(out, fx["regress"][:, 1:])
    np.testing.assert_allclose(out, fx["regress"][:, 1:], rtol=1e-10, atol=0)
    keep = select(out, pv["vs_min"], pv["vs_max"], pv["b_min"], pv["b_max"])
    assert np.array_equal(np.flatnonzero(keep) + 1, fx["selected"])


@pytest.mark.gpu
def test_select_program_writes_the_reference_files(tmp_path):
    fx, data, pv = _load("select")
    synth.write_dataset(str(tmp_path), data)
    os.rename(tmp_path / "selected_win.dat", tmp_path / "detected_win.dat")
    with open(tmp_path / "select.in", "w") as fh:
        fh.write("n_procs = 1\nstation_file = station_xy.list\n")
        for k, v in pv.items():
            fh.write("%s = %r\n" % (k, v))
    r = subprocess.run([sys.executable, "-m", "hypotremormcmc_amd.select", "select.in"], cwd=tmp_path, timeout=300,
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    reg = np.array([float(x) for x in open(tmp_path / "regress.dat").read().split()]).reshape(-1, 7)
    np.testing.assert_allclose(reg, fx["regress"], rtol=1e-10, atol=0)
    sel = [int(ln.split()[0]) for ln in open(tmp_path / "selected_win.dat") if ln.strip()]
    assert sel == fx["selected"].tolist()


def test_select_parameter_keys_are_required(tmp_path):
    from hypotremormcmc_amd.param import Param, ParamError

    (tmp_path / "station_xy.list").write_text("S001 0.0 0.0 0.0 1.0 1.0\n")
    (tmp_path / "p.in").write_text("n_procs = 1\nstation_file = station_xy.list\nz_guess = 7.0\nvs_min = 2.0\nvs_max = 4.0\nb_min = 0.0\n")
    with pytest.raises(ParamError):
        Param(str(tmp_path / "p.in"), from_where="select")     # b_max missing (src/cls_param.f90:123-126, :294-346)


def test_regress_refuses_arrays_of_other_shapes(monkeypatch):
    """a t_err, a or a_err smaller than t would be read past its end by the C side: refused before the library"""
    from hypotremormcmc_amd import select as sel

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(sel._lib, "load", no_library)
    S, W = 5, 4
    st = np.zeros(S)
    t = np.ones((W, S))
    for k, name in enumerate(("t_err", "a", "a_err")):
        args = [t.copy(), t.copy(), t.copy()]
        args[k] = np.ones((W - 1, S))
        with pytest.raises(ValueError, match="^%s has shape" % name):
            sel.regress(st, st, st, 1.0, t, *args)
        args[k] = np.ones(W * S)                         # the right size, flat
        with pytest.raises(ValueError, match="^%s has shape" % name):
            sel.regress(st, st, st, 1.0, t, *args)
    with pytest.raises(ValueError, match="shape"):
        sel.regress(st, st, st, 1.0, np.ones(S), np.ones(S), np.ones(S), np.ones(S))
    with pytest.raises(ValueError, match="n_sta"):
        sel.regress(np.zeros(S + 1), st, st, 1.0, t, t, t, t)


def test_c_abi_refuses_a_regress_launch_beyond_32_bits():
    """256 work-items per four windows: 2^26 - 3 windows and more need 2^32 work-items.  The guard answers HTM_EINVAL
    before any device call (device -1: past the guard the call fails in the device selection, with tiny buffers)."""
    from hypotremormcmc_amd import _lib
    from hypotremormcmc_amd._lib import dp

    lib = _lib.load()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(dp)
    for n_win in (2 ** 26 - 3, 2 ** 26, 2 ** 31 - 1):
        assert lib.htm_select_regress(-1, 3, n_win, p, p, p, 1.0, p, p, p, p, p) == -1
        assert b"work-items" in lib.htm_last_error(), n_win
    lib.htm_select_regress(-1, 3, 2 ** 26 - 4, p, p, p, 1.0, p, p, p, p, p)
    assert b"work-items" not in lib.htm_last_error() and b"device" in lib.htm_last_error().lower()


# ---- k_regress at the shapes and edges where it could go wrong, against exact sums -------------------------------------
#
# The kernel's per-station terms are formed here in float64 in its own operation order (-ffp-contract=off on both sides),
# so they are the kernel's bits as long as d and log(d) are; 1 ulp is allowed on each device sqrt and 2 on each device log.
# The sums are exact (math.fsum), the few operations after them in long double.  The tolerance is derived per window:
# each sum may differ from the exact one by its association error, at most (ceil(S / 64) + 6) u sum|terms| (a serial sum
# per lane, then six tree levels), plus what the allowed d and log(d) errors move its terms by; that is propagated to the
# six outputs to first order by perturbing one sum (mean, centred sum) at a time by its bound.

U = 2.0 ** -53
LD = np.longdouble


def _spread(f, x, e):
    """f(x) and the first-order bound of |f(x + dx) - f(x)| over |dx_k| <= e_k (one argument at a time, both signs)"""
    f0 = f(x)
    tot = np.zeros_like(f0)
    for k in range(len(x)):
        dev = []
        for s in (1, -1):
            xp = x.copy()
            xp[k] += s * e[k]
            dev.append(np.abs(f(xp) - f0))
        tot += np.maximum(dev[0], dev[1])
    return f0, tot


def _post(s):
    s0, s1, s2, s3, s4, s5, s6, s7, s8, s9 = s
    det_t, det_a = s2 * s4 - s0 * s0, s7 * s9 - s5 * s5
    slope_t, icpt_t = (s2 * s3 - s0 * s1) / det_t, (s4 * s1 - s0 * s3) / det_t
    slope_a, icpt_a = (s7 * s8 - s5 * s6) / det_a, (s9 * s6 - s5 * s8) / det_a
    return np.array([1 / slope_t, -slope_a, icpt_t, icpt_a, s0 / s2, s1 / s2, s5 / s7, s6 / s7], dtype=LD)


def _cc(c):
    return np.array([c[2] / np.sqrt(c[0] * c[1]), c[5] / np.sqrt(c[3] * c[4])], dtype=LD)


def _regress_exact(sx, sy, sz, zg, t, te, a, ae, near):
    """one window -> (the six outputs in long double, their tolerances, the spread of its distances)"""
    S = t.size
    k = math.ceil(S / 64) + 6
    dx, dy, dz = sx - sx[near], sy - sy[near], sz - zg
    d = np.sqrt(dx * dx + dy * dy + dz * dz)
    lg = np.log(d)
    aj = a + lg
    wt, wa = 1.0 / (te * te), 1.0 / (ae * ae)
    terms = [d * wt, t * wt, wt, d * t * wt, d * d * wt, d * wa, aj * wa, wa, d * aj * wa, d * d * wa]
    ed = 2 * U * d                                          # 1 ulp of d
    ea = 4 * U * np.abs(lg) + ed / d + 2 * U * np.abs(aj)   # 2 ulp of log(d), what d's ulp moves it by, a + log d rounding
    moved = [wt * ed, 0 * d, 0 * d, np.abs(t * wt) * ed, 2 * d * wt * ed, wa * ed, wa * ea, 0 * d,
             np.abs(aj * wa) * ed + d * wa * ea, 2 * d * wa * ed]
    s = np.array([math.fsum(x) for x in terms], dtype=LD)
    # association, moved terms, two roundings per term (weight, products), the products the sums enter after the pass
    e = np.array([1.01 * ((k + 2) * U * float(np.sum(np.abs(x))) + float(np.sum(m))) + 4 * U * abs(float(v))
                  for x, m, v in zip(terms, moved, s)], dtype=LD)
    f0, fb = _spread(_post, s, e)
    out = f0[:4]
    tol = 2 * fb[:4] + 4 * U * np.abs(out)
    m = f0[4:]                                              # mx_t, my_t, mx_a, my_a
    em = fb[4:] + U * np.abs(m)                             # ... and the division of each on the device
    x, yt, ya = d.astype(LD), t.astype(LD), aj.astype(LD)
    cxt, cyt, cxa, cya = x - m[0], yt - m[1], x - m[2], ya - m[3]
    ext, eyt = U * np.abs(cxt) + em[0] + ed, U * np.abs(cyt) + em[1]
    exa, eya = U * np.abs(cxa) + em[2] + ed, U * np.abs(cya) + em[3] + ea
    pairs = [(cxt, cxt, ext, ext), (cyt, cyt, eyt, eyt), (cxt, cyt, ext, eyt),
             (cxa, cxa, exa, exa), (cya, cya, eya, eya), (cxa, cya, exa, eya)]
    c = np.array([np.sum(p * q) for p, q, _, _ in pairs], dtype=LD)
    ec = LD(1.01) * np.array([np.sum(np.abs(q) * ep + np.abs(p) * eq + ep * eq) + (k + 2) * U * np.sum(np.abs(p * q))
                              for p, q, ep, eq in pairs], dtype=LD)
    c0, cb = _spread(_cc, c, ec)
    # how far the weighted distances spread: det / (sum w * sum w d^2) of each regression, 0 for a single distance
    spread = min(float((s[2] * s[4] - s[0] * s[0]) / (s[2] * s[4])), float((s[7] * s[9] - s[5] * s[5]) / (s[7] * s[9])))
    return np.concatenate([out, c0]), np.concatenate([tol, 2 * cb + 4 * U * np.abs(c0)]), spread


def _sweep_window(rng, sx, sy, sz, zg, plant, wide):
    """t, t_err, a, a_err of one window, linear in the distance from the planted nearest station min(plant); every index
    of plant gets the same, largest amplitude"""
    j = min(plant)
    dn = np.sqrt((sx - sx[j]) ** 2 + (sy - sy[j]) ** 2 + (sz - zg) ** 2)
    S = sx.size
    t = 5.0 + dn / 3.0 + rng.normal(0.0, 0.05, S)
    a = 2.0 - 0.03 * dn - np.log(dn) + rng.normal(0.0, 0.02, S)
    if wide:                                                # weights 1/err^2 over 1e-4 .. 1e4
        te, ae = 10.0 ** rng.uniform(-2, 2, S), 10.0 ** rng.uniform(-2, 2, S)
    else:
        te, ae = 0.1 * 10.0 ** rng.uniform(-0.3, 0.3, S), 0.05 * 10.0 ** rng.uniform(-0.3, 0.3, S)
    a[list(plant)] = a.max() + 0.5
    return t, te, a, ae


SWEEP_S = [3, 4, 63, 64, 65, 70, 127, 128, 129, 1000]
SWEEP_W = [1, 2, 3, 4, 5, 7, 9, 1001]


def _sweep_launch(rng, S, W, degenerate):
    if degenerate:
        # every station within ~2e-3 of one point and the source 21 below it: all distances within ~1e-4 of each
        # other, the determinants ~1e-8 of their terms
        sx = 10.0 + 2e-3 * rng.uniform(-1, 1, S)
        sy = -5.0 + 2e-3 * rng.uniform(-1, 1, S)
        sz = 1.0 + 2e-3 * rng.uniform(-1, 1, S)
        zg = -20.0
    else:
        sx, sy, sz, zg = rng.uniform(-50, 50, S), rng.uniform(-50, 50, S), rng.uniform(0, 2, S), 6.0
    tops = [j for j in (0, 63, 64, S - 1) if j < S] + ([int(rng.integers(64, S))] if S > 64 else [])
    # ties of the largest amplitude: across lanes with the lower index in the higher lane, and within one lane
    if S > 65:
        ties = [(2, 65), (1, 65), (3, 64), (60, 64 + int(rng.integers(0, 60)))]
    else:
        ties = [(0, S - 1), (1, S - 1), (0, 1)]
    ties = [p for p in ties if max(p) < S]
    rows, plants, kinds = [], [], []
    for w in range(W):
        kind = "degenerate" if degenerate else ("plain", "wide", "tie")[w % 3]
        plant = ties[(w // 3) % len(ties)] if kind == "tie" else (tops[w % len(tops)],)
        rows.append(_sweep_window(rng, sx, sy, sz, zg, plant, kind == "wide"))
        plants.append(min(plant))
        kinds.append(kind)
    t, te, a, ae = (np.array([r[q] for r in rows]) for q in range(4))
    return sx, sy, sz, zg, t, te, a, ae, plants, kinds


def _check_sweep(S, regress):
    """every window of every launch against its own exact reference; -> the number of well-conditioned windows"""
    from hypotremormcmc_amd.obs_data import maxloc

    assert np.finfo(LD).eps < 2.0 ** -60, "long double is no wider than double here"
    rng = np.random.default_rng(1000 + S)
    launches = [(W, False) for W in SWEEP_W if W < 1000 or S <= 70] + [(5, True)]
    n_plain = 0
    for W, degenerate in launches:
        sx, sy, sz, zg, t, te, a, ae, plants, kinds = _sweep_launch(rng, S, W, degenerate)
        near = maxloc(a)
        assert np.array_equal(near, plants)
        out = regress(sx, sy, sz, zg, t, te, a, ae)
        assert out.shape == (W, 6) and np.all(np.isfinite(out))
        for w in range(W):
            ref, tol, spread = _regress_exact(sx, sy, sz, zg, t[w], te[w], a[w], ae[w], int(near[w]))
            err = np.abs(out[w].astype(LD) - ref)
            assert np.all(err <= tol), (S, W, w, kinds[w], out[w], ref.astype(float), err.astype(float), tol.astype(float))
            if kinds[w] == "plain" and spread > 0.1:    # well-conditioned: the tolerance cannot hide an operand mix-up
                assert np.all(tol <= 1e-12 * np.abs(ref)), (S, W, w, (tol / np.abs(ref)).astype(float))
                n_plain += 1
    return n_plain


@pytest.mark.parametrize("S", [3, 65, 1000])
def test_sweep_reference_takes_the_oracle_within_its_tolerance(S):
    """the exact reference and its derived tolerance, checked on the CPU with the oracle's serial sums in place of the
    kernel: the bound holds there too, and is below 1e-12 relative on the well-conditioned windows"""
    from oracle import oracle

    assert _check_sweep(S, oracle.select_regress) >= len(SWEEP_W) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("S", SWEEP_S)
def test_regress_shapes_against_exact_sums(S):
    """k_regress over W in SWEEP_W (1001 only up to 70 stations) and one launch of near-degenerate geometry; maxima
    planted at j = 0, 63, 64, S - 1 and a random j >= 64, ties across and within lanes, weights over eight decades"""
    from hypotremormcmc_amd.select import regress

    assert _check_sweep(S, regress) >= len(SWEEP_W) - 1
