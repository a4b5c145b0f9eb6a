#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the REFERENCE ITSELF (oracle/_ref, built by `make -C oracle ref`).

Runs only in the build container (needs /root/reference for the build and /opt/conda MPICH to run); the
resulting fixtures are data only -- inputs (seeded synthetic data + parameter values) and the reference's
outputs (likelihoodRR.out traces, sample files, proposal_count.txt, direct forward-call known answers,
RNG vectors).  Nothing of the reference's source text is stored.

    python tests/golden/make_golden.py            # regenerate every fixture

Cases
  c1        5 ev x  8 stn, seed 0, 2 ranks x 2 chains, 20000 it   (BASELINE config #1 plumbing case)
  c2      100 ev x 16 stn, seed 2, 1 rank  x 2 chains,  4000 it   (BASELINE config #2; 2 chains: quirk 1)
  missing   6 ev x 10 stn, seed 7, 5 entries with t_stdv = 0, 1 rank x 3 chains (missing-data rule)
  timeonly  8 ev x 12 stn, seed 3, use_amp = F, solve_qs = solve_a_corr = F, 3 ranks x 2 chains
  amponly   8 ev x 12 stn, seed 13, use_time = F, solve_t_corr = F (solve_vs stays T: vs enters the attenuation term),
         4 entries with t_stdv = 0, 3 ranks x 2 chains (run under mpiexec -np 3).  Pins that the missing-data rule stays
         keyed on t_stdv when travel times are unused.
  missing64 9 ev x 64 stn, seed 17, 1 rank x 3 chains, 1500 it; missing entries from an explicit index list
         (`missing_idx`, stored as in_missing_idx): station 0 of event 0, station 63 of event 8, event 4 with every station
         but one missing, station 17 missing in every event, three scattered ones -- 76 entries (the four patterns alone
         take 73).  Full rows of 64 with both data types: the shape of the specialised chain master's packed records.
  fixedcorr 7 ev x  9 stn, seed 4, solve_t_corr = solve_vs = F, 2 ranks x 3 chains, n_cool = 2
  c3     1000 ev x 64 stn, seed 1, 1 rank x 8 chains, 600 it: inputs are NOT stored (2 MB) -- the seeded
         generator reproduces them; a checksum of the inputs is stored instead.
  select, select_wide   step 4 (hypo_tremor_select): 60 windows x 12 stations under 2 ranks, 33 x 70 under 3 ranks
  select_edges, select_min   step 4 on constructed windows (70 and 3 stations): rows of NaN, -inf, ties of the largest
         amplitude, +-0, a station at depth z_guess, zero errors, +inf; each under mpiexec -np 1 and -np 3 (the outputs
         must be identical).  The inputs are stored; so is each window's nearest station, recovered from the
         reference's dist_plot.NNNNNN.dat.
  c4     1000 ev x 64 stn, seed 1, 8 ranks x 8 chains = 64 tempered chains, temp_high = 200, 400 it (BASELINE
         configs[3], run under mpiexec -np 8); inputs as for c3.
  xcorr_overlap, xcorr_gapped   steps 2 and 3 (hypo_tremor_correlate, hypo_tremor_measure) on seeded
         synth.make_tremor_envelopes data, each under mpiexec -np 1 and -np 3 (the outputs must be identical).  These
         two programs are linked with oracle/ref_dft.c in place of FFTW (oracle/Makefile): their values agree with
         an FFTW build's to rounding only.  Inputs are regenerated from the stored generator arguments and checked
         against a stored checksum.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from hypotremormcmc_amd import synth  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "hypo_tremor_mcmc_ref")
PROBE_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_probe")
STATS_BIN = os.path.join(ROOT, "oracle", "_ref", "hypo_tremor_statistics_ref")
STAT_FILES = ("uniform_structure.stat", "station_corrections.stat", "hypo.stat", "hypo.stat.removed")
MPIEXEC = "/opt/conda/bin/mpiexec"
OUT = os.path.dirname(os.path.abspath(__file__))

CASES = {
    "c1": dict(n_events=5, n_sta=8, seed=0, n_missing=0,
               params=dict(n_procs=2, n_chains=2, n_cool=1, n_iter=20000, n_burn=10000, n_interval=100)),
    "c2": dict(n_events=100, n_sta=16, seed=2, n_missing=0,
               params=dict(n_procs=1, n_chains=2, n_cool=1, n_iter=4000, n_burn=2000, n_interval=50)),
    "missing": dict(n_events=6, n_sta=10, seed=7, n_missing=5,
                    params=dict(n_procs=1, n_chains=3, n_cool=1, n_iter=6000, n_burn=1000, n_interval=25)),
    "timeonly": dict(n_events=8, n_sta=12, seed=3, n_missing=0,
                     params=dict(n_procs=3, n_chains=2, n_cool=1, n_iter=6000, n_burn=3000, n_interval=40,
                                 use_amp="F", solve_qs="F", solve_a_corr="F")),
    "amponly": dict(n_events=8, n_sta=12, seed=13, n_missing=4,
                    params=dict(n_procs=3, n_chains=2, n_cool=1, n_iter=6000, n_burn=3000, n_interval=40,
                                use_time="F", solve_t_corr="F", solve_vs="T")),
    "missing64": dict(n_events=9, n_sta=64, seed=17, n_missing=0,
                      missing_idx=([(0, 0), (8, 63)] + [(4, j) for j in range(64) if j != 40] + [(i, 17) for i in range(9)]
                                   + [(2, 31), (2, 32), (6, 5)]),
                      params=dict(n_procs=1, n_chains=3, n_cool=1, n_iter=1500, n_burn=500, n_interval=25)),
    "fixedcorr": dict(n_events=7, n_sta=9, seed=4, n_missing=0,
                      params=dict(n_procs=2, n_chains=3, n_cool=2, n_iter=5000, n_burn=0, n_interval=20,
                                  solve_t_corr="F", solve_vs="F", temp_high="50.0")),
    # depth steps several times the prior width: the Rayleigh prior rejects every few steps (a rejection consumes no
    # judge draw, which shifts everything behind it in the random stream)
    "rejects": dict(n_events=40, n_sta=12, seed=9, n_missing=0,
                    params=dict(n_procs=2, n_chains=4, n_cool=1, n_iter=3000, n_burn=1000, n_interval=10,
                                step_size_z=6.0, step_size_vs=0.4)),
    "c3": dict(n_events=1000, n_sta=64, seed=1, n_missing=0, store_inputs=False,
               params=dict(n_procs=1, n_chains=8, n_cool=1, n_iter=600, n_burn=300, n_interval=10)),
    # BASELINE configs[3]: 64 chains with parallel tempering over 8 ranks (mpiexec -np 8), temp_high = 200
    "c4": dict(n_events=1000, n_sta=64, seed=1, n_missing=0, store_inputs=False,
               params=dict(n_procs=8, n_chains=8, n_cool=1, n_iter=400, n_burn=100, n_interval=10, temp_high="200.0")),
}


def checksum(data) -> str:
    h = hashlib.sha256()
    for a in (data.sta_x, data.sta_y, data.sta_z, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv):
        h.update(np.ascontiguousarray(a, dtype="<f8").tobytes())
    return h.hexdigest()


def read_records(path, n_val):
    dt = np.dtype([("iter", "<i4"), ("val", "<f8", (n_val,))])
    if not os.path.exists(path) or os.path.getsize(path) == 0:
        return np.zeros(0, np.int32), np.zeros((0, n_val))
    a = np.fromfile(path, dtype=dt)
    return a["iter"].copy(), a["val"].reshape(-1, n_val).copy()


def probe(workdir, data, params, n_cases=4):
    """Known answers straight from the reference's cls_forward / mod_random / cls_obs_data."""
    E, S = data.n_events, data.n_sta
    rng = np.random.default_rng(1234 + E + S)
    tf = lambda v: "T" if str(v).upper().startswith("T") else "F"
    cases = []
    with open(os.path.join(workdir, "probe_in.txt"), "w") as f:
        f.write(f"{S} {E} {tf(params.get('use_time', 'T'))} {tf(params.get('use_amp', 'T'))} {n_cases}\n")
        for arr in (data.sta_x, data.sta_y, data.sta_z):
            f.write(" ".join("%.17g" % v for v in arr) + "\n")
        for k in range(n_cases):
            hypo = data.ev_xyz + rng.normal(0, 2.0, data.ev_xyz.shape)
            hypo[:, 2] = np.abs(hypo[:, 2]) + 0.5
            hypo = hypo.reshape(-1)
            tc = rng.normal(0, 0.3, S)
            ac = rng.normal(0, 0.02, S)
            vs = 3.0 + rng.normal(0, 0.3)
            qs = 250.0 + rng.normal(0, 40.0)
            evt = int(rng.integers(1, E + 1))
            xyz = hypo[3 * (evt - 1):3 * evt] + rng.normal(0, 1.0, 3)
            xyz[2] = abs(xyz[2]) + 0.1
            cases.append(dict(hypo=hypo, t_corr=tc, a_corr=ac, vs=vs, qs=qs, evt_id=evt, xyz=xyz))
            f.write(" ".join("%.17g" % v for v in hypo) + "\n")
            f.write(" ".join("%.17g" % v for v in tc) + "\n")
            f.write("%.17g\n" % vs)
            f.write(" ".join("%.17g" % v for v in ac) + "\n")
            f.write("%.17g\n" % qs)
            f.write("%d\n" % evt)
            f.write(" ".join("%.17g" % v for v in xyz) + "\n")
    subprocess.check_call([PROBE_BIN], cwd=workdir, stdout=subprocess.DEVNULL)
    toks = open(os.path.join(workdir, "probe_out.txt")).read().split()
    pos = 0
    out = {}
    rngv = np.empty((4, 12))
    for r in range(4):
        assert toks[pos] == "rng" and toks[pos + 1] == "rank"
        pos += 3
        rngv[r] = [float(t) for t in toks[pos:pos + 12]]
        pos += 12
    out["probe_rng"] = rngv
    assert toks[pos] == "initial_guess"
    pos += 1
    out["probe_xy_mu"] = np.array([float(t) for t in toks[pos:pos + 2 * E]]).reshape(E, 2)
    pos += 2 * E
    L = np.empty((n_cases, 3))
    for k in range(n_cases):
        assert toks[pos] == "case"
        pos += 2
        L[k] = [float(t) for t in toks[pos:pos + 3]]
        pos += 3
        if k == 0:
            for name, n in (("t_syn", S * E), ("a_syn", S * E), ("t_syn_single", S), ("a_syn_single", S)):
                assert toks[pos] == name, (toks[pos], name)
                pos += 1
                out["probe_" + name] = np.array([float(t) for t in toks[pos:pos + n]])
                pos += n
    out["probe_L"] = L
    for key in ("hypo", "t_corr", "a_corr", "xyz"):
        out["probe_in_" + key] = np.array([c[key] for c in cases])
    out["probe_in_vs"] = np.array([c["vs"] for c in cases])
    out["probe_in_qs"] = np.array([c["qs"] for c in cases])
    out["probe_in_evt_id"] = np.array([c["evt_id"] for c in cases], dtype=np.int32)
    return out


def run_case(name, spec):
    data = synth.make_synthetic(spec["n_events"], spec["n_sta"], spec["seed"], spec["n_missing"])
    missing_idx = np.array(sorted(set(spec.get("missing_idx", []))), dtype=np.int64).reshape(-1, 2)
    data.t_stdv[missing_idx[:, 0], missing_idx[:, 1]] = 0.0      # (event, station) pairs set by hand
    work = tempfile.mkdtemp(prefix="htm_golden_")
    try:
        synth.write_dataset(work, data)
        params = synth.write_param_file(os.path.join(work, "run.in"), **spec["params"])
        n_procs = int(params["n_procs"])
        subprocess.check_call([MPIEXEC, "-np", str(n_procs), REF_BIN, "run.in"], cwd=work,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        E, S = data.n_events, data.n_sta
        fx = {}
        for r in range(n_procs):
            it, v = read_records(os.path.join(work, "likelihood%02d.out" % r), 1)
            fx[f"lik_iter_{r}"] = it
            fx[f"lik_{r}"] = v[:, 0]
            for nm, nv in (("vs", 1), ("qs", 1), ("t_corr", S), ("a_corr", S), ("hypo", 3 * E)):
                it, v = read_records(os.path.join(work, "%s.%02d.out" % (nm, r)), nv)
                if not spec.get("store_inputs", True) and nm == "hypo":
                    keep = 2 if n_procs == 1 else (1 if r in (0, n_procs - 1) else 0)
                    v = v[len(v) - keep:]  # keep the fixture small: the last hypocentre sample(s) only, of the outer ranks
                    it = it[len(it) - keep:]
                fx[f"{nm}_iter_{r}"] = it
                fx[f"{nm}_{r}"] = v
        # step 6 of the reference on the files step 5 just wrote: the four .stat files, as text.
        # Needs il = int(0.025 * n_mod) >= 1, i.e. n_mod >= 40 (below that the reference indexes element 0).
        p_ = {k: int(params[k]) for k in ("n_iter", "n_burn", "n_procs", "n_cool", "n_interval")}
        n_mod = (p_["n_iter"] - p_["n_burn"]) * p_["n_procs"] * p_["n_cool"] // p_["n_interval"]
        if n_mod >= 40:
            # step 6 reads its parameter file in the step-4 ("select") mode, which insists on five keys it never uses
            with open(os.path.join(work, "stats.in"), "w") as fh:
                fh.write(open(os.path.join(work, "run.in")).read())
                fh.write("z_guess = 7.0\nvs_min = 2.0\nvs_max = 4.0\nb_min = 0.0\nb_max = 1.0\n")
            subprocess.check_call([MPIEXEC, "-np", str(n_procs), STATS_BIN, "stats.in"], cwd=work,
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            for fn in STAT_FILES:
                fx["stat_" + fn.replace(".", "_")] = np.array(open(os.path.join(work, fn)).read())
            fx["stat_n_mod"] = np.array(n_mod)
        rows = [ln.split('"') for ln in open(os.path.join(work, "proposal_count.txt"))]
        fx["count_labels"] = np.array([r[1] for r in rows])
        fx["n_propose"] = np.array([int(r[2].split()[0]) for r in rows], dtype=np.int64)
        fx["n_accept"] = np.array([int(r[2].split()[1]) for r in rows], dtype=np.int64)
        if spec.get("store_inputs", True):
            fx.update(probe(work, data, params))
            for key in ("sta_x", "sta_y", "sta_z", "t_obs", "t_stdv", "a_obs", "a_stdv", "ev_xyz"):
                fx["in_" + key] = getattr(data, key)
        fx["in_checksum"] = np.array(checksum(data))
        fx["in_seed"] = np.array(spec["seed"])
        fx["in_n_missing"] = np.array(spec["n_missing"])
        if len(missing_idx):
            fx["in_missing_idx"] = missing_idx
        fx["in_shape"] = np.array([E, S])
        fx["param_keys"] = np.array(list(params.keys()))
        fx["param_vals"] = np.array([str(v) for v in params.values()])
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **fx)
        print(name, "ok:", {k: (v.shape if hasattr(v, "shape") else v) for k, v in fx.items()
                            if k.startswith("lik_") and not k.startswith("lik_iter")})
    finally:
        shutil.rmtree(work, ignore_errors=True)


SELECT_BIN = os.path.join(ROOT, "oracle", "_ref", "hypo_tremor_select_ref")
SELECT_CASES = {
    # step 4 (hypo_tremor_select) of the reference on detected windows: regress.dat + selected_win.dat
    "select": dict(n_events=60, n_sta=12, seed=21, n_procs=2, z_guess=8.0, vs_min=2.6, vs_max=3.4, b_min=0.0, b_max=0.05),
    "select_wide": dict(n_events=33, n_sta=70, seed=22, n_procs=3, z_guess=5.0, vs_min=2.9, vs_max=3.1, b_min=0.01, b_max=0.03),
}


def run_select_case(name, spec):
    """Reference step 4, unmodified, under mpiexec: inputs = the seeded synthetic opt_data files (the step-5 inputs),
    outputs = regress.dat rows {id, vs, b, t0, a0, cc_t, cc_a} and the selected window ids."""
    data = synth.make_synthetic(spec["n_events"], spec["n_sta"], spec["seed"], 0)
    work = tempfile.mkdtemp(prefix="htm_golden_sel_")
    try:
        synth.write_dataset(work, data)
        shutil.copy(os.path.join(work, "selected_win.dat"), os.path.join(work, "detected_win.dat"))
        os.remove(os.path.join(work, "selected_win.dat"))
        keys = ("z_guess", "vs_min", "vs_max", "b_min", "b_max")
        with open(os.path.join(work, "select.in"), "w") as fh:
            fh.write("n_procs = %d\nstation_file = station_xy.list\n" % spec["n_procs"])
            for k in keys:
                fh.write("%s = %r\n" % (k, spec[k]))
        subprocess.check_call([MPIEXEC, "-np", str(spec["n_procs"]), SELECT_BIN, "select.in"], cwd=work,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        # list-directed output wraps its records over lines: 7 numbers per window
        reg = np.array([float(x) for x in open(os.path.join(work, "regress.dat")).read().split()]).reshape(-1, 7)
        sel = [int(ln.split()[0]) for ln in open(os.path.join(work, "selected_win.dat")) if ln.strip()]
        assert 0 < len(sel) < len(reg), (len(sel), len(reg))       # the thresholds split the set
        fx = dict(regress=reg, selected=np.array(sel, dtype=np.int32), in_checksum=np.array(checksum(data)),
                  in_seed=np.array(spec["seed"]), in_shape=np.array([spec["n_events"], spec["n_sta"]]),
                  param_keys=np.array(list(keys)), param_vals=np.array([spec[k] for k in keys]))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **fx)
        print(name, "ok:", reg.shape, "selected", len(sel))
    finally:
        shutil.rmtree(work, ignore_errors=True)


EDGE_CASES = {
    # step 4 on windows built for maxloc's edges and the NaN / inf paths; 70 stations: lanes 0-5 of a wave hold two each
    "select_edges": dict(n_sta=70, seed=31, z_guess=1.25, z_station=17, vs_min=0.5, vs_max=50.0, b_min=-1.0, b_max=1.0),
    # 3 stations, the fewest htm_select_regress takes
    "select_min": dict(n_sta=3, seed=32, z_guess=0.75, z_station=2, vs_min=0.5, vs_max=50.0, b_min=-1.0, b_max=1.0),
}


def edge_rows(S, kz):
    """[(label, nearest station as the reference's maxloc rule gives it, edit of one window's t, t_err, a, a_err)]"""
    def top(*js):                       # the same maximum at every j of js
        def f(t, te, a, ae):
            m = a.max() + 0.5
            a[list(js)] = m
        return f

    def fill(*pairs):                   # (index or slice, value) in order
        def f(t, te, a, ae):
            for ix, v in pairs:
                a[ix] = v
        return f

    def both(f, g):
        return lambda *x: (f(*x), g(*x))

    def zero_amp(t, te, a, ae):
        a[:] = 0.0
        ae[:] = 0.0

    def signed_zeros(j0, j1):
        def f(t, te, a, ae):
            a[:] = -(np.abs(a) + 0.1)
            a[j0] = -0.0
            a[j1] = 0.0
        return f

    def t_err_zero(j):
        def f(t, te, a, ae):
            te[j] = 0.0
        return f

    nan, inf = float("nan"), float("inf")
    if S < 64:                          # the small case: every station in its own lane
        return [("all NaN", 0, fill((slice(None), nan))),
                ("a[0] NaN, maximum at 2", 2, both(top(2), fill((0, nan)))),
                ("a[0] NaN, the rest -inf", 1, fill((slice(None), -inf), (0, nan))),
                ("all -inf", 0, fill((slice(None), -inf))),
                ("-inf, NaN, -1e301", 2, fill((0, -inf), (1, nan), (2, -1e301))),
                ("amplitudes and their errors 0", 0, zero_amp),
                ("equal maxima at 0 and 2", 0, top(0, 2)),
                ("-0.0 at 0, +0.0 at 1", 0, signed_zeros(0, 1)),
                ("maximum at the station at depth z_guess", kz, top(kz)),
                ("maximum at 1, t_err 0 at 0", 1, both(top(1), t_err_zero(0))),
                ("+inf at 1", 1, fill((1, inf))),
                ("maximum at 0", 0, top(0))]
    mix = fill((slice(0, None, 3), -inf), (slice(1, None, 3), nan), (slice(2, None, 3), -1e302), (40, -1e301))
    return [("all NaN", 0, fill((slice(None), nan))),
            ("a[0] NaN, maximum at 66", 66, both(top(66), fill((0, nan)))),
            ("a[0] NaN, the rest -inf", 1, fill((slice(None), -inf), (0, nan))),
            ("all -inf", 0, fill((slice(None), -inf))),
            ("-inf / NaN / -1e302, maximum -1e301 at 40", 40, mix),
            ("amplitudes and their errors 0", 0, zero_amp),
            ("equal maxima at 2 and 65", 2, top(2, 65)),
            ("equal maxima at 1 and 65", 1, top(1, 65)),
            ("equal maxima at 3 and 64", 3, top(3, 64)),
            ("-0.0 at 5, +0.0 at 9, the rest negative", 5, signed_zeros(5, 9)),
            ("maximum at the station at depth z_guess", kz, top(kz)),
            ("maximum at 30, t_err 0 at 11", 30, both(top(30), t_err_zero(11))),
            ("+inf at 20", 20, fill((20, inf))),
            ("maximum at 0", 0, top(0)),
            ("maximum at 63", 63, top(63)),
            ("maximum at 64", 64, top(64)),
            ("maximum at 69", 69, top(69))]


def edge_inputs(spec):
    """generic, distinct stations (one at depth z_guess) and per-window t, t_err, a, a_err edited per edge_rows"""
    S, kz, zg = spec["n_sta"], spec["z_station"], spec["z_guess"]
    rng = np.random.default_rng(spec["seed"])
    sx, sy, sz = rng.uniform(-50.0, 50.0, S), rng.uniform(-50.0, 50.0, S), rng.uniform(0.0, 2.0, S)
    sz[kz] = zg
    rows = edge_rows(S, kz)
    W = len(rows)
    ev = np.stack([rng.uniform(-40.0, 40.0, W), rng.uniform(-40.0, 40.0, W), rng.uniform(3.0, 15.0, W)], axis=1)
    d = np.sqrt((ev[:, None, 0] - sx) ** 2 + (ev[:, None, 1] - sy) ** 2 + (ev[:, None, 2] - sz) ** 2)
    t = 5.0 + d / 3.0 + rng.normal(0.0, 0.1, (W, S))
    a = 2.0 - 0.03 * d - np.log(d) + rng.normal(0.0, 0.05, (W, S))
    t_err, a_err = rng.uniform(0.05, 0.2, (W, S)), rng.uniform(0.02, 0.1, (W, S))
    for w, (_, _, edit) in enumerate(rows):
        edit(t[w], t_err[w], a[w], a_err[w])
    return sx, sy, sz, t, t_err, a, a_err, rows


def nearest_from_dist_plot(path, sx, sy, sz, zg):
    """the station whose distances reproduce the first column of the reference's dist_plot.NNNNNN.dat"""
    col = np.array([float(v) for v in open(path).read().split()]).reshape(sx.size, 5)[:, 0]
    hits = [k for k in range(sx.size)
            if np.array_equal(np.sqrt((sx - sx[k]) * (sx - sx[k]) + (sy - sy[k]) * (sy - sy[k]) + (sz - zg) * (sz - zg)), col)]
    assert len(hits) == 1, (path, hits)
    return hits[0]


def run_edge_once(work, spec, inputs, n_procs):
    """reference step 4 under mpiexec -np n_procs -> regress rows, selected ids, nearest station per window (0-based)"""
    sx, sy, sz, t, t_err, a, a_err, rows = inputs
    S, W = sx.size, t.shape[0]
    with open(os.path.join(work, "station_xy.list"), "w") as f:
        for j in range(S):
            f.write("S%03d %.17g %.17g %.17g 1.0 1.0\n" % (j + 1, sx[j], sy[j], sz[j]))
    with open(os.path.join(work, "detected_win.dat"), "w") as f:
        for w in range(W):
            f.write("%d %.1f\n" % (w + 1, 150.0 * w))
    for w in range(W):
        with open(os.path.join(work, "opt_data.%06d.dat" % (w + 1)), "w") as f:
            for j in range(S):
                f.write("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n" % (sx[j], sy[j], sz[j], t[w, j], t_err[w, j], a[w, j], a_err[w, j]))
    keys = ("z_guess", "vs_min", "vs_max", "b_min", "b_max")
    with open(os.path.join(work, "select.in"), "w") as fh:
        fh.write("n_procs = %d\nstation_file = station_xy.list\n" % n_procs)
        for k in keys:
            fh.write("%s = %r\n" % (k, spec[k]))
    subprocess.check_call([MPIEXEC, "-np", str(n_procs), SELECT_BIN, "select.in"], cwd=work,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    reg = np.array([float(x) for x in open(os.path.join(work, "regress.dat")).read().split()]).reshape(-1, 7)
    sel = [int(ln.split()[0]) for ln in open(os.path.join(work, "selected_win.dat")) if ln.strip()]
    near = [nearest_from_dist_plot(os.path.join(work, "dist_plot.%06d.dat" % (w + 1)), sx, sy, sz, spec["z_guess"])
            for w in range(W)]
    return reg, sel, near


def run_edge_case(name, spec):
    """Reference step 4, unmodified, on constructed degenerate windows under 1 and 3 ranks (outputs must be equal, NaN
    equal to NaN).  Stored: the inputs, regress.dat rows, the selected ids, and each window's nearest station as the
    reference's own dist_plot file shows it."""
    inputs = edge_inputs(spec)
    outs = []
    for n_procs in (1, 3):
        work = tempfile.mkdtemp(prefix="htm_golden_edge_")
        try:
            outs.append(run_edge_once(work, spec, inputs, n_procs))
        finally:
            shutil.rmtree(work, ignore_errors=True)
    (reg, sel, near), (reg3, sel3, near3) = outs
    assert np.array_equal(reg[:, :5], reg3[:, :5], equal_nan=True) and sel == sel3 and near == near3, "1 and 3 ranks differ"
    # The reference zeroes vs, b, t0 and a0 before its MPI_SUM reduction but not cc_t and cc_a
    # (src/hypo_tremor_select.f90:71-80): under several ranks those two columns also carry what the other ranks'
    # untouched arrays happened to hold.  The 1-rank run is stored; the 3-rank one must equal it wherever it is not NaN.
    cc, cc3 = reg[:, 5:], reg3[:, 5:]
    assert np.all((cc == cc3) | np.isnan(cc3)), "cc columns of 1 and 3 ranks differ beyond the reference's NaN"
    if np.any(np.isnan(cc3) & ~np.isnan(cc)):
        print(name, "3 ranks: NaN from the reference's uninitialised cc arrays at", np.argwhere(np.isnan(cc3) & ~np.isnan(cc)).tolist())
    sx, sy, sz, t, t_err, a, a_err, rows = inputs
    assert near == [r[1] for r in rows], (near, [r[1] for r in rows])     # the rule DESIGN.md §3.3 states
    assert np.array_equal(reg[:, 0], np.arange(1, len(rows) + 1))
    assert 0 < len(sel) < len(rows), sel
    keys = ("z_guess", "vs_min", "vs_max", "b_min", "b_max")
    fx = dict(regress=reg, selected=np.array(sel, dtype=np.int32), nearest=np.array(near, dtype=np.int32),
              labels=np.array([r[0] for r in rows]), in_sta_x=sx, in_sta_y=sy, in_sta_z=sz, in_t=t, in_t_err=t_err,
              in_a=a, in_a_err=a_err, param_keys=np.array(list(keys)), param_vals=np.array([spec[k] for k in keys]))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **fx)
    print(name, "ok:", reg.shape, "selected", sel, "nearest", near)


CORRELATE_BIN = os.path.join(ROOT, "oracle", "_ref", "hypo_tremor_correlate_ref")
MEASURE_BIN = os.path.join(ROOT, "oracle", "_ref", "hypo_tremor_measure_ref")
XCORR_CASES = {
    # overlapping windows (n_step = n / 2), noise, three bursts; the taper is active (nleng = 3)
    "xcorr_overlap": dict(gen=dict(n_sta=5, n_win=40, n=64, n_step=32, burst_win=[5, 14, 27], delay=[0, 2, -1, 3, 1],
                                   log_amp=[0.0, 0.3, -0.2, 0.1, -0.4], noise=0.3, width=3.0, burst_amp=10.0,
                                   level=1.0, dt=1.0, seed=11),
                          alpha=0.99, n_pair_thred=5),
    # gapped windows (n_step > n), dt = 0.5; the delays have a mean of half a sample, so every t of a burst window
    # falls on +-0.5 dt, +-1.5 dt, +-2.5 dt: step 3's nint(t / dt) rounds half away from zero
    "xcorr_gapped": dict(gen=dict(n_sta=6, n_win=24, n=50, n_step=70, burst_win=[6, 17], delay=[0, 1, 2, 3, -2, -1],
                                  log_amp=[0.0, -0.3, 0.2, 0.4, -0.1, 0.25], noise=0.1, width=2.5, burst_amp=10.0,
                                  level=1.0, dt=0.5, seed=12),
                         alpha=0.995, n_pair_thred=10),
}


def xcorr_envelopes(gen):
    """the case's envelopes, regenerated from its generator arguments"""
    return synth.make_tremor_envelopes(**gen)


def xcorr_checksum(env) -> str:
    return hashlib.sha256(np.ascontiguousarray(env.amps, dtype="<f8").tobytes()).hexdigest()


def run_xcorr_once(work, env, spec, n_procs):
    """reference steps 2 and 3 under mpiexec -np n_procs in a fresh directory -> {file name: bytes}"""
    g = spec["gen"]
    synth.write_envelopes(work, env, n_procs=n_procs, t_win_corr=repr(g["n"] * g["dt"]),
                          t_step_corr=repr(g["n_step"] * g["dt"]), alpha=repr(spec["alpha"]),
                          n_pair_thred=spec["n_pair_thred"])
    for exe in (CORRELATE_BIN, MEASURE_BIN):
        subprocess.check_call([MPIEXEC, "-np", str(n_procs), exe, "tremor.in"], cwd=work,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return {f: open(os.path.join(work, f), "rb").read() for f in sorted(os.listdir(work))
            if f.endswith((".corr", ".max_corr")) or f in ("cc_thred.dat", "detected_win.dat") or f.startswith("opt_data.")}


def run_xcorr_case(name, spec):
    """Reference steps 2 and 3, unmodified but for the FFT stand-in.  Stored: cc [n_win][n_pair][n] (the .corr
    values, the reference's lag order), cc_max [n_win][n_pair], the thresholds as the .corr element of rank
    int(n*n_win*alpha) and as printed in cc_thred.dat, the detected window ids and times, and every detected window's
    opt_data columns [n_det][n_sta][7] (x y z t t_stdv amp amp_stdv)."""
    g = spec["gen"]
    env = xcorr_envelopes(g)
    S, n, n_win = g["n_sta"], g["n"], g["n_win"]
    assert np.min(env.amps) > 0.0           # no zero-energy window: the reference's stale buffer depends on the ranks
    outs = []
    for n_procs in (1, 3):
        work = tempfile.mkdtemp(prefix="htm_golden_xc_")
        try:
            outs.append(run_xcorr_once(work, env, spec, n_procs))
        finally:
            shutil.rmtree(work, ignore_errors=True)
    assert outs[0] == outs[1], "reference steps 2 and 3 differ between 1 and 3 ranks"
    files = outs[0]
    stn = env.stations
    prs = [(stn[i], stn[j]) for i in range(S - 1) for j in range(i + 1, S)]
    cc = np.empty((n_win, len(prs), n))
    cc_max = np.empty((n_win, len(prs)))
    for p, (a, b) in enumerate(prs):
        v = np.frombuffer(files[f"{a}.{b}.corr"], dtype="<f8").reshape(n_win, n, 3)
        cc[:, p] = v[:, :, 2]
        cc_max[:, p] = np.frombuffer(files[f"{a}.{b}.max_corr"], dtype="<f8").reshape(n_win, 2)[:, 1]
    rank = int(n * n_win * spec["alpha"])
    thred = np.array([np.sort(cc[:, p].ravel())[rank - 1] for p in range(len(prs))])
    # list-directed output: whitespace-separated tokens, lines wrapped wherever the compiler likes
    tok = files["cc_thred.dat"].decode().split()
    assert tok[0::3] == [a for a, _ in prs] and tok[1::3] == [b for _, b in prs]
    thred_text = np.array([float(t) for t in tok[2::3]])
    assert np.all(np.abs(thred_text - thred) <= 4 * np.spacing(thred)), (thred_text - thred)
    tok = files["detected_win.dat"].decode().split()
    det = np.array([int(t) for t in tok[0::2]], dtype=np.int32)
    det_time = np.array([float(t) for t in tok[1::2]])
    assert set(g["burst_win"]) <= set(det.tolist()) and len(det) < n_win, det
    opt = np.array([[float(t) for t in files["opt_data.%06d.dat" % w].decode().split()] for w in det]).reshape(-1, S, 7)
    if name == "xcorr_gapped":
        frac = np.abs(opt[:, :, 3] / g["dt"]) % 1.0
        assert np.any(frac == 0.5), "no t on a half sample"
    first = f"{prs[0][0]}.{prs[0][1]}"
    fx = dict(cc=cc, cc_max=cc_max, thred=thred, thred_text=thred_text, thred_rank=np.array(rank), detected=det,
              detected_time=det_time, opt=opt,
              corr0_sha256=np.array(hashlib.sha256(files[first + ".corr"]).hexdigest()),
              max_corr0_sha256=np.array(hashlib.sha256(files[first + ".max_corr"]).hexdigest()),
              in_checksum=np.array(xcorr_checksum(env)),
              in_gen_keys=np.array(list(g.keys())), in_gen_vals=np.array([repr(v) for v in g.values()]),
              alpha=np.array(spec["alpha"]), n_pair_thred=np.array(spec["n_pair_thred"]))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **fx)
    print(name, "ok: detected", det.tolist(), "threshold rank", rank)


if __name__ == "__main__":
    if not all(os.path.exists(b) for b in (REF_BIN, PROBE_BIN, STATS_BIN, SELECT_BIN, CORRELATE_BIN, MEASURE_BIN)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    for nm in (sys.argv[1:] or list(CASES) + list(SELECT_CASES) + list(EDGE_CASES) + list(XCORR_CASES)):
        if nm in SELECT_CASES:
            run_select_case(nm, SELECT_CASES[nm])
        elif nm in EDGE_CASES:
            run_edge_case(nm, EDGE_CASES[nm])
        elif nm in XCORR_CASES:
            run_xcorr_case(nm, XCORR_CASES[nm])
        else:
            run_case(nm, CASES[nm])
