"""GPU: the fp32-forward / fp64-accept mode (BASELINE configs[4]: 10 000 events x 128 stations, fp32 forward with
fp64 accept; htm_forward_set_precision).

The reference is fp64 throughout (src/cls_forward.f90), so this mode has no bit-level oracle.  Its arithmetic is pinned term by
term against a numpy.longdouble restatement of the mode itself (T7 - T9 below, tests/fp32_restatement.py); what the mode costs a
sampler is a STATISTICAL tolerance, stated here (T1 - T6).  What is single precision: the synthetic travel time and amplitude of a
station-event pair (distance, sqrt, division, log; src/cls_forward.f90:115-118, :201-204) and the stored
observations.  What stays fp64: coordinate differences, the weighted demean sums (:125-132), residuals, the misfit
sum (:281-299), the Metropolis decision (src/cls_mcmc.f90:194-199) -- checked against the fp64 oracle:

  T1  full log-likelihood: |L32 - L64| <= 3e-6 |L64|                    (random models, 1 000 x 64 and 10 000 x 128)
  T2  single-event update: the ERROR of the log-likelihood difference a proposal is judged on,
      e = (L32_new - L32_old) - (L64_new - L64_old), has |mean| <= 2e-3, rms <= 1e-2 over random proposals with
      the sample file's step sizes -- three to four orders below the differences themselves (rms ~ 10) --
  T3  and flips fewer than 0.5 % of Metropolis decisions made with common random numbers;
  T4  chains: over a few hundred iterations at the configs[4] per-GPU shape (16 chains) the fp32 and the fp64 run
      accept the same number of proposals per type within 4 binomial sigma + 2 % and their cold chains'
      log-likelihoods agree to 2e-3 relative.
  T5  near the posterior: a model within one (small) step of the truth, proposals of 0.05 km -- the differences judged are of
      order one, where a 5e-4 error can reach a Metropolis comparison: over 10 000 proposals with common random numbers fewer
      than 0.2 % of the decisions differ, and the error keeps T2's bounds;
  T6  posterior level, the only tolerance that means something for a sampler: the same job run with the fp64 forward, with the
      fp64 forward and other random seeds, and with the fp32 forward; medians and 2.5 % / 97.5 % points of EVERY parameter from
      the device's step-6 statistics (htm_quantiles).  The fp32 run differs from the fp64 run by no more than two fp64 runs
      with different seeds differ from each other (in units of each parameter's posterior width): rms <= 1.3 x + 0.05 -- both
      with the first run's seeds (common random numbers: the runs part only where a decision flips) and with the other seeds.
  T7  term level (tests/test_gpu_fp32_terms.py): full, stacked and one-event values against the mode's definition in
      numpy.longdouble on the inputs as the library stores them, |L - L_ref| <= ULPS32 * 2^-24 * D32 + 16 * 2^-53 * M, D32 the
      first-order sensitivity of L to one rounding of every synthetic's terms, M the magnitudes of L's terms; ULPS32 = 4 measured on
      the CPU from the documented arithmetic alone (tests/test_fp32_restatement.py), where coordinates rounded to float before the
      difference, a sqrt 4 ulp high and a neighbour's correction exceed it -- T1 is relative to |L|, which is not what the error
      scales with, and passes the first of them; pair probes put an event's weight on two stations so that L resolves single
      synthetics;
  T8  exact translation: coordinates on a 2^-16 km grid shifted by 2^12 and 2^20 km give the same bits, in fp32 and in fp64
      (the coordinate differences stay fp64);
  T9  ragged shapes: every n_sta <= 128 chunk shape x 1, 5, 37 events, 1001 x 64, 4099 x 70 and the single-type modes with missing
      entries at T7 and T1, the refusal above 128 stations and the switch fp32 -> fp64 -> fp32 (same file); every chain loop with
      the fp32 forward at ragged rows against the oracle's decisions (tests/test_gpu_data_modes.py).
The measured values are written to gpurun_out/fp32_tolerances.txt."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _note(line):
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "fp32_tolerances.txt"), "a") as fh:
            fh.write(line + "\n")
    except OSError:
        pass


def _forwards(data):
    from hypotremormcmc_amd.forward import Forward
    from hypotremormcmc_amd.obs_data import ObsData

    obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
    kw = dict(n_sta=data.n_sta, n_events=data.n_events, sta_x=data.sta_x, sta_y=data.sta_y, sta_z=data.sta_z, obs=obs)
    return Forward(**kw), Forward(forward_precision="fp32", **kw)


def _model(data, rng):
    hypo = data.ev_xyz + rng.normal(0, 1.5, data.ev_xyz.shape)
    hypo[:, 2] = np.abs(hypo[:, 2]) + 0.5
    return (hypo.reshape(-1), rng.normal(0, 0.2, data.n_sta), 3.0 + rng.normal(0, 0.2), rng.normal(0, 0.02, data.n_sta),
            250.0 + rng.normal(0, 30.0))


@pytest.mark.parametrize("E,S,seed", [(1000, 64, 1), (10000, 128, 5)])
def test_fp32_full_and_partial_likelihood_against_fp64(E, S, seed):
    from hypotremormcmc_amd import synth
    from oracle import oracle

    data = synth.make_synthetic(E, S, seed)
    f64, f32 = _forwards(data)
    orc = oracle.Forward(data.sta_x, data.sta_y, data.sta_z, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv, True, True)
    rng = np.random.default_rng(100 + seed)
    # ---- T1
    worst = 0.0
    for _ in range(4):
        h, tc, vs, ac, qs = _model(data, rng)
        L64, L32 = f64.calc_log_likelihood(h, tc, vs, ac, qs), f32.calc_log_likelihood(h, tc, vs, ac, qs)
        Lo = orc.calc_log_likelihood(h, tc, vs, ac, qs)
        assert abs(L64 - Lo) <= 1e-9 * abs(Lo)      # (the oracle's serial sum drifts ~1e-10 at 1.3 M terms)
        worst = max(worst, abs(L32 - Lo) / abs(Lo))
    _note(f"T1 {E}x{S}: max |L32 - L64| / |L64| = {worst:.3e}")
    assert worst <= 3e-6
    # ---- T2, T3: proposals of the sample file's step sizes (0.4 km horizontal, 0.4 km depth), common random numbers
    h, tc, vs, ac, qs = _model(data, rng)
    L0 = orc.calc_log_likelihood(h, tc, vs, ac, qs)
    n = 400
    err, dL = np.empty(n), np.empty(n)
    for k in range(n):
        evt = int(rng.integers(1, E + 1))
        h2 = h.copy()
        h2[3 * (evt - 1) + int(rng.integers(0, 3))] += rng.normal(0, 0.4)
        d64 = orc.partially_update_log_likelihood(evt, h, L0, h2, tc, vs, ac, qs) - L0
        d32 = f32.partially_update_log_likelihood(evt, h, L0, h2, tc, vs, ac, qs) - L0
        d64g = f64.partially_update_log_likelihood(evt, h, L0, h2, tc, vs, ac, qs) - L0
        assert abs(d64g - d64) <= 1e-9 * max(1.0, abs(d64)) + 1e-6     # L0 ~ 1e6: the difference carries ~1e-10 of it
        err[k], dL[k] = d32 - d64, d64
    logr = np.log(rng.uniform(size=n))
    flips = np.mean((logr <= dL) != (logr <= dL + err))
    _note(f"T2 {E}x{S}: error of the judged difference: mean {err.mean():.3e} rms {np.sqrt((err ** 2).mean()):.3e} max {np.abs(err).max():.3e}; "
          f"differences rms {np.sqrt((dL ** 2).mean()):.3e}; T3 decision flips {flips:.4f}")
    assert abs(err.mean()) <= 2e-3 and np.sqrt((err ** 2).mean()) <= 1e-2
    assert flips <= 0.005


def test_fp32_decisions_near_the_posterior():
    """T5: where |dL| ~ 1 (src/cls_mcmc.f90:193-203 compares log r with dL / T + prior ratio)"""
    from hypotremormcmc_amd import synth
    from oracle import oracle

    E, S = 1000, 64
    data = synth.make_synthetic(E, S, 1)
    f64, f32 = _forwards(data)
    orc = oracle.Forward(data.sta_x, data.sta_y, data.sta_z, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv, True, True)
    rng = np.random.default_rng(77)
    step = 0.05
    h = (data.ev_xyz + rng.normal(0, step, data.ev_xyz.shape)).reshape(-1)
    tc, ac, vs, qs = rng.normal(0, 0.01, S), rng.normal(0, 0.002, S), 3.0 + rng.normal(0, 0.005), 250.0 + rng.normal(0, 2.0)
    L0 = orc.calc_log_likelihood(h, tc, vs, ac, qs)
    n = 10000
    err, dL = np.empty(n), np.empty(n)
    for k in range(n):
        evt = int(rng.integers(1, E + 1))
        h2 = h.copy()
        h2[3 * (evt - 1) + int(rng.integers(0, 3))] += rng.normal(0, step)
        d64 = orc.partially_update_log_likelihood(evt, h, L0, h2, tc, vs, ac, qs) - L0
        d32 = f32.partially_update_log_likelihood(evt, h, L0, h2, tc, vs, ac, qs) - L0
        err[k], dL[k] = d32 - d64, d64
    logr = np.log(rng.uniform(size=n))
    flips = int(np.sum((logr <= dL) != (logr <= dL + err)))
    acc = float(np.mean(logr <= dL))
    _note(f"T5 {E}x{S} near the truth (step {step} km): judged differences median |dL| {np.median(np.abs(dL)):.3f}, rms {np.sqrt((dL ** 2).mean()):.3f}, "
          f"acceptance {acc:.3f}; error mean {err.mean():.3e} rms {np.sqrt((err ** 2).mean()):.3e} max {np.abs(err).max():.3e}; "
          f"decisions that differ {flips}/{n}")
    assert 0.05 < acc < 0.95 and np.median(np.abs(dL)) < 5.0, "not the regime this test is about"
    assert abs(err.mean()) <= 2e-3 and np.sqrt((err ** 2).mean()) <= 1e-2
    assert flips <= 0.002 * n


@pytest.mark.parametrize("E,S,nc,n_iter", [(100, 16, 8, 4_000_000), (1000, 64, 8, 600_000)])
def test_fp32_posterior_quantiles_within_monte_carlo_error(E, S, nc, n_iter, monkeypatch):
    """T6: medians and 2.5 % / 97.5 % points of every parameter (src/cls_statistics.f90:216-264) from the fp32-forward run against
    the Monte-Carlo error of the fp64 run -- two fp64 runs whose random streams start from other seeds
    (src/hypo_tremor_mcmc.f90:72)"""
    from hypotremormcmc_amd import driver, statistics, synth
    from hypotremormcmc_amd.obs_data import ObsData

    data = synth.make_synthetic(E, S, 3)
    obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)

    def run(prec, seeds):
        monkeypatch.setattr(driver, "SEEDS", seeds)
        params = dict(synth.DEFAULT_PARAMS, n_procs=1, n_chains=nc, n_cool=2, n_iter=n_iter, n_burn=n_iter // 3, n_interval=100,
                      forward_precision=prec)
        fwd, cs = driver.build_rank(params, data.sta_x, data.sta_y, data.sta_z, obs, 0, n_procs=1)
        cs.run(n_iter)
        sm = cs.samples()
        cols = np.concatenate([sm["vs"][:, None], sm["qs"][:, None], sm["t_corr"], sm["a_corr"], sm["hypo"]], axis=1)
        acc = cs.counts()
        del cs, fwd
        return statistics.quantiles(cols), len(cols), acc

    base, other = (5551111, 453222, 4444431, 6765), (7712345, 991234, 1357911, 424242)
    qa, na, _ = run("fp64", base)
    qb, nb, _ = run("fp64", other)
    q32, n32, _ = run("fp32", base)          # common random numbers with the first run: differs from it only through flipped decisions
    q32b, n32b, _ = run("fp32", other)       # ... and against the first run as an independent sampler
    assert na == nb == n32 == n32b and abs(na - 2 * (n_iter - n_iter // 3) // 100) <= 4
    width = np.maximum((qa[:, 2] - qa[:, 0]) / 3.92, 1e-12)[:, None]
    rms = lambda z: float(np.sqrt(np.mean(z ** 2)))
    zb, z32, z32b = (qb - qa) / width, (q32 - qa) / width, (q32b - qa) / width
    _note(f"T6 {E}x{S}x{nc}, {n_iter} iterations, {na} samples, {qa.shape[0]} parameters x 3 quantiles, in posterior widths: "
          f"fp64 (other seeds) - fp64: rms {rms(zb):.3f} max {np.abs(zb).max():.3f};  fp32 (same seeds) - fp64: rms {rms(z32):.3f} max "
          f"{np.abs(z32).max():.3f};  fp32 (other seeds) - fp64: rms {rms(z32b):.3f} max {np.abs(z32b).max():.3f}; "
          f"medians only: {rms(zb[:, 1]):.3f} / {rms(z32[:, 1]):.3f} / {rms(z32b[:, 1]):.3f}")
    assert rms(z32) <= 1.3 * rms(zb) + 0.05 and rms(z32b) <= 1.3 * rms(zb) + 0.05
    assert np.abs(z32).max() <= 1.5 * np.abs(zb).max() + 0.25


def test_fp32_chains_at_the_configs4_shape_agree_statistically():
    from hypotremormcmc_amd import driver, synth
    from hypotremormcmc_amd.obs_data import ObsData

    E, S, nc, n_iter = 10000, 128, 16, 400
    data = synth.make_synthetic(E, S, 5)
    obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
    res = {}
    for prec in ("fp64", "fp32"):
        params = dict(synth.DEFAULT_PARAMS, n_procs=1, n_chains=nc, n_cool=4, n_iter=n_iter, n_burn=100, n_interval=4,
                      forward_precision=prec)
        fwd, cs = driver.build_rank(params, data.sta_x, data.sta_y, data.sta_z, obs, 0, n_procs=1)
        assert fwd.forward_precision == prec
        cs.run(n_iter)
        it, ch, lk = cs.likelihood_trace()
        res[prec] = dict(counts=cs.counts(), it=it, lk=lk, first=np.array([lk[i] for i in range(len(it)) if it[i] == 1]))
        del cs, fwd
    # the first iteration evaluates every chain's initial model in full: same models, so T1 applies to each record
    a, b = res["fp64"]["first"], res["fp32"]["first"]
    assert len(a) == len(b) > 0
    rel0 = np.max(np.abs(a - b) / np.abs(a))
    (p64, a64), (p32, a32) = res["fp64"]["counts"], res["fp32"]["counts"]
    assert np.array_equal(p64, p32) or abs(int(p64.sum()) - int(p32.sum())) <= 0.02 * p64.sum()
    lines = []
    for k in range(7):
        n = max(int(p64[k]), 1)
        r64, r32 = a64[k] / n, a32[k] / max(int(p32[k]), 1)
        tol = 4.0 * np.sqrt(max(r64 * (1 - r64), 0.05) / n) * np.sqrt(2.0) + 0.02
        lines.append(f"type {k + 1}: proposed {int(p64[k])}/{int(p32[k])} accepted {int(a64[k])}/{int(a32[k])} (tolerance {tol:.3f})")
        assert abs(r64 - r32) <= tol, lines[-1]
    m64 = res["fp64"]["lk"][res["fp64"]["it"] > 200].mean(); m32 = res["fp32"]["lk"][res["fp32"]["it"] > 200].mean()
    _note(f"T4 {E}x{S}x{nc}: first-iteration records max rel {rel0:.3e}; mean cold log-likelihood after 200 it fp64 {m64:.6e} fp32 {m32:.6e} "
          f"(rel {abs(m64 - m32) / abs(m64):.3e}); " + "; ".join(lines))
    assert rel0 <= 3e-6
    assert abs(m64 - m32) <= 2e-3 * abs(m64)


# ---- BASELINE configs[4] as a multi-rank job: tempered chains over several ranks with the fp32 forward ----------------
def _t4_compare(tag, r64, r32, n_skip):
    """T4 between an fp64 and an fp32 run of the same job (common random numbers): same records at iteration 1 within
    T1, same temperature trajectory of the cold chains where T3 says so (a flipped decision in < 0.5 % of the steps),
    acceptance counts within 4 binomial sigma + 2 %, cold chains' log-likelihood within 2e-3 relative."""
    (p64, a64), (p32, a32) = r64["counts"], r32["counts"]
    assert np.array_equal(p64, p32) or abs(int(p64.sum()) - int(p32.sum())) <= 0.02 * p64.sum()
    lines = []
    for k in range(7):
        n = max(int(p64[k]), 1)
        q64, q32 = a64[k] / n, a32[k] / max(int(p32[k]), 1)
        tol = 4.0 * np.sqrt(max(q64 * (1 - q64), 0.05) / n) * np.sqrt(2.0) + 0.02
        lines.append(f"type {k + 1}: {int(p64[k])}/{int(p32[k])} proposed, {int(a64[k])}/{int(a32[k])} accepted")
        assert abs(q64 - q32) <= tol, lines[-1]
    same_rec, n_rec, rel0, m64, m32 = 0, 0, 0.0, [], []
    for (it64, ch64, lk64), (it32, ch32, lk32) in zip(r64["traces"], r32["traces"]):
        f64_, f32_ = lk64[it64 == 1], lk32[it32 == 1]
        assert len(f64_) == len(f32_)
        if len(f64_):
            rel0 = max(rel0, float(np.max(np.abs(f64_ - f32_) / np.abs(f64_))))
        # which chain is cold at which recorded iteration is decided by the swaps: equal lists = equal swap decisions
        k = min(len(it64), len(it32))
        same_rec += int(np.sum((it64[:k] == it32[:k]) & (ch64[:k] == ch32[:k]))); n_rec += max(len(it64), len(it32))
        m64.extend(lk64[it64 > n_skip]); m32.extend(lk32[it32 > n_skip])
    m64, m32 = float(np.mean(m64)), float(np.mean(m32))
    _note(f"T4 {tag}: first-iteration records max rel {rel0:.3e}; records on the same (iteration, chain) {same_rec}/{n_rec}; "
          f"mean cold log-likelihood fp64 {m64:.6e} fp32 {m32:.6e} (rel {abs(m64 - m32) / abs(m64):.3e}); " + "; ".join(lines))
    assert rel0 <= 3e-6
    assert same_rec >= 0.98 * n_rec
    assert abs(m64 - m32) <= 2e-3 * abs(m64)


def test_configs4_eight_ranks_of_sixteen_chains_fp32_forward(monkeypatch):
    """BASELINE configs[4]: 10 000 events x 128 stations, 128 tempered chains over 8 ranks, fp32 forward / fp64 accept
    (src/cls_forward.f90:268-303 under src/cls_parallel.f90:100-216).  Eight rank objects on the one GPU, records
    exchanged by device copies (LocalWorld): the lock-step kernels k_mcmc<2, true, 1> against the same job in fp64."""
    from hypotremormcmc_amd import driver, synth
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.parallel import LocalWorld

    monkeypatch.setenv("HTM_STREAM_CAP", str(1 << 17))      # eight ranks' stream rings on one device: the short ring
    E, S, nc, world, n_iter = 10000, 128, 16, 8, 120
    data = synth.make_synthetic(E, S, 5)
    obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
    res = {}
    for prec in ("fp64", "fp32"):
        params = dict(synth.DEFAULT_PARAMS, n_procs=world, n_chains=nc, n_cool=4, temp_high=200.0, n_iter=n_iter, n_burn=n_iter,
                      n_interval=2, forward_precision=prec)
        fwd, sets = None, []
        for r in range(world):
            fwd, cs = driver.build_rank(params, data.sta_x, data.sta_y, data.sta_z, obs, r, n_procs=world, fwd=fwd)
            sets.append(cs)
        assert fwd.forward_precision == prec
        LocalWorld(sets).run(n_iter)
        npr = np.zeros(7, np.int64); nac = np.zeros(7, np.int64)
        for cs in sets:
            a, b = cs.counts(); npr += a; nac += b
        res[prec] = dict(counts=(npr, nac), traces=[cs.likelihood_trace() for cs in sets])
        for cs in sets:
            cs.close()
        del sets, fwd
    _t4_compare(f"{E}x{S}, {world} ranks x {nc} chains (LocalWorld)", res["fp64"], res["fp32"], n_iter // 2)


def _fp32_direct_worker(rank, world, port, q):
    import sys

    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HTM_XCHG="1",
                      HTM_RANKS_PER_GPU=str(world), HTM_STREAM_CAP=str(1 << 17))
    import torch.distributed as dist

    from hypotremormcmc_amd import driver, synth
    from hypotremormcmc_amd.obs_data import ObsData
    from hypotremormcmc_amd.parallel import TorchWorld

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        E, S, nc, n_iter = 10000, 128, 16, 300
        data = synth.make_synthetic(E, S, 5)
        obs = ObsData.from_arrays(data.sta_x, data.sta_y, data.t_obs, data.t_stdv, data.a_obs, data.a_stdv)
        out = {}
        for prec in ("fp64", "fp32"):
            params = dict(synth.DEFAULT_PARAMS, n_procs=world, n_chains=nc, n_cool=4, temp_high=200.0, n_iter=n_iter,
                          n_burn=n_iter, n_interval=2, forward_precision=prec)
            fwd, cs = driver.build_rank(params, data.sta_x, data.sta_y, data.sta_z, obs, rank, n_procs=world, device=0)
            tw = TorchWorld(cs)
            assert tw.direct, "peer mapping of the inboxes failed"
            tw.run(n_iter // 3)
            tw.run(n_iter - n_iter // 3)
            assert tw.direct and tw.fell_back is None
            npr, nac = tw.reduce_counts()
            out[prec] = dict(counts=(npr, nac), trace=cs.likelihood_trace())
            cs.close()
            del tw, cs, fwd
            dist.barrier()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_configs4_two_processes_fp32_forward_through_the_in_kernel_exchange():
    """The same shape with the ranks in separate processes and the swap records exchanged INSIDE the persistent kernels
    (k_mcmc<2, true, 2>; inboxes mapped between the processes as a node maps them between GPUs): 2 ranks x 16 chains,
    fp32 against fp64, both through that transport."""
    import queue
    import socket
    import time

    import torch.multiprocessing as mp

    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fp32_direct_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, t_end = {}, time.time() + 500
    while len(res) < world and time.time() < t_end:
        try:
            r, out = q.get(timeout=2)
            res[r] = out
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
        assert p.exitcode == 0
    assert sorted(res) == list(range(world))
    r64 = dict(counts=res[0]["fp64"]["counts"], traces=[res[r]["fp64"]["trace"] for r in range(world)])
    r32 = dict(counts=res[0]["fp32"]["counts"], traces=[res[r]["fp32"]["trace"] for r in range(world)])
    _t4_compare("10000x128, 2 processes x 16 chains (in-kernel exchange)", r64, r32, 150)
