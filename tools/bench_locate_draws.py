"""htm_forward_locate_draw_evidence (every window's log evidence under every one of K draws in ONE kernel)
against the only way to get the same numbers without it: K calls of htm_forward_locate, one per draw, reading loc[6] of each;
and, next to it, htm_forward_locate_marginal at the same K, which does the same arithmetic per (cell, station, draw).

    1000 windows x 64 stations, both data types, step 5's prior, 32 x 32 x 16 cells, K = 8, 64

All three are synchronous host calls and are timed alike, in the same process, as tools/bench_locate_marginal.py times them:
a host clock around the call (around all K calls of the yardstick); one warm-up call of each with 8 windows on the same grid
with the same K (code objects loaded, the device awake); then --reps timed calls with all windows (no marginals, no volume
come back): the median, with the fastest and the slowest.  The new call's log_z is compared with the K calls' log evidences at
the size that is timed.  Every K is a process of its own under its own `timeout`; the first that fails ends the run.  The lines
go to the screen and, appended, to --out (the job and the driver: tools/locate_bench_job.py).

    python tools/bench_locate_draws.py [--windows 1000] [--stations 64] [--reps 3] [--draws 8 64] [--use both|time|amp]
                                       [--precision fp64|fp32]   # the arithmetic of all three
                                       [--lib NAME=PATH ...]     # A/B: the same with other builds of the library (HTM_LIB)
    python tools/bench_locate_draws.py --one K                   # one K in this process
    python tools/bench_locate_draws.py --once K                  # one call of the new entry point and nothing else, for a kernel trace
"""
import sys

sys.path.insert(0, ".")
import locate_bench_job as bj


def one(args, K):
    import numpy as np

    from hypotremormcmc_amd import locate as lc

    job = bj.Job(args, K)
    grid, cells = job.grid()
    E, S = job.E, job.S

    def evidence(fwd, n):
        return lc.draw_evidence(fwd, job.tc, job.vs, job.ac, job.qs, grid, prior=job.prior[:n])["log_z"]

    def marginal(fwd, n):
        return lc.locate_marginal(fwd, job.tc, job.vs, job.ac, job.qs, grid, prior=job.prior[:n], marginals=False)["log_evidence"]

    def k_calls(fwd, n):
        return np.stack([lc.locate(fwd, job.tc[k], job.vs[k], job.ac[k], job.qs[k], grid, prior=job.prior[:n], marginals=False)["log_evidence"]
                         for k in range(K)], axis=1)

    fwd = job.forward_of(E)
    if args.once is not None:
        evidence(fwd, E)
        fwd.close()
        return
    warm = job.forward_of(min(E, 8))
    for f in (evidence, marginal, k_calls):
        f(warm, min(E, 8))
    warm.close()
    names = ("htm_forward_locate_draw_evidence", "htm_forward_locate_marginal", f"{K} x htm_forward_locate")
    times, results = {}, {}
    for name, f in zip(names, (evidence, marginal, k_calls)):
        ts, res = bj.timed(lambda: f(fwd, E), args.reps)
        assert np.isfinite(res).all()
        times[name], results[name] = ts, res
        t = float(np.median(ts))
        print(f"{name + job.tag:34s} K = {K:3d}, {E} windows x {S} stations, {bj.GRID_NAME} cells: {t * 1e3:10.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}) "
              f"= {E * cells * K / t:.3e} (window, position, draw)/s", flush=True)
    fwd.close()
    new, marg, old = (times[n] for n in names)
    diff = np.max(np.abs(results[names[0]] - results[names[2]]) / np.abs(results[names[2]]))
    print(f"K = {K:3d}: {np.median(old) / np.median(new):.2f} x (medians); the new call's slowest {max(new) * 1e3:.2f} ms against the {K} calls' fastest "
          f"{min(old) * 1e3:.2f} ms: {min(old) / max(new):.2f} x; against htm_forward_locate_marginal {np.median(new) / np.median(marg):.2f} x its time; "
          f"largest relative difference of log_z from the {K} calls' log evidences {diff:.1e}", flush=True)


if __name__ == "__main__":
    sys.exit(bj.main_over_draws(__file__, __doc__, one, [8, 64], "profiles/locate_draws_bench.txt"))
