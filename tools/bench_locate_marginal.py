"""htm_forward_locate_marginal (the structure marginalised over K draws in ONE kernel) against the only way to
do the job without it: K calls of htm_forward_locate, one per draw (which still leaves K volumes to combine on the host --
that part is not even counted here).

    1000 windows x 64 stations, both data types, step 5's prior, 32 x 32 x 16 cells, K = 1, 8, 64

Both are synchronous host calls and are timed alike, in the same process, as tools/bench_locate.py times the old call: a host
clock around the call (around all K calls of the yardstick); one warm-up call with 8 windows on the same grid with the same K
(code objects loaded, the device awake); then --reps timed calls with all windows (summaries only: no marginals, no volume
come back): the median, with the fastest and the slowest.  Every K is a process of its own under its own `timeout`; the first
that fails ends the run.  The lines go to the screen and, appended, to --out (the job and the driver: tools/locate_bench_job.py).

    python tools/bench_locate_marginal.py [--windows 1000] [--stations 64] [--reps 3] [--draws 1 8 64] [--use both|time|amp]
                                          [--precision fp64|fp32]   # the arithmetic of both sides
                                          [--lib NAME=PATH ...]     # A/B: the same with other builds of the library (HTM_LIB)
    python tools/bench_locate_marginal.py --one K                   # one K in this process
    python tools/bench_locate_marginal.py --once K                  # one marginal call and nothing else, for a kernel trace
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

    def marginal(fwd, n):
        return lc.locate_marginal(fwd, job.tc, job.vs, job.ac, job.qs, grid, prior=job.prior[:n], marginals=False)

    def k_calls(fwd, n):
        for k in range(K):
            res = lc.locate(fwd, job.tc[k], job.vs[k], job.ac[k], job.qs[k], grid, prior=job.prior[:n], marginals=False)
        return res

    fwd = job.forward_of(E)
    if args.once is not None:
        marginal(fwd, E)
        fwd.close()
        return
    warm = job.forward_of(min(E, 8))
    marginal(warm, min(E, 8))
    k_calls(warm, min(E, 8))
    warm.close()
    times = {}
    for name, f in (("htm_forward_locate_marginal", marginal), (f"{K} x htm_forward_locate", k_calls)):
        ts, res = bj.timed(lambda: f(fwd, E), args.reps)
        assert (res["index"] >= 0).all()
        times[name] = ts
        t = float(np.median(ts))
        print(f"{name + job.tag:30s} K = {K:3d}, {E} windows x {S} stations, {bj.GRID_NAME} cells: {t * 1e3:10.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}) "
              f"= {E * cells * K / t:.3e} (window, position, draw)/s", flush=True)
    fwd.close()
    new, old = times["htm_forward_locate_marginal"], times[f"{K} x htm_forward_locate"]
    print(f"K = {K:3d}: {np.median(old) / np.median(new):.2f} x (medians); the marginal call's slowest {max(new) * 1e3:.2f} ms against the {K} calls' fastest "
          f"{min(old) * 1e3:.2f} ms: {min(old) / max(new):.2f} x", flush=True)


if __name__ == "__main__":
    sys.exit(bj.main_over_draws(__file__, __doc__, one, [1, 8, 64], "profiles/locate_marginal_bench.txt"))
