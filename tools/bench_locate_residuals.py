"""What the residual pass costs: htm_forward_locate_residuals (the stations' residuals, the source terms and the fit of every
window) against htm_forward_locate on the same job, same build, same process, one after the other.

    1000 windows x 64 stations   32 x 32 x 16 cells (4 km cells)
                                 128 x 128 x 64 cells (1 km cells; --big-windows of the windows, default all)

Both are synchronous host calls: a host clock around each; one warm-up call of each on the same grid with 8 windows (the same
kernels: code objects loaded, the device awake), then the median of --reps calls with all windows, the two calls alternating
(summaries only from the plain call: no marginals, no volume; the residual call brings loc, the marginals, res and fit back and
keeps a batch's volume on the device).  The pass's share of a residual call is taken from a kernel trace of `--once`, a run
of its own.

    python tools/bench_locate_residuals.py [--windows 1000] [--stations 64] [--big-windows 1000] [--reps 3] [--use both|time|amp]
                                           [--precision fp64|fp32] [--lib NAME=PATH ...] [--out FILE]
    python tools/bench_locate_residuals.py --one         # the measurement in this process
    python tools/bench_locate_residuals.py --once        # one residual call on the large grid and nothing else, for a kernel trace

The measurement is a process of its own under `timeout`, once per build (the job and the driver: tools/locate_bench_job.py).
"""
import argparse
import sys

sys.path.insert(0, ".")
import locate_bench_job as bj


def measure(args):
    import numpy as np

    from hypotremormcmc_amd import locate as lc

    job = bj.Job(args)
    E, S, prior = job.E, job.S, job.prior
    zero = np.zeros(S)
    plain = lambda fwd, n, grid: lc.locate(fwd, zero, 3.0, zero, 250.0, grid, prior=prior[:n], marginals=False)
    resid = lambda fwd, n, grid: lc.residuals(fwd, zero, 3.0, zero, 250.0, grid, prior=prior[:n])

    def both(name, n):
        grid, cells = job.grid(name)
        fwd = job.forward_of(n)
        if args.once:
            times, res = bj.timed(lambda: resid(fwd, n, grid), 1)
            fwd.close()
            print(f"htm_forward_locate_residuals{job.tag} {n:5d} windows x {S} stations, {name} cells: {times[0] * 1e3:10.2f} ms, one call", flush=True)
            return
        warm = job.forward_of(min(n, 8))
        plain(warm, min(n, 8), grid)
        resid(warm, min(n, 8), grid)
        warm.close()
        tp, tr = [], []
        for _ in range(args.reps):          # alternating: a drift of the machine reaches both
            t, a = bj.timed(lambda: plain(fwd, n, grid), 1)
            tp += t
            t, b = bj.timed(lambda: resid(fwd, n, grid), 1)
            tr += t
        fwd.close()
        assert (a["index"] >= 0).all() and np.array_equal(a["loc"], b["loc"]) and np.isfinite(b["res"][:, :, [k for k in range(4) if job.use[k // 2]]]).all()
        p, r = float(np.median(tp)), float(np.median(tr))
        for what, t, ts in (("htm_forward_locate          ", p, tp), ("htm_forward_locate_residuals", r, tr)):
            print(f"{what}{job.tag} {n:5d} windows x {S} stations, {name} cells: {t * 1e3:10.2f} ms per call (min {min(ts) * 1e3:.2f}, "
                  f"max {max(ts) * 1e3:.2f}) = {n * cells * S / t:.3e} station terms/s", flush=True)
        print(f"residuals / plain{job.tag}, {name} cells: {r / p:.2f}", flush=True)

    if args.once:
        both("128 x 128 x 64", min(args.big_windows, E))
        return
    both("32 x 32 x 16", E)
    both("128 x 128 x 64", min(args.big_windows, E))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    bj.add_arguments(ap)
    ap.add_argument("--big-windows", type=int, default=1000, help="windows located on the large grid")
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args(argv)
    if args.one or args.once:
        measure(args)
        return 0
    return bj.drive(__file__, args, [("the measurement", ["--one", "--big-windows", str(args.big_windows)])], args.out)


if __name__ == "__main__":
    sys.exit(main())
