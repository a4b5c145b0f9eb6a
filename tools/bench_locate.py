"""(window, position) evaluations per second of htm_forward_locate (the location posteriors on a grid under a fixed
structure) against the only way to do the same job without it: Forward.calc_log_likelihood_batch_dev over
the same positions, 64 models per call, every model holding all windows at one cell centre -- each call re-reads every
window's observations for every position and reduces across lanes per model.

    1000 windows x 64 stations   32 x 32 x 16 cells (4 km cells)
                                 128 x 128 x 64 cells (1 km cells; --big-windows of the windows, default all)

htm_forward_locate is a synchronous host call: a host clock around it; one warm-up call on the same grid with 8 windows (the
same kernels: code objects loaded, the device awake), then the median of --reps calls with all windows (summaries only: no
marginals, no volume come back).  The kernels' share of a call is taken from a kernel trace of `--once`, a run of its own.
The yardstick is timed with HIP events on the handle's stream (htm_forward_time_full_batch_dev: a warm-up call, then the
mean of 20 calls) on a slice of the grid -- 64 positions are one call, and every call costs the same.

    python tools/bench_locate.py [--windows 1000] [--stations 64] [--big-windows 1000] [--reps 3] [--use both|time|amp]
                                 [--precision fp64|fp32]   # the arithmetic of htm_forward_locate (the yardstick stays fp64)
                                 [--lib NAME=PATH ...]     # A/B: the same with other builds of the library (HTM_LIB)
    python tools/bench_locate.py --one         # the measurement in this process
    python tools/bench_locate.py --once        # one call on the large grid and nothing else, for a kernel trace

The measurement is a process of its own under `timeout`, once per build (the job and the driver: tools/locate_bench_job.py).
"""
import argparse
import sys

sys.path.insert(0, ".")
import locate_bench_job as bj


def measure(args):
    import numpy as np
    import torch

    from hypotremormcmc_amd import locate as lc

    job = bj.Job(args)
    E, S, prior = job.E, job.S, job.prior
    zero = np.zeros(S)

    def locate_rate(name, n):
        fwd = job.forward_of(n)
        grid, cells = job.grid(name)
        if not args.once:
            warm = job.forward_of(min(n, 8))
            lc.locate(warm, zero, 3.0, zero, 250.0, grid, prior=prior[:min(n, 8)], marginals=False)
            warm.close()
        times, res = bj.timed(lambda: lc.locate(fwd, zero, 3.0, zero, 250.0, grid, prior=prior[:n], marginals=False), 1 if args.once else args.reps)
        fwd.close()
        assert (res["index"] >= 0).all()
        t = float(np.median(times))
        print(f"htm_forward_locate{job.tag}   {n:5d} windows x {S} stations, {name} cells: {t * 1e3:10.2f} ms per call "
              f"(min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}) = {n * cells / t:.3e} (window, position)/s "
              f"= {n * cells * S / t:.3e} station terms/s", flush=True)
        return n * cells / t

    if args.once:
        locate_rate("128 x 128 x 64", min(args.big_windows, E))
        return
    rates = {"32 x 32 x 16": locate_rate("32 x 32 x 16", E)}
    rates["128 x 128 x 64"] = locate_rate("128 x 128 x 64", min(args.big_windows, E))

    # the yardstick: 64 models per call, model m = every window at cell centre m of a slice of the grid
    fwd = job.forward_of(E)
    dev = torch.device("cuda")
    for name in bj.GRIDS:
        grid, _ = job.grid(name)
        x = grid[0] + (np.arange(64) + 0.5) * grid[1]                       # the first 64 cells of the row (iy, iz) = (ny / 2, nz / 2)
        pos = np.stack([x, np.full(64, grid[3] + (grid[5] // 2 + 0.5) * grid[4]), np.full(64, grid[6] + (grid[8] // 2 + 0.5) * grid[7])], axis=1)
        pos = pos[np.arange(64) % int(grid[2])]
        hypo = torch.tensor(np.tile(pos[:, None, :], (1, E, 1)).reshape(64, 3 * E), dtype=torch.float64, device=dev)
        corr = torch.zeros(64, S, dtype=torch.float64, device=dev)
        vs = torch.full((64,), 3.0, dtype=torch.float64, device=dev)
        qs = torch.full((64,), 250.0, dtype=torch.float64, device=dev)
        out = torch.empty(64, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        us = fwd.time_full_batch_dev(64, hypo.data_ptr(), corr.data_ptr(), vs.data_ptr(), corr.data_ptr(), qs.data_ptr(), out.data_ptr(), 20)
        rate = E * 64 / (us * 1e-6)
        print(f"loglik_full_batch_dev {E:5d} windows x {S} stations, 64 positions of {name} per call: {us:10.2f} us per call "
              f"= {rate:.3e} (window, position)/s; htm_forward_locate is {rates[name] / rate:.1f} x that", flush=True)
    fwd.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    bj.add_arguments(ap)
    ap.add_argument("--big-windows", type=int, default=1000, help="windows located on the large grid")
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args(argv)
    if args.one or args.once:
        measure(args)
        return 0
    return bj.drive(__file__, args, [("the measurement", ["--one", "--big-windows", str(args.big_windows)])])


if __name__ == "__main__":
    sys.exit(main())
