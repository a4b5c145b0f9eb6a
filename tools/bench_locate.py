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

    python tools/bench_locate.py [--windows 1000] [--stations 64] [--big-windows 1000] [--reps 3]
    python tools/bench_locate.py --once        # one call on the large grid and nothing else, for a kernel trace
"""
import argparse
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from hypotremormcmc_amd import locate as lc
from hypotremormcmc_amd import synth
from hypotremormcmc_amd.forward import Forward, ObsArrays

GRIDS = {"128 x 128 x 64": np.array([-64.0, 1.0, 128, -64.0, 1.0, 128, 0.5, 0.5, 64]),
         "32 x 32 x 16": np.array([-64.0, 4.0, 32, -64.0, 4.0, 32, 0.5, 2.0, 16])}


def forward_of(data, n):
    obs = ObsArrays(data.t_obs[:n], data.t_stdv[:n], data.a_obs[:n], data.a_stdv[:n])
    return Forward(data.n_sta, n, data.sta_x, data.sta_y, data.sta_z, obs)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--stations", type=int, default=64)
    ap.add_argument("--big-windows", type=int, default=1000, help="windows located on the large grid")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args(argv)
    E, S = args.windows, args.stations
    data = synth.make_synthetic(E, S, 3)
    zero = np.zeros(S)
    prior = np.stack([np.zeros(E), np.zeros(E), np.full(E, 30.0), np.zeros(E), np.full(E, 10.0)], axis=1)

    def locate_rate(name, n):
        fwd = forward_of(data, n)
        grid = GRIDS[name]
        cells = int(grid[2] * grid[5] * grid[8])
        if not args.once:
            warm = forward_of(data, min(n, 8))
            lc.locate(warm, zero, 3.0, zero, 250.0, grid, prior=prior[:min(n, 8)], marginals=False)
            warm.close()
        times = []
        for rep in range(1 if args.once else args.reps):
            t0 = time.perf_counter()
            res = lc.locate(fwd, zero, 3.0, zero, 250.0, grid, prior=prior[:n], marginals=False)
            times.append(time.perf_counter() - t0)
        fwd.close()
        assert (res["index"] >= 0).all()
        t = float(np.median(times))
        print(f"htm_forward_locate   {n:5d} windows x {S} stations, {name} cells: {t * 1e3:10.2f} ms per call "
              f"(min {min(times) * 1e3:.2f}, max {max(times) * 1e3:.2f}) = {n * cells / t:.3e} (window, position)/s "
              f"= {n * cells * S / t:.3e} station terms/s", flush=True)
        return n * cells / t

    if args.once:
        locate_rate("128 x 128 x 64", min(args.big_windows, E))
        return
    rates = {"32 x 32 x 16": locate_rate("32 x 32 x 16", E)}
    rates["128 x 128 x 64"] = locate_rate("128 x 128 x 64", min(args.big_windows, E))

    # the yardstick: 64 models per call, model m = every window at cell centre m of a slice of the grid
    fwd = forward_of(data, E)
    dev = torch.device("cuda")
    for name, grid in GRIDS.items():
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


if __name__ == "__main__":
    main()
