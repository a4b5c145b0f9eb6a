"""htm_forward_locate_draw_evidence (every window's log evidence under every one of K draws in ONE kernel)
against the only way to get the same numbers without it: K calls of htm_forward_locate, one per draw, reading loc[6] of each;
and, next to it, htm_forward_locate_marginal at the same K, which does the same arithmetic per (cell, station, draw).

    1000 windows x 64 stations, both data types, step 5's prior, 32 x 32 x 16 cells, K = 8, 64

All three are synchronous host calls and are timed alike, in the same process, as tools/bench_locate_marginal.py times them:
a host clock around the call (around all K calls of the yardstick); one warm-up call of each with 8 windows on the same grid
with the same K (code objects loaded, the device awake); then --reps timed calls with all windows (no marginals, no volume
come back): the median, with the fastest and the slowest.  The new call's log_z is compared with the K calls' log evidences at
the size that is timed.  Every K is a process of its own under its own `timeout`; the first that fails ends the run.  The lines
go to the screen and, appended, to --out.

    python tools/bench_locate_draws.py [--windows 1000] [--stations 64] [--reps 3] [--draws 8 64]
                                       [--lib NAME=PATH ...]     # A/B: the same with other builds of the library (HTM_LIB)
    python tools/bench_locate_draws.py --one K                   # one K in this process
    python tools/bench_locate_draws.py --once K                  # one call of the new entry point and nothing else, for a kernel trace
"""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, ".")

GRID_NAME = "32 x 32 x 16"
STEP_SECONDS = 300


def one(args, K):
    import numpy as np

    from hypotremormcmc_amd import locate as lc
    from hypotremormcmc_amd import synth
    from hypotremormcmc_amd.forward import Forward, ObsArrays

    grid = np.array([-64.0, 4.0, 32, -64.0, 4.0, 32, 0.5, 2.0, 16])
    E, S = args.windows, args.stations
    cells = int(grid[2] * grid[5] * grid[8])
    data = synth.make_synthetic(E, S, 3)
    prior = np.stack([np.zeros(E), np.zeros(E), np.full(E, 30.0), np.zeros(E), np.full(E, 10.0)], axis=1)
    rng = np.random.default_rng(11)                  # draws that scatter about the structure the data were made with
    vs, qs = 3.0 * (1.0 + 0.01 * rng.normal(size=K)), 250.0 * (1.0 + 0.05 * rng.normal(size=K))
    tc, ac = rng.normal(0.0, 0.02, (K, S)), rng.normal(0.0, 0.01, (K, S))

    def forward_of(n):
        return Forward(S, n, data.sta_x, data.sta_y, data.sta_z, ObsArrays(data.t_obs[:n], data.t_stdv[:n], data.a_obs[:n], data.a_stdv[:n]))

    def evidence(fwd, n):
        return lc.draw_evidence(fwd, tc, vs, ac, qs, grid, prior=prior[:n])["log_z"]

    def marginal(fwd, n):
        return lc.locate_marginal(fwd, tc, vs, ac, qs, grid, prior=prior[:n], marginals=False)["log_evidence"]

    def k_calls(fwd, n):
        return np.stack([lc.locate(fwd, tc[k], vs[k], ac[k], qs[k], grid, prior=prior[:n], marginals=False)["log_evidence"] for k in range(K)], axis=1)

    fwd = forward_of(E)
    if args.once is not None:
        evidence(fwd, E)
        fwd.close()
        return
    warm = forward_of(min(E, 8))
    for f in (evidence, marginal, k_calls):
        f(warm, min(E, 8))
    warm.close()
    names = ("htm_forward_locate_draw_evidence", "htm_forward_locate_marginal", f"{K} x htm_forward_locate")
    times, results = {}, {}
    for name, f in zip(names, (evidence, marginal, k_calls)):
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = f(fwd, E)
            ts.append(time.perf_counter() - t0)
        assert np.isfinite(res).all()
        times[name], results[name] = ts, res
        t = float(np.median(ts))
        print(f"{name:34s} K = {K:3d}, {E} windows x {S} stations, {GRID_NAME} cells: {t * 1e3:10.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}) "
              f"= {E * cells * K / t:.3e} (window, position, draw)/s", flush=True)
    fwd.close()
    new, marg, old = (times[n] for n in names)
    diff = np.max(np.abs(results[names[0]] - results[names[2]]) / np.abs(results[names[2]]))
    print(f"K = {K:3d}: {np.median(old) / np.median(new):.2f} x (medians); the new call's slowest {max(new) * 1e3:.2f} ms against the {K} calls' fastest "
          f"{min(old) * 1e3:.2f} ms: {min(old) / max(new):.2f} x; against htm_forward_locate_marginal {np.median(new) / np.median(marg):.2f} x its time; "
          f"largest relative difference of log_z from the {K} calls' log evidences {diff:.1e}", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--stations", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="also run with this build of the library")
    ap.add_argument("--out", default="profiles/locate_draws_bench.txt")
    ap.add_argument("--one", type=int, metavar="K")
    ap.add_argument("--once", type=int, metavar="K")
    args = ap.parse_args(argv)
    if args.one is not None or args.once is not None:
        one(args, args.one if args.one is not None else args.once)
        return 0
    builds = [("the library as built", None)] + [tuple(b.rsplit("=", 1)) for b in args.lib]
    with open(args.out, "a") as fh:
        for name, path in builds:
            head = f"# {name}" + (f" ({path})" if path else "")
            print(head, flush=True)
            fh.write(head + "\n")
            env = dict(os.environ)
            if path:
                env["HTM_LIB"] = os.path.abspath(path)
            for K in args.draws:
                cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--one", str(K), "--windows", str(args.windows),
                       "--stations", str(args.stations), "--reps", str(args.reps)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                sys.stdout.write(p.stdout)
                sys.stdout.flush()
                fh.write(p.stdout)
                fh.flush()
                if p.returncode != 0:
                    msg = f"# K = {K}: exit status {p.returncode}; nothing more is run\n"
                    sys.stdout.write(msg)
                    fh.write(msg)
                    return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
