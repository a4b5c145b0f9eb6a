"""What tools/bench_locate.py, bench_locate_marginal.py and bench_locate_draws.py share: the job they time (the grid, synth's
data, step 5's prior, draws that scatter about the structure the data were made with, the Forward of the first n windows), the
timing of a synchronous host call (a host clock around it, --reps calls after the tool's warm-up) and the driver that runs
every step of a tool (a K, or bench_locate's whole measurement) as a process of its own under its own `timeout`, once per
build of the library: the library as built, then every --lib NAME=PATH through HTM_LIB.  The first step that fails ends the
run.  The lines go to the screen and, appended, to --out.
"""
import os
import subprocess
import sys
import time

GRID_NAME = "32 x 32 x 16"
GRIDS = {"128 x 128 x 64": [-64.0, 1.0, 128, -64.0, 1.0, 128, 0.5, 0.5, 64],
         GRID_NAME: [-64.0, 4.0, 32, -64.0, 4.0, 32, 0.5, 2.0, 16]}
STEP_SECONDS = 300
USE = {"both": (True, True), "time": (True, False), "amp": (False, True)}      # --use: use_time, use_amp of the Forward


class Job:
    """E windows x S stations of synth's data with step 5's prior, and (with K) K draws of the structure"""

    def __init__(self, args, K=None):
        import numpy as np

        from hypotremormcmc_amd import synth

        self.use = USE[args.use]
        self.precision = args.precision              # of the three locate entry points (Forward.set_locate_precision)
        self.tag = "" if args.precision == "fp64" else f" [{args.precision}]"
        E, S = self.E, self.S = args.windows, args.stations
        self.data = synth.make_synthetic(E, S, 3)
        self.prior = np.stack([np.zeros(E), np.zeros(E), np.full(E, 30.0), np.zeros(E), np.full(E, 10.0)], axis=1)
        if K is not None:
            rng = np.random.default_rng(11)                  # draws that scatter about the structure the data were made with
            self.vs, self.qs = 3.0 * (1.0 + 0.01 * rng.normal(size=K)), 250.0 * (1.0 + 0.05 * rng.normal(size=K))
            self.tc, self.ac = rng.normal(0.0, 0.02, (K, S)), rng.normal(0.0, 0.01, (K, S))

    @staticmethod
    def grid(name=GRID_NAME):
        """(grid9, cells) of the grid of that name"""
        import numpy as np

        g = np.array(GRIDS[name])
        return g, int(g[2] * g[5] * g[8])

    def forward_of(self, n):
        from hypotremormcmc_amd.forward import Forward, ObsArrays

        d = self.data
        fwd = Forward(self.S, n, d.sta_x, d.sta_y, d.sta_z, ObsArrays(d.t_obs[:n], d.t_stdv[:n], d.a_obs[:n], d.a_stdv[:n]),
                      use_time=self.use[0], use_amp=self.use[1])
        fwd.set_locate_precision(self.precision)
        return fwd


def timed(f, reps):
    """(the seconds of `reps` calls of f(), a host clock around each; the last call's result)"""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = f()
        ts.append(time.perf_counter() - t0)
    return ts, res


def add_arguments(ap, draws=None):
    """the options the three tools share (--draws: the two over draws)"""
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--stations", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    if draws:
        ap.add_argument("--draws", type=int, nargs="+", default=draws)
    ap.add_argument("--use", choices=list(USE), default="both", help="the data types the Forward uses (the kernels' MODE)")
    ap.add_argument("--precision", choices=("fp64", "fp32"), default="fp64", help="the arithmetic of the locate entry points (DESIGN.md 3.13); "
                    "fp32 is named in every line")
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH", help="also run with this build of the library")


def drive(script, args, steps, out=None):
    """Every build, every step = (its name in a failure's line, the step's own arguments) as `python script <step's arguments>
    <the shared options>` under `timeout`; returns the exit status of the first step that fails, or 0."""
    builds = [("the library as built", None)] + [tuple(b.rsplit("=", 1)) for b in args.lib]
    shared = ["--windows", str(args.windows), "--stations", str(args.stations), "--reps", str(args.reps)]
    if args.use != "both":
        shared += ["--use", args.use]
    if args.precision != "fp64":
        shared += ["--precision", args.precision]
    fh = open(out, "a") if out else None

    def say(text):
        sys.stdout.write(text)
        sys.stdout.flush()
        if fh:
            fh.write(text)
            fh.flush()

    try:
        for name, path in builds:
            say(f"# {name}" + (f" ({path})" if path else "") + (f", --use {args.use}" if args.use != "both" else "")
                + (f", --precision {args.precision}" if args.precision != "fp64" else "") + "\n")
            env = dict(os.environ)
            if path:
                env["HTM_LIB"] = os.path.abspath(path)
            for label, argv in steps:
                cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(script)] + argv + shared
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                say(p.stdout)
                if p.returncode != 0:
                    say(f"# {label}: exit status {p.returncode}; nothing more is run\n")
                    return p.returncode
        return 0
    finally:
        if fh:
            fh.close()


def main_over_draws(script, doc, one, draws, out):
    """the command line of the two tools over draws: every K of --draws through `drive`, or --one K / --once K in this process"""
    import argparse

    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0])
    add_arguments(ap, draws)
    ap.add_argument("--out", default=out)
    ap.add_argument("--one", type=int, metavar="K")
    ap.add_argument("--once", type=int, metavar="K")
    args = ap.parse_args()
    if args.one is not None or args.once is not None:
        one(args, args.one if args.one is not None else args.once)
        return 0
    return drive(script, args, [(f"K = {K}", ["--one", str(K)]) for K in args.draws], args.out)
