#!/usr/bin/env python3
"""Search for short two-chain jobs whose swap pair needs more than 12 redraws (tests/redraw_cases.py).  CPU only: runs
the oracle with its swap log over a grid of shapes, synth seeds and parameter overrides and prints a table row for every
job that holds such an iteration within --max-iter.

    python tools/find_redraw_cases.py --procs 1 --S 64 --E 3:40 --seeds 11:14 --max-iter 400
    python tools/find_redraw_cases.py --procs 2 --S 16,64,70 --E 5:60 --max-iter 1300 --judge-rank 1

Each of E, S, the seed, step_size_z, use_amp and the solve switches shifts where on rank 0's stream the swaps start; a
job is a hit when one of them starts exactly where the stream then gives 13 or more draws on one side of 0.5."""
import argparse
import itertools
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from hypotremormcmc_amd import synth  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import redraw_cases as rc  # noqa: E402

OVERRIDES = [
    {}, {"use_amp": "F"}, {"use_time": "F"}, {"solve_qs": "F"}, {"solve_vs": "F"}, {"solve_t_corr": "F"}, {"solve_a_corr": "F"},
    {"solve_t_corr": "F", "solve_a_corr": "F"},
]


def ints(text):
    out = []
    for part in text.split(","):
        if ":" in part:
            a, b = part.split(":")
            out += list(range(int(a), int(b) + 1))
        else:
            out.append(int(part))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--procs", type=int, default=1, choices=(1, 2), help="n_procs; n_chains = 2 / n_procs")
    ap.add_argument("--E", default="5:40")
    ap.add_argument("--S", default="64")
    ap.add_argument("--seeds", default="11:13")
    ap.add_argument("--sz", default="0.4,6.0,12.0", help="step_size_z values")
    ap.add_argument("--max-iter", type=int, default=400)
    ap.add_argument("--judge-rank", type=int, default=-1, help="keep only events whose judge draw is this rank's")
    ap.add_argument("--all-overrides", action="store_true", help="also vary use_amp / use_time / the solve switches")
    a = ap.parse_args()
    n_chains = 2 // a.procs
    overs = OVERRIDES if a.all_overrides else OVERRIDES[:1]
    hits = []
    for E, S, seed in itertools.product(ints(a.E), ints(a.S), ints(a.seeds)):
        data = synth.make_synthetic(E, S, seed)
        for sz, over in itertools.product([float(v) for v in a.sz.split(",")], overs):
            over = dict(over, step_size_z=sz)
            job = oracle.Job(rc.params_of(a.procs, n_chains, a.max_iter, over), data)
            job.enable_swaplog(a.max_iter)
            job.run(a.max_iter)
            for it, i1, i2, nd, jr in rc.events(job.swaplog()):
                if a.judge_rank < 0 or jr == a.judge_rank:
                    hits.append((int(it), E, S, seed, over, int(nd), int(jr), int(i1)))
    for it, E, S, seed, over, nd, jr, i1 in sorted(hits, key=lambda h: h[0]):
        print("(%d, %d, %d, %d, %d, %r, %d, %d),   # %d pair draws, i1 = %d, judge draw on rank %d"
              % (E, S, a.procs, n_chains, seed, over, it + 100, it, nd, i1, jr))
    print("%d hits" % len(hits), file=sys.stderr)


if __name__ == "__main__":
    main()
