"""Coarse to fine against one fine grid: the resolution of 1 km cells for every window

    (a) on one grid of 128 x 128 x 64 cells of 1 km (htm_forward_locate, or htm_forward_locate_marginal over K draws), and
    (b) on 32 x 32 x 16 cells of 4 km, then on a box of its own per window about the best coarse cell, --factor 4 at --radius 2:
        20 x 20 x 20 cells of 1 km (locate.refine: the coarse call, locate.refine_boxes, htm_forward_locate_boxes)

    1000 windows x 64 stations, both data types, step 5's prior; K = 0 (a fixed structure) and K = 64 draws

The two lattices coincide, so the share of windows whose refined best cell IS the one-grid best cell is counted, next to the
flags of the refinement.  All calls are synchronous host calls and are timed alike, in the same process, as
tools/bench_locate.py times them: a host clock around the call; one warm-up call of each with 8 windows (code objects loaded,
the device awake); then --reps timed calls with all windows: the median, with the fastest and the slowest.  The fine pass is
timed alone too (htm_forward_locate_boxes on the boxes that the coarse pass gave), with its (window, position)/s next to the
one grid's: its tiles are whole x-rows of one z-layer, 400 cells of a box in a workgroup built for 4096, and that is what the
difference of the two rates measures.  Every K is a process of its own under its own `timeout`; the first that fails ends the
run.  The lines go to the screen and, appended, to --out (the job and the driver: tools/locate_bench_job.py).

    python tools/bench_locate_refine.py [--windows 1000] [--stations 64] [--reps 3] [--draws 0 64] [--use both|time|amp]
                                        [--precision fp64|fp32] [--lib NAME=PATH ...]
    python tools/bench_locate_refine.py --one K                  # one K in this process (0: a fixed structure)
    python tools/bench_locate_refine.py --once K                 # one fine pass and nothing else, for a kernel trace
"""
import sys

sys.path.insert(0, ".")
import locate_bench_job as bj

FACTOR, RADIUS = 4, 2
FINE_NAME = "128 x 128 x 64"


def one(args, K):
    import numpy as np

    from hypotremormcmc_amd import locate as lc

    job = bj.Job(args, K if K else None)
    E, S = job.E, job.S
    coarse_grid, _ = job.grid()
    fine_grid, fine_cells = job.grid(FINE_NAME)
    structure = (job.tc, job.vs, job.ac, job.qs) if K else (np.zeros(S), 3.0, np.zeros(S), 250.0)
    single = lc.locate_marginal if K else lc.locate
    how = f"K = {K:3d}" if K else "fixed structure"

    def one_grid(fwd, n):
        return single(fwd, *structure, fine_grid, prior=job.prior[:n], marginals=False)

    def coarse(fwd, n):
        return single(fwd, *structure, coarse_grid, prior=job.prior[:n])

    def fine(fwd, n, first):
        bx = lc.refine_boxes(first["index"][:n], coarse_grid, FACTOR, RADIUS)
        return lc.locate_boxes(fwd, *structure, bx["fine_grid"], bx["origins"], prior=job.prior[:n])

    def both(fwd, n):
        return lc.refine(fwd, *structure, coarse_grid, FACTOR, radius=RADIUS, prior=job.prior[:n])

    fwd = job.forward_of(E)
    if args.once is not None:
        fine(fwd, E, coarse(fwd, E))
        fwd.close()
        return
    m = min(E, 8)
    warm = job.forward_of(m)
    one_grid(warm, m)
    both(warm, m)
    warm.close()

    def report(name, ts, positions):
        t = float(np.median(ts))
        print(f"{name + job.tag:44s} {how}, {E} windows x {S} stations: {t * 1e3:10.2f} ms (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f})"
              + (f" = {E * positions / t:.3e} (window, position)/s" if positions else ""), flush=True)
        return t

    ts, whole = bj.timed(lambda: one_grid(fwd, E), args.reps)
    t_whole = report(f"(a) one grid of {FINE_NAME} cells", ts, fine_cells)
    ts, first = bj.timed(lambda: coarse(fwd, E), args.reps)
    t_coarse = report(f"(b) the coarse pass, {bj.GRID_NAME} cells", ts, int(np.prod(lc.grid_counts(coarse_grid))))
    ts, boxes = bj.timed(lambda: fine(fwd, E, first), args.reps)
    box_cells = int(np.prod(boxes["marg_x"].shape[1:] + boxes["marg_y"].shape[1:] + boxes["marg_z"].shape[1:]))
    t_fine = report(f"(b) the fine pass alone, {box_cells} cells per window", ts, box_cells)
    ts, res = bj.timed(lambda: both(fwd, E), args.reps)
    t_both = report("(b) coarse, boxes and fine: locate.refine", ts, 0)
    fwd.close()
    # the refined best cell on the one grid's lattice
    nf = lc.grid_counts(res["fine_grid"])
    f = np.stack([res["index"] % nf[0], (res["index"] // nf[0]) % nf[1], res["index"] // (nf[0] * nf[1])], axis=1) + res["i0"] * FACTOR
    n1 = lc.grid_counts(fine_grid)
    same = (res["index"] >= 0) & (f[:, 0] + n1[0] * (f[:, 1] + n1[1] * f[:, 2]) == whole["index"])
    print(f"{how}: one grid {t_whole / t_both:.1f} x the time of the refinement; the fine pass evaluates {E * box_cells / t_fine / (E * fine_cells / t_whole):.2f} x the one grid's "
          f"(window, position)/s and is {t_fine / t_both:.0%} of the refinement ({t_coarse / t_both:.0%} the coarse pass); the refined best cell is the one grid's in "
          f"{int(same.sum())} of {E} windows; {int(res['inner_face'].sum())} on an inner face, {int(res['outer_face'].sum())} on an outer face, "
          f"{int((res['mass_bound'] < lc.MASS_BOUND_LOW).sum())} with a mass bound below {lc.MASS_BOUND_LOW}", flush=True)


if __name__ == "__main__":
    sys.exit(bj.main_over_draws(__file__, __doc__, one, [0, 64], "profiles/locate_refine_bench.txt"))
