"""Short two-chain jobs in which select_pair (src/cls_parallel.f90:226-230) needs more redraws of i2 than k_stream_rec
precomputes (12: csrc/htm_chains_kernels.hpp), so that the chain loop under test has to follow the stream in its own
fallback.  Shared by tests/test_redraw_cases.py (CPU: the oracle's swap log holds every stated event) and
tests/test_gpu_redraw.py (the device).  Found by tools/find_redraw_cases.py, which runs only the oracle.

With n_procs * n_chains == 2 a redraw fails with probability 1/2: the event comes about once in 4096 iterations.  Where on
rank 0's stream a swap starts depends on everything that draws before it, so E, S, the synth seed, the step sizes and the
solve / use switches all move it.

They move it less than one would think.  A swap ends right behind the first draw on the other side of 0.5, wherever in a run of
equal draws it started, so jobs whose streams differ by a few positions fall into step again within a few iterations: only
rejections by the depth prior (a step then takes one draw less) and the solve switches send a job down another path for long.
Rank 0's stream has runs of 13 or more draws on one side of 0.5 at positions 1701, 4879, 17024, 19563, 38321, 46038, ...; the
search (about 40 000 jobs: E 3..200, four values of S, seeds 11..13, step_size_z 0.4..30, every single switch) found no job whose
swap starts at 1701, 4879 or 17024.  Single-rank jobs meet 19563 (a run of 14) at iterations 1150..1250; two ranks of one chain
start a swap at 19564, one position into the same run, at iterations 2059..2099 (i1 = 0), and at 46038 near iteration 4900
(i1 = 1: the only early event whose judge draw is rank 1's) -- hence the lengths below."""
import functools

from hypotremormcmc_amd import synth

MIN_PAIR_DRAWS = 14      # one draw for i1, thirteen or more for i2: more than 12 redraws

# name: (E, S, n_procs, n_chains, synth seed, parameter overrides, n_iter, event iteration); n_iter = event iteration + 100
CASES = {
    # 64 stations with both data types: the free-running master's specialised instantiation (15 pair draws, swap start 19563)
    "spec64": (64, 64, 1, 2, 12, {"step_size_z": 12.0}, 1283, 1183),
    # two stations per lane, a ragged row: the generic instantiations only
    "ragged70": (33, 70, 1, 2, 11, {"step_size_z": 6.0}, 1294, 1194),
    # two ranks of one chain; i1 = 0: rank 0 draws the pair and the judge number
    "ranks2_judge0": (20, 16, 2, 1, 11, {"step_size_z": 12.0}, 2191, 2091),
    # two ranks of one chain; i1 = 1: rank 0 draws the pair and nothing else, the judge number is rank 1's
    # (on its way the job passes an event of the other kind, i1 = 0, at iteration 2059)
    "ranks2_judge1": (20, 64, 2, 1, 12, {"step_size_z": 0.4}, 4999, 4899),
}
# the event's (pair draws, i1, rank of the judge draw) as the search printed them
EVENTS = {"spec64": (15, 0, 0), "ragged70": (15, 0, 0), "ranks2_judge0": (14, 0, 0), "ranks2_judge1": (14, 1, 1)}

# the golden fixture that holds the event by accident (1 rank x 2 chains, S = 16, 4000 iterations)
C2_EVENT_ITER = 3860


def params_of(n_procs, n_chains, n_iter, over):
    p = dict(synth.DEFAULT_PARAMS, n_procs=n_procs, n_chains=n_chains, n_cool=1, n_iter=n_iter, n_burn=n_iter // 2, n_interval=5)
    p.update(over)
    return p


def build(name):
    """(data, params, n_iter, event iteration) of a case"""
    E, S, n_procs, n_chains, seed, over, n_iter, k = CASES[name]
    return synth.make_synthetic(E, S, seed), params_of(n_procs, n_chains, n_iter, over), n_iter, k


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the oracle's job of a case after n_iter iterations, with its step log and swap log: computed once, read by every test"""
    from oracle import oracle

    data, params, n_iter, _ = build(name)
    p64 = {k: v for k, v in params.items() if k != "forward_precision"}
    job = oracle.Job(p64, data)
    job.enable_steplog(n_iter * 2)
    job.enable_swaplog(n_iter)
    job.run(n_iter)
    return job


def events(swaplog):
    """rows of a swap log at which the loops leave their precomputed pair"""
    return swaplog[swaplog[:, 3] >= MIN_PAIR_DRAWS]
