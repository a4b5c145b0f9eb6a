"""CPU side of the redraw-fallback tests: the oracle's swap log (oracle/htm_oracle.c log_swap) changes nothing it observes,
agrees with an independent count of rank 0's draws, and holds the event every row of tests/redraw_cases.py states -- so that a
change to the generator or to a fixture that moves the event away is a red test here, not a GPU test that checks nothing."""
import numpy as np
import pytest

from tests import redraw_cases as rc
from tests.helpers import load_case

GOFF = {1: 1, 2: 2, 3: 1, 4: 2, 5: 3, 6: 3, 7: 3}      # draws of a step before its perturbation: a_select (+ index, + component)


def _stream_positions(n):
    """rank 0's generator state after 0 .. n serial draws -> the number of draws"""
    from oracle import oracle

    r = oracle.Rng(0)
    pos = {r.state: 0}
    for k in range(1, n + 1):
        r.rand_u()
        pos[r.state] = k
    return pos


def _final(job):
    out = [job.counts()]
    for r in range(int(job.p.n_procs)):
        out += [job.rng_state(r), job.likelihood_trace(r), job.samples(r)]
        out += [job.chain(r, c) for c in range(int(job.p.n_chains))]
    return out


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("name", ["spec64", "ranks2_judge1"])
def test_swap_log_changes_no_draw(name):
    """one job with the log on and one with it off: the same generator states, traces, samples, counters and chain states"""
    from oracle import oracle

    data, params, n_iter, _ = rc.build(name)
    on = oracle.Job(params, data); on.enable_swaplog(n_iter); on.run(n_iter)
    off = oracle.Job(params, data); off.run(n_iter)
    assert len(on.swaplog()) == n_iter and len(off.swaplog()) == 0
    assert _same(_final(on), _final(off))
    # a full log keeps its rows and the run goes on unchanged
    small = oracle.Job(params, data); small.enable_swaplog(7); small.run(n_iter)
    assert np.array_equal(small.swaplog(), on.swaplog()[:7]) and _same(_final(small), _final(off))


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_swap_log_accounts_for_every_draw_of_rank_0(name):
    """Per iteration, rank 0's stream advances by the draws of its chains' steps (step log: goff + 3 with the prior satisfied, the
    judge's number included, else goff + 2) + the logged pair draws + the swap's judge draw where it is rank 0's; the position
    is read off a serially drawn stream, not computed."""
    from oracle import oracle

    data, params, n_iter, k = rc.build(name)
    job = oracle.Job(params, data)
    job.enable_steplog(2 * n_iter); job.enable_swaplog(n_iter)
    pos = _stream_positions(16 * n_iter + 6 * data.n_events + 8 * data.n_sta + 64)
    at = [pos[job.rng_state(0)]]
    for _ in range(n_iter):
        job.run(1)
        at.append(pos[job.rng_state(0)])
    si, _ = job.steplog()
    sw = job.swaplog()
    assert np.array_equal(sw[:, 0], np.arange(1, n_iter + 1)) and len(si) == 2 * n_iter
    assert np.all(sw[:, 1] != sw[:, 2]) and np.all((sw[:, 1:3] >= 0) & (sw[:, 1:3] < 2)) and np.all(sw[:, 3] >= 2)
    assert np.array_equal(sw[:, 4], sw[:, 1] // int(params["n_chains"]))
    mine = si[si[:, 1] == 0]
    draws = np.array([GOFF[t] for t in mine[:, 3]]) + np.where(mine[:, 5] == 1, 3, 2)
    step_draws = np.bincount(mine[:, 0], weights=draws, minlength=n_iter + 1)[1:].astype(np.int64)
    want = step_draws + sw[:, 3] + (sw[:, 4] == 0)
    assert np.array_equal(np.diff(at), want)
    # the event's swap starts where the stream then stays on one side of 0.5 for the logged number of draws less one
    start = at[k - 1] + step_draws[k - 1]
    r = oracle.Rng(0)
    u = [r.rand_u() for _ in range(start + sw[k - 1, 3])][start:]
    assert len({int(2 * v) for v in u[:-1]}) == 1 and int(2 * u[-1]) != int(2 * u[0])


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_every_case_holds_its_event(name):
    E, S, n_procs, n_chains, seed, over, n_iter, k = rc.CASES[name]
    assert n_procs * n_chains == 2 and n_iter == k + 100
    sw = rc.oracle_run(name).swaplog()
    assert len(sw) == n_iter
    it, i1, i2, nd, jr = sw[k - 1]
    assert it == k and nd >= rc.MIN_PAIR_DRAWS, "%s: the swap of iteration %d takes %d draws: no fallback there" % (name, k, nd)
    assert (nd, i1, jr) == rc.EVENTS[name]


def test_the_table_covers_what_the_loops_need():
    rows = rc.CASES.values()
    assert any(S == 64 and "use_amp" not in o and "use_time" not in o and p == 1 for _, S, p, _, _, o, _, _ in rows)      # the specialised master
    assert any(S % 64 != 0 for _, S, *_ in rows)
    two = [n for n, r in rc.CASES.items() if r[2] == 2 and r[3] == 1]
    assert {rc.EVENTS[n][2] for n in two} == {0, 1}      # the judge draw on rank 0 and on rank 1


def test_fixture_c2_holds_its_event():
    """the golden fixture c2 passes through the fallback once, at iteration 3860 (three GPU tests run it to the end)"""
    from oracle import oracle

    _, data, params = load_case("c2")
    n_iter = int(params["n_iter"])
    job = oracle.Job(params, data); job.enable_swaplog(n_iter); job.run(n_iter)
    ev = rc.events(job.swaplog())
    assert list(ev[:, 0]) == [rc.C2_EVENT_ITER] and ev[0, 3] == 14
