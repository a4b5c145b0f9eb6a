"""CPU: the specialised chain master's batch of LDS reads at its turn (csrc/htm_flow.hpp FlowTurn, DESIGN.md 3.0 "from the turn to
the decision") in the protocol model, tools/flow_protocol_sim.py with batched=True: with every poll of the turn a wave reads,
behind the checks and the epoch and in this order, its own temperature of the iteration before, the plan of that iteration's
swap, every chain's committed key and every chain's (T, L) -- each a separate shared-memory access the scheduler may switch at.
The plan is used only if that same round lets the turn pass, the partner's record only if that same round's committed key shows
the partner's commit; otherwise the wave spins on the key and reads the record behind it.  Everything -- every step's start
position, final states, temperatures, stream position -- must equal the serial loop, at 1, 2, 3, 4, 5 and 8 chains, with
rejections (epochs adopted while turns poll: batches dropped), stop requests and a straggling wave."""
import importlib.util
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _sim():
    spec = importlib.util.spec_from_file_location("flow_protocol_sim", os.path.join(ROOT, "tools", "flow_protocol_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("first", [1, 101, 201, 301])
def test_batched_turn_equals_the_serial_loop(first):
    sim = _sim()
    stats = {}
    for seed in range(first, first + 100):
        assert sim.run_case(seed, batched=True, stats=stats), "seed %d differs from the serial loop" % seed
    # both ways to the partner's record ran, and epochs changed (batches were dropped)
    assert stats["hits"] > 100 and stats["misses"] > 20 and stats["epochs"] > 100, stats


def test_the_model_catches_a_record_read_ahead_of_its_key():
    """the model's own check: with the records read BEFORE the committed keys that validate them, some interleaving gives a
    stale (T, L) to a swap decision -- the model must find it"""
    sim = _sim()
    assert not all(sim.run_case(seed, batched="records first") for seed in range(1, 101))
