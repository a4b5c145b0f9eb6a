"""CPU: the batch plan of a residual request (htm_forward_locate_residuals; csrc/htm_locate_plan.hpp, locate.plan(residuals=True))
against a restatement of the formula as include/htm_hip.h states it, in the style of tests/test_locate_plan.py: every integer and
byte total exactly, for both precisions, with and without a prior, over that file's grids; the two budgets that the GPU test
quotes, as literals; that a request without residuals has the dict it had; the requests that no entry point makes."""
import numpy as np
import pytest

from hypotremormcmc_amd import _lib, locate
from tests import locate_cases as cases
from tests.test_locate_plan import MAX_ITEMS, SHAPES, grid_of, restated as restated_plain

BLOCK = 1024        # cells of a workgroup of the residual pass


def restated(n_sta, n_events, grid, mb, prior=False, precision="fp64"):
    """the plan of a residual request: htm_forward_locate's with the volume kept, plus the residual pass's arrays"""
    p, _ = restated_plain(n_sta, n_events, grid, mb, volume=True, prior=prior, precision=precision)
    cells, n_tiles = p["cells"], p["n_tiles"]
    n_rblk = (cells + BLOCK - 1) // BLOCK
    extra = dict(w=1, rbase=2 * n_sta + 4, rpart=n_rblk * (2 * n_sta + 6), res=4 * n_sta, fit=10)
    per_event = 8 * (n_tiles * p["stride"] + 16 + 2 * p["n_marg"] + cells + sum(extra.values())) + 80 * n_sta + 32
    assert per_event == p["per_event_bytes"] + 8 * sum(extra.values())
    quotient = mb * 1048576.0 / per_event
    limits = [65535, MAX_ITEMS // (max(n_tiles, n_rblk) * 256), (MAX_ITEMS - 256) // n_sta, int(min(quotient, 65535.0))]
    p["per_event"].update(extra)
    p.update(per_event_bytes=float(per_event), nb_limit=limits, nb=max(1, min([n_events] + limits)))
    return p


@pytest.mark.parametrize("mb", [None, "0.3", "37.5"])
def test_every_number_equals_the_restatement(monkeypatch, mb):
    if mb is None:
        monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    else:
        monkeypatch.setenv("HTM_LOCATE_MB", mb)
    n = 0
    for shape in SHAPES:
        for S in (3, 65, 300):
            for E in (1, 5, 70000):
                for prior in (False, True):
                    for precision in ("fp64", "fp32"):
                        want = restated(S, E, grid_of(*shape), 1024.0 if mb is None else float(mb), prior, precision)
                        got = locate.plan(S, E, grid_of(*shape), prior=prior, precision=precision, residuals=True)
                        assert got == want, (shape, S, E, prior, precision, mb)
                        n += 1
    assert n == len(SHAPES) * 36


def test_the_blocks_of_cells_bound_a_batch_where_they_outnumber_the_tiles(monkeypatch):
    monkeypatch.setenv("HTM_LOCATE_MB", "1e7")
    # 4096 x 5 x 3: 15 tiles of one row each, 60 blocks of 1024 cells
    p = locate.plan(3, 70000, grid_of(4096, 5, 3), residuals=True)
    assert p["n_tiles"] == 15 and p["nb_limit"][1] == MAX_ITEMS // (60 * 256) and locate.plan(3, 70000, grid_of(4096, 5, 3))["nb_limit"][1] == MAX_ITEMS // (15 * 256)
    # 1 x 300 x 2: four tiles, one block
    assert locate.plan(3, 70000, grid_of(1, 300, 2), residuals=True)["nb_limit"][1] == MAX_ITEMS // (4 * 256)


QUOTED = dict(n_sta=65, n_events=5, grid=cases.GRIDS["67x3x5"], prior=True)      # cases.parity_case(65, 5, "67x3x5", ..)


def test_the_batches_of_test_gpu_locate_residuals(monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    p = locate.plan(residuals=True, **QUOTED)
    # 385 + 16 + 150 + 1005 + 1 + 134 + 136 + 260 + 10 = 2097 doubles, 65 station records and the event's
    assert p["per_event_bytes"] == 22008.0 == 8 * 2097 + 80 * 65 + 32 and p["nb"] == 5
    assert p["per_event"]["rbase"] == 134 and p["per_event"]["rpart"] == 136 and p["per_event"]["res"] == 260 and p["per_event"]["fit"] == 10
    assert p["per_event"]["vol"] == 1005 and p["per_event"]["w"] == 1
    assert 22008 <= int(0.03 * 1048576) == 31457 < 2 * 22008 <= int(0.05 * 1048576) == 52428 < 3 * 22008
    monkeypatch.setenv("HTM_LOCATE_MB", "0.03")
    assert locate.plan(residuals=True, **QUOTED)["nb"] == 1
    monkeypatch.setenv("HTM_LOCATE_MB", "0.05")
    assert locate.plan(residuals=True, **QUOTED)["nb"] == 2


def test_a_request_without_residuals_keeps_its_dict(monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    p = locate.plan(**QUOTED)
    assert set(p["per_event"]) == {"sta", "ev", "part", "logz", "sum", "loc", "marg", "prior", "vol", "w"}
    assert p == restated_plain(65, 5, QUOTED["grid"], 1024.0, prior=True)[0] == locate.plan(residuals=False, **QUOTED)


def test_requests_that_no_entry_point_makes(monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    text = "libhtm_hip error -1: the residuals come under a fixed structure, without a volume and without a stack"
    for kw in (dict(job="marginal", n_draws=4), dict(job="draw_evidence", n_draws=4), dict(volume=True), dict(n_layer=1)):
        with pytest.raises(_lib.HtmError) as e:
            locate.plan(residuals=True, **dict(QUOTED, **kw))
        assert str(e.value) == text, kw
    with pytest.raises(ValueError):
        locate.plan(job="refine", residuals=True, **QUOTED)
    # the refusals of a plain request come first, with their texts
    with pytest.raises(_lib.HtmError, match="n_draws = 2 under a fixed structure: need 0"):
        locate.plan(residuals=True, n_draws=2, **QUOTED)
    bad = np.array(QUOTED["grid"])
    bad[2] = 0
    with pytest.raises(_lib.HtmError, match="grid axis x: 0 cells"):
        locate.plan(residuals=True, **dict(QUOTED, grid=bad))
