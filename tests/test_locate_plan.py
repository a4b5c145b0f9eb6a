"""CPU: the batch plan of the locate entry points (csrc/htm_locate_plan.hpp; htm_forward_locate_plan, locate.plan) against an
independent restatement of the workspace formula and the batch limits, written from the text of include/htm_hip.h and from the
function that held them before they were a unit of their own (locate_run_as of htm_forward.hip, the commit before this file):
every returned integer and byte total, exactly, over a grid of requests that holds every value at which a rule switches; the
byte counts that the comments of the GPU tests quote, as literals; every refusal, one fault at a time, with its text.  No GPU:
the plan makes no HIP call."""
import itertools

import numpy as np
import pytest

from hypotremormcmc_amd import _lib, locate
from tests import locate_cases as cases
from tests import locate_stack_cases as sc

INT_MAX = 2 ** 31 - 1
MAX_ITEMS = 2 ** 32 - 1           # a launch's work-items
BY_EVENTS, BY_TILES, BY_PACK, BY_BUDGET = range(4)      # htm_locate_plan::nb_limit


def grid_of(nx, ny, nz):
    return np.array([-44.0, 1.3, nx, -21.0, 14.0, ny, 0.5, 3.1, nz])


class Refused(Exception):
    pass


def restated(n_sta, n_events, grid, mb, job="fixed", n_draws=0, volume=False, prior=False, n_layer=0, layer=False, precision="fp64"):
    """the plan as the entry points made it before it had a unit of its own; raises Refused(the message)"""
    nx, ny, nz = (int(grid[k]) for k in (2, 5, 8))
    cells = nx * ny * nz
    if cells > INT_MAX:
        raise Refused("%d x %d x %d cells: more than 2^31 - 1" % (nx, ny, nz))
    rows = max(1, min(ny, 256, 4096 // nx))
    tpl = (ny + rows - 1) // rows
    stride = 4 + nx + 2 * rows
    n_tiles = nz * tpl
    nm = nx + ny + nz
    draws, evid, stacked = job != "fixed", job == "draw_evidence", n_layer > 0
    K = n_draws
    Kpad = (K + 7) // 8 * 8
    if evid:
        doubles = n_tiles * Kpad * 2 + K + 4 + nm
    else:
        doubles = n_tiles * stride + (cells if volume or stacked else 0) + 2 * nm + 16 + (1 if stacked else 0)
    per_event = 8 * doubles + 80 * n_sta + 32
    pair = 8 if precision == "fp32" else 16
    table = pair * (n_sta + 1) * Kpad + 8 * (2 * n_sta + 2) * K if draws else 0
    budget = mb * 1048576.0
    if draws and float(table + per_event) > budget:
        raise Refused("HTM_LOCATE_MB = %g: the table of %d draws (%d bytes) and one event (%d bytes) do not fit" % (mb, K, table, per_event))
    map_cells = nx * ny + nx * nz + ny * nz
    fixed = 0
    if stacked:
        n_out = n_layer * (cells + map_cells + 2)
        if n_out > INT_MAX:
            raise Refused("%d layers of %d + %d cells and a tally: more than 2^31 - 1 doubles" % (n_layer, cells, map_cells))
        fixed = 8 * n_out + (4 * n_events if layer else 0)
        if float(fixed + table + per_event) > budget:
            raise Refused("HTM_LOCATE_MB = %g: the stack of %d layers (%d bytes)%s and one event (%d bytes) do not fit"
                          % (mb, n_layer, fixed, ", the table of the draws" if draws else "", per_event))
    quotient = (budget - float(table) - float(fixed)) / float(per_event)
    limits = [65535, MAX_ITEMS // (n_tiles * 256), (MAX_ITEMS - 256) // n_sta, int(min(quotient, 65535.0))]
    nb = max(1, min([n_events] + limits))
    # the arrays that a call allocates, in elements: per event of a batch, and once per call
    per_event_len = dict(sta=n_sta, ev=1, part=n_tiles * Kpad * 2 if evid else n_tiles * stride, logz=K if evid else 0, sum=4 if evid else 0,
                         loc=0 if evid else 16, marg=0 if evid else nm, prior=nm if prior else 0,
                         vol=cells if (volume or stacked) and not evid else 0, w=1 if stacked else 0)
    nl = n_layer
    per_call_len = dict(dtc=K * n_sta, dac=K * n_sta, rk=2 * K, corr=n_sta * Kpad, vq=Kpad, stack=nl * cells, xy=nl * nx * ny, xz=nl * nx * nz,
                        yz=nl * ny * nz, tally=nl * 2, layer=n_events if stacked and layer else 0)
    if not draws:
        per_call_len.update(dtc=0, dac=0, rk=0, corr=0, vq=0)
    return dict(rows=rows, tpl=tpl, stride=stride, cells=cells, n_tiles=n_tiles, n_marg=nm, map_cells=map_cells, n_draws=K, n_draws_padded=Kpad,
                per_event=per_event_len, per_call=per_call_len, per_event_bytes=float(per_event), table_bytes=float(table), fixed_bytes=float(fixed),
                nb_limit=limits, nb=nb), quotient


def outcome(f, *a, **kw):
    """("plan", the plan) or ("refused", the message)"""
    try:
        r = f(*a, **kw)
        return "plan", (r[0] if isinstance(r, tuple) else r)
    except Refused as e:
        return "refused", str(e)
    except _lib.HtmError as e:
        text = str(e)
        assert text.startswith("libhtm_hip error -1: "), text      # HTM_EINVAL
        return "refused", text[len("libhtm_hip error -1: "):]


# ---- the grid of requests ------------------------------------------------------------------------------------------------------
# nx 1, 16, 17, 4096; rows = ny (16x3), = 256 (1x300: 4096 / nx and ny are larger), = 4096 / nx (17x300: 240); ny above rows, so
# that tpl > 1 (1x300, 17x300, 16x257, 4096x5)
SHAPES = [(1, 1, 1), (16, 3, 5), (1, 300, 2), (17, 300, 2), (16, 257, 1), (4096, 5, 3), (67, 3, 5)]
JOBS = [("fixed", 0)] + [(j, k) for j in ("marginal", "draw_evidence") for k in (1, 8, 9, 4096)]
STACKS = [(0, False), (1, False), (1, True), (3, True)]
BUDGETS = [None, "0.3", "37.5"]           # HTM_LOCATE_MB: the default, and two under which some shapes fit and some do not


def requests():
    for (job, K), (n_layer, layer), prior, volume, precision, S, E in itertools.product(JOBS, STACKS, (False, True), (False, True), ("fp64", "fp32"),
                                                                                        (3, 65, 300), (1, 5, 70000)):
        if job == "draw_evidence" and (volume or n_layer):       # no entry point makes that call
            continue
        yield dict(n_sta=S, n_events=E, job=job, n_draws=K, volume=volume, prior=prior, n_layer=n_layer, layer=layer, precision=precision)


def test_the_grid_holds_every_switch():
    rows = {s: restated(3, 1, grid_of(*s), 1024.0)[0] for s in SHAPES}
    assert rows[(16, 3, 5)]["rows"] == 3 and rows[(1, 300, 2)]["rows"] == 256 and rows[(17, 300, 2)]["rows"] == 4096 // 17
    assert rows[(4096, 5, 3)]["rows"] == 1 and rows[(1, 1, 1)]["tpl"] == 1
    assert all(rows[s]["tpl"] > 1 for s in ((1, 300, 2), (17, 300, 2), (16, 257, 1), (4096, 5, 3)))
    assert {s[0] for s in SHAPES} >= {1, 16, 17, 4096}
    rq = list(requests())
    assert {r["n_draws"] for r in rq} == {0, 1, 8, 9, 4096} and {r["job"] for r in rq} == {"fixed", "marginal", "draw_evidence"}
    assert {(r["n_layer"], r["layer"]) for r in rq} == set(STACKS)


@pytest.mark.parametrize("mb", BUDGETS)
def test_every_number_equals_the_restatement(monkeypatch, mb):
    if mb is None:
        monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    else:
        monkeypatch.setenv("HTM_LOCATE_MB", mb)
    seen = {"plan": 0, "refused": 0}
    binds = set()
    for shape in SHAPES:
        g = grid_of(*shape)
        for rq in requests():
            S, E = rq["n_sta"], rq["n_events"]
            kw = {k: v for k, v in rq.items() if k not in ("n_sta", "n_events")}
            want = outcome(restated, S, E, g, 1024.0 if mb is None else float(mb), **kw)
            got = outcome(locate.plan, S, E, g, **kw)
            assert got == want, (shape, rq, mb)
            seen[got[0]] += 1
            if got[0] == "plan":
                p = got[1]
                assert p["nb"] == max(1, min([E] + p["nb_limit"]))
                binds.add(min(range(4), key=lambda i: p["nb_limit"][i]) if p["nb"] < E else None)
    print(f"HTM_LOCATE_MB {mb}: {seen['plan']} plans, {seen['refused']} refusals; limits that bound a batch: {sorted(map(str, binds))}")
    assert seen["plan"] > 1000
    if mb is not None:
        assert seen["refused"] > 100


# ---- which limit binds ---------------------------------------------------------------------------------------------------------
def test_each_limit_on_the_batch_binds_once(monkeypatch):
    def planned(mb, S, E, shape, **kw):
        monkeypatch.setenv("HTM_LOCATE_MB", mb)
        p = locate.plan(S, E, grid_of(*shape), **kw)
        want, quotient = restated(S, E, grid_of(*shape), float(mb), **kw)
        assert p == want
        return p, quotient

    # 70000 events of next to nothing: the launch's grid, 65535 in y (the budget's quotient is far above it)
    p, q = planned("1024", 3, 70000, (1, 1, 1))
    assert p["nb"] == 65535 == p["nb_limit"][BY_EVENTS] and p["nb_limit"][BY_TILES] > 65535 and p["nb_limit"][BY_PACK] > 65535 and q > 65535.0
    # 4096 tiles of 256 threads per event: 2^32 - 1 work-items hold 4095 events
    p, q = planned("1e5", 3, 70000, (17, 1, 4096))
    assert p["n_tiles"] == 4096 and p["nb"] == 4095 == p["nb_limit"][BY_TILES]
    assert all(p["nb_limit"][i] > 4095 for i in (BY_EVENTS, BY_PACK, BY_BUDGET)) and q > 65535.0
    # 70000 stations: the pack kernel's thread per (event, station)
    p, q = planned("1e6", 70000, 70000, (1, 1, 1))
    assert p["nb"] == (MAX_ITEMS - 256) // 70000 == p["nb_limit"][BY_PACK] == 61356
    assert all(p["nb_limit"][i] > 61356 for i in (BY_EVENTS, BY_TILES, BY_BUDGET)) and q > 65535.0
    # the budget: one event of 17680 bytes in 0.02 MiB
    p, q = planned("0.02", 65, 5, (67, 3, 5), volume=True, prior=True)
    assert p["nb"] == 1 == p["nb_limit"][BY_BUDGET] and all(p["nb_limit"][i] > 5 for i in (BY_EVENTS, BY_TILES, BY_PACK)) and 1.0 < q < 2.0


# ---- the figures that the GPU tests quote ------------------------------------------------------------------------------------
QUOTED = dict(n_sta=65, n_events=5, grid=cases.GRIDS["67x3x5"], prior=True)      # cases.parity_case(65, 5, "67x3x5", ..) and 9 draws


def nb_under(monkeypatch, mb, **kw):
    monkeypatch.setenv("HTM_LOCATE_MB", mb)
    return locate.plan(**dict(QUOTED, **kw))["nb"]


def test_the_byte_counts_of_test_gpu_locate_draws(monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    p = locate.plan(job="draw_evidence", n_draws=9, **QUOTED)
    assert p["per_event_bytes"] == 7216.0 and p["table_bytes"] == 26400.0 and p["fixed_bytes"] == 0.0
    assert p["n_tiles"] == 5 and p["n_draws_padded"] == 16
    # 36700 bytes hold the table and one event (33616), not two (40832); 44040 the table and two events, not three (48048)
    assert 26400 + 7216 == 33616 <= int(0.035 * 1048576) == 36700 < 26400 + 2 * 7216 == 40832
    assert 40832 <= int(0.042 * 1048576) == 44040 < 26400 + 3 * 7216 == 48048
    assert nb_under(monkeypatch, "0.035", job="draw_evidence", n_draws=9) == 1
    assert nb_under(monkeypatch, "0.042", job="draw_evidence", n_draws=9) == 2


def test_the_batches_of_test_gpu_locate_and_marginal(monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    p = locate.plan(volume=True, **QUOTED)
    assert p["per_event_bytes"] == 17680.0 and p["nb"] == 5          # "17.3 KiB"
    assert nb_under(monkeypatch, "0.02", volume=True) == 1
    assert nb_under(monkeypatch, "0.04", volume=True) == 2
    assert nb_under(monkeypatch, "0.05", volume=True, job="marginal", n_draws=9) == 1
    assert nb_under(monkeypatch, "0.065", volume=True, job="marginal", n_draws=9) == 2
    # test_gpu_locate_fp32.py: the fp32 table of 9 draws and its input
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    assert locate.plan(volume=True, job="marginal", n_draws=9, precision="fp32", **QUOTED)["table_bytes"] == 17952.0


def test_the_batches_of_test_gpu_locate_stack(monkeypatch):
    g = cases.GRIDS["67x3x5"]
    fixed, per_event = sc.workspace_bytes(g, sc.N_STA, sc.N_EVENTS, 3, True)
    kw = dict(n_sta=sc.N_STA, n_events=sc.N_EVENTS, grid=g, prior=True, n_layer=3, layer=True)
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    p = locate.plan(**kw)
    assert (p["fixed_bytes"], p["per_event_bytes"]) == (float(fixed), float(per_event))
    for events, nb in ((1.5, 1), (3.5, 3)):
        monkeypatch.setenv("HTM_LOCATE_MB", repr((fixed + events * per_event) / 1048576.0))
        assert locate.plan(**kw)["nb"] == nb


# ---- refusals, one fault at a time ----------------------------------------------------------------------------------------------
def refused(monkeypatch, mb, text, **kw):
    if mb is None:
        monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    else:
        monkeypatch.setenv("HTM_LOCATE_MB", mb)
    with pytest.raises(_lib.HtmError) as e:
        locate.plan(**dict(QUOTED, **kw))
    assert str(e.value) == "libhtm_hip error -1: " + text


def test_refusals(monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    assert locate.plan(**QUOTED)["nb"] == 5          # nothing is wrong with the request itself
    bad = grid_of(67, 3, 5)
    bad[2] = 0
    refused(monkeypatch, None, "grid axis x: 0 cells: need an integer in 1..4096", grid=bad)
    bad = grid_of(67, 3, 5)
    bad[4] = -14.0
    refused(monkeypatch, None, "grid axis y: origin -21, cell size -14: need a finite origin and a finite cell size > 0", grid=bad)
    refused(monkeypatch, None, "4096 x 4096 x 128 cells: more than 2^31 - 1", grid=grid_of(4096, 4096, 128))
    refused(monkeypatch, "0", "HTM_LOCATE_MB = 0: a positive number of MiB")
    refused(monkeypatch, "-1e0", "HTM_LOCATE_MB = -1e0: a positive number of MiB")
    refused(monkeypatch, "some", "HTM_LOCATE_MB = some: a positive number of MiB")
    # the grid is looked at before the budget
    refused(monkeypatch, "0", "4096 x 4096 x 128 cells: more than 2^31 - 1", grid=grid_of(4096, 4096, 128))
    for job, per_event in (("marginal", 9640), ("draw_evidence", 7216)):
        # less than the table; the table fits, an event with it does not
        refused(monkeypatch, "0.01", "HTM_LOCATE_MB = 0.01: the table of 9 draws (26400 bytes) and one event (%d bytes) do not fit" % per_event,
                job=job, n_draws=9)
        refused(monkeypatch, "0.03", "HTM_LOCATE_MB = 0.03: the table of 9 draws (26400 bytes) and one event (%d bytes) do not fit" % per_event,
                job=job, n_draws=9)
    # 2^29 cells, which one layer may have, in four layers
    refused(monkeypatch, None, "4 layers of 536870912 + 17039360 cells and a tally: more than 2^31 - 1 doubles", grid=grid_of(4096, 4096, 32),
            n_layer=4, layer=True, prior=False)
    # the stack and half an event
    g = cases.GRIDS["67x3x5"]
    fixed, per_event = sc.workspace_bytes(g, sc.N_STA, sc.N_EVENTS, 3, True)
    kw = dict(n_sta=sc.N_STA, n_events=sc.N_EVENTS, grid=g, n_layer=3, layer=True)
    mb = (fixed + 0.5 * per_event) / 1048576.0
    refused(monkeypatch, repr(mb), "HTM_LOCATE_MB = %g: the stack of 3 layers (%d bytes) and one event (%d bytes) do not fit" % (mb, fixed, per_event), **kw)
    table = 16 * (sc.N_STA + 1) * 16 + 8 * (2 * sc.N_STA + 2) * 9
    mb = (fixed + table + 0.5 * per_event) / 1048576.0
    refused(monkeypatch, repr(mb), "HTM_LOCATE_MB = %g: the stack of 3 layers (%d bytes), the table of the draws and one event (%d bytes) do not fit"
            % (mb, fixed, per_event), job="marginal", n_draws=9, **kw)


def test_requests_that_no_entry_point_makes(monkeypatch):
    monkeypatch.delenv("HTM_LOCATE_MB", raising=False)
    for text, kw in (("n_sta and n_events must be positive", dict(n_sta=0)), ("n_sta and n_events must be positive", dict(n_events=0)),
                     ("n_draws = 0: need 1..4096", dict(job="marginal")), ("n_draws = 4097: need 1..4096", dict(job="draw_evidence", n_draws=4097)),
                     ("n_draws = 2 under a fixed structure: need 0", dict(n_draws=2)),
                     ("n_layer = 3 without a layer per window", dict(n_layer=3)),
                     ("the draws' evidences come without a volume and without a stack", dict(job="draw_evidence", n_draws=2, volume=True))):
        refused(monkeypatch, None, text, **kw)
    with pytest.raises(ValueError):
        locate.plan(job="refine", **QUOTED)
