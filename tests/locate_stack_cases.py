"""The cases that tests/test_locate_stack.py (CPU: the restatement's side of every precondition) and
tests/test_gpu_locate_stack.py (the device) share: data, structures, grids and priors are those of tests/locate_cases.py, 6
stations and 7 events unless the case is a fixture of its own; the layerings; the workspace formula of include/htm_hip.h."""
import numpy as np

from tests import locate_cases as cases

N_STA, N_EVENTS = 6, 7
# non-monotone: the layer changes inside a batch, layer 1 stays empty, one window is switched off, one is out of range
LAYERS3 = [2, 0, 2, -1, 0, 7, 2]
LAYERINGS = {"one": (None, 1), "three": (LAYERS3, 3)}

# name -> (how to make the case, the events it has)
CASES = {
    "1x1x1": (lambda: cases.parity_case(N_STA, N_EVENTS, "1x1x1", "both"), N_EVENTS),
    "5x3x2": (lambda: cases.parity_case(N_STA, N_EVENTS, "5x3x2", "both"), N_EVENTS),
    "5x3x2 time": (lambda: cases.parity_case(N_STA, N_EVENTS, "5x3x2", "time"), N_EVENTS),
    "5x3x2 amp": (lambda: cases.parity_case(N_STA, N_EVENTS, "5x3x2", "amp"), N_EVENTS),
    "67x3x5": (lambda: cases.parity_case(N_STA, N_EVENTS, "67x3x5", "both"), N_EVENTS),
    "70x60x2": (lambda: cases.parity_case(N_STA, N_EVENTS, "70x60x2", "both"), N_EVENTS),
    "300x3x1": (lambda: cases.parity_case(N_STA, N_EVENTS, "300x3x1", "both"), N_EVENTS),
    "excluded": (cases.excluded_case, 3),
    "missing": (cases.missing_case, 5),
}
INDEPENDENT = ("5x3x2", "70x60x2")          # the cases that are also held against the independent restatement


def case(name):
    return CASES[name][0]()


def layering(name, which):
    """(layer [E] or None, n_layer) of the case"""
    layer, n_layer = LAYERINGS[which]
    return (None if layer is None else np.array(layer[:CASES[name][1]], dtype=np.int32)), n_layer


def workspace_bytes(grid, n_sta, n_events, n_layer, with_layer):
    """(once per call, per event of a batch) in bytes: the formula of include/htm_hip.h for a fixed structure"""
    nx, ny, nz = (int(grid[k]) for k in (2, 5, 8))
    cells = nx * ny * nz
    rows = max(1, min(ny, 256, 4096 // nx))
    n_tiles = nz * ((ny + rows - 1) // rows)
    stride = 4 + nx + 2 * rows
    per_event = 8 * (n_tiles * stride + cells + 1 + 2 * (nx + ny + nz) + 16) + 80 * n_sta + 32
    fixed = 8 * n_layer * (cells + nx * ny + nx * nz + ny * nz + 2) + (4 * n_events if with_layer else 0)
    return fixed, per_event
