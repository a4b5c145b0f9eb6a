"""The cases that the residual tests share (tests/test_locate_residuals.py on the CPU, tests/test_gpu_locate_residuals.py on the
device): keys of tests/locate_cases.py, whose volumes are computed once per process.  k_locate_residuals takes the stations in
blocks of 64 (kLocResSta): 63, 64 and 65 stand on both sides of one block, 130 on the far side of two."""
from tests import locate_cases as cases

STATIONS = (3, 63, 64, 65, 130)
PARITY = [(S, E, g, m) for S in STATIONS for E in (1, 5) for g in ("1x1x1", "5x3x2", "67x3x5") for m in ("both", "time", "amp")]
# 8400 cells: nine blocks of 1024 cells, the last one ragged; a row longer than a workgroup
LARGE = [(5, 1, "70x60x2", "both"), (4, 1, "300x3x1", "both")]
GPU_CASES = PARITY + LARGE + ["missing", "excluded"]
FP32_CASES = [(6, 2, "5x3x2", "both"), (65, 2, "67x3x5", "both")]


def case_id(key):
    return key if isinstance(key, str) else "%dsta-%dev-%s-%s" % key


def case(key):
    if key == "missing":
        return cases.missing_case()
    if key == "excluded":
        return cases.excluded_case()
    return cases.parity_case(*key)
