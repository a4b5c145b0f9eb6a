"""CPU: the host side of `locate --draws K --draw-weights` (hypotremormcmc_amd/locate.py: draw_weights, joint_draw_weights, the two
writers, the argument handling), what htm_forward_locate_draw_evidence refuses without a device, the restatement
(tests/locate_draws_restatement.py) on hand-made evidences, and the reference's side of the preconditions of
tests/test_gpu_locate_draws.py."""
import numpy as np
import pytest

from hypotremormcmc_amd import locate as lc
from tests import locate_draws_restatement as dr
from tests import locate_marginal_cases as mc

INF = np.inf


# ---- the restatement on hand-made evidences --------------------------------------------------------------------------------
def test_equal_columns_count_every_draw():
    for K in (1, 5, 9, 64):
        s = dr.summarise(np.full((2, K), -123.25))
        assert np.array_equal(s["n_eff"], [K, K]) and np.array_equal(s["w_max"], [1.0 / K] * 2) and list(s["k_max"]) == [0, 0]
        assert np.array_equal(s["log_evidence"], [-123.25] * 2)


def test_one_finite_column_is_one_draw():
    z = np.full((1, 7), -INF)
    z[0, 4] = 3.5
    s = dr.summarise(z)
    assert s["n_eff"][0] == 1.0 and s["w_max"][0] == 1.0 and s["k_max"][0] == 4
    assert abs(s["log_evidence"][0] - (3.5 - np.log(7.0))) < 1e-15


def test_no_cell_is_nan_and_minus_one():
    s = dr.summarise(np.full((2, 3), -INF))
    assert np.isnan(s["n_eff"]).all() and np.isnan(s["w_max"]).all() and np.isnan(s["log_evidence"]).all() and list(s["k_max"]) == [-1, -1]


def test_summary_against_plain_sums_and_ties():
    """where nothing underflows: the weights' plain forms; among equal largest values the lowest index"""
    rng = np.random.default_rng(4)
    z = rng.normal(-50.0, 1.5, (6, 11))
    z[2, 3] = z[2, 8] = z[2].max() + 1.0
    s = dr.summarise(z)
    w = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    assert np.allclose(s["n_eff"], 1.0 / (w * w).sum(axis=1), rtol=1e-13) and np.allclose(s["w_max"], w.max(axis=1), rtol=1e-13)
    assert np.allclose(s["log_evidence"], np.log(np.exp(z).mean(axis=1)), rtol=1e-13) and s["k_max"][2] == 3
    assert list(s["k_max"]) == [int(np.argmax(r)) for r in z]
    # far apart: the weights underflow, the result does not
    s = dr.summarise(np.array([[-1e5, -1e5 - 800.0, -2e5]]))
    assert s["n_eff"][0] == 1.0 and s["w_max"][0] == 1.0 and s["log_evidence"][0] == -1e5 - np.log(3.0)


def test_log_z_ref_leaves_excluded_cells_out_per_draw():
    """two cells, two draws, one event: a NaN cell and a -inf cell are left out of the draw they occur in, not of the other"""
    grid = np.array([0.0, 2.0, 2, 0.0, 1.0, 1, 0.0, 0.5, 1])
    ell_k = np.array([[[[[-1.0, np.nan]]]], [[[[-2.0, -3.0]]]], [[[[np.nan, -INF]]]]])          # [K][E][nz][ny][nx]
    case = {"grid": grid, "ell_k": ell_k, "log_prior": np.array([[[[0.5, -INF]]]])}
    flat = dr.log_z_ref(case, prior=False)
    assert flat.shape == (3, 1) and flat[0, 0] == -1.0 + 0.0 and flat[2, 0] == -INF             # (log of the cell volume: log 1)
    assert abs(flat[1, 0] - np.log(np.exp(-2.0) + np.exp(-3.0))) < 1e-15
    assert np.array_equal(dr.log_z_ref(case)[:, 0], [-0.5, -1.5, -INF])


# ---- draw_weights, joint_draw_weights ---------------------------------------------------------------------------------------
def test_draw_weights():
    z = np.array([[0.0, np.log(3.0), -INF], [-1e4, -1e4, -1e4], [-INF, -INF, -INF]])
    w = lc.draw_weights(z)
    assert np.allclose(w[0], [0.25, 0.75, 0.0], rtol=1e-15) and np.array_equal(w[1], [1 / 3] * 3) and np.isnan(w[2]).all()
    assert np.allclose(lc.draw_weights(z[0]), w[0], rtol=0, atol=0)
    s = dr.summarise(z)
    assert np.allclose(1.0 / (w[:2] ** 2).sum(axis=1), s["n_eff"][:2], rtol=1e-15) and np.allclose(w[:2].max(axis=1), s["w_max"][:2], rtol=1e-15)


def test_joint_draw_weights():
    z = np.array([[-10.0, -11.0, -12.0], [-INF, -INF, -INF], [-20.0, -19.0, -30.0]])            # (the window without a cell does not count)
    log_w, w = lc.joint_draw_weights(z)
    assert np.array_equal(log_w, [0.0, 0.0, -12.0]) and abs(w.sum() - 1.0) < 1e-15 and w[0] == w[1] and abs(w[2] / w[0] - np.exp(-12.0)) < 1e-18
    # a draw that leaves one window without a cell has no joint weight
    log_w, w = lc.joint_draw_weights(np.array([[-1.0, -INF], [-2.0, -1.0]]))
    assert np.array_equal(log_w, [0.0, -INF]) and np.array_equal(w, [1.0, 0.0])
    for none in (np.full((2, 3), -INF), np.array([[-1.0, -INF], [-INF, -1.0]])):
        log_w, w = lc.joint_draw_weights(none)
        assert np.isnan(log_w).all() and np.isnan(w).all()


# ---- the text of both files -------------------------------------------------------------------------------------------------
def test_text_of_the_draws_file():
    ev = {"n_eff": np.array([2.5, 1.0, np.nan]), "w_max": np.array([0.5, 0.987654321, np.nan]), "k_max": np.array([3, 0, -1]),
          "log_evidence": np.array([-1234.5678901, 2.0, np.nan])}
    text = lc.draws_text([7, 12, 400], ev, [1, 3, 5, 7, 9])
    lines = text.split("\n")
    assert lines[0] == lc.DRAWS_HEADER and lines[0].startswith("# window ID") and lines[-1] == "" and len(lines) == 5
    assert lines[1] == "        7       2.500000       0.500000    0.500000000        7   -1234.567890  0"          # (0.5 is not above 0.5)
    assert lines[2] == "       12       1.000000       0.200000    0.987654321        1       2.000000  1"
    assert lines[3] == "      400            NaN            NaN            NaN       -1            NaN  0"
    assert len({len(ln) for ln in lines[1:4]}) == 1


def test_text_of_the_structure_file():
    z = np.array([[-10.0, -11.0, -INF], [-20.0, -19.0, -30.0]])
    lines = lc.structure_text([2, 7, 12], [3.0, 3.125, 2.9], [250.0, 240.5, 260.0], z).split("\n")
    assert lines[0] == lc.STRUCTURE_HEADER and len(lines) == 5 and lines[-1] == ""
    assert lines[1] == "        2     3.000000   250.000000       0.000000    0.500000000"
    assert lines[2] == "        7     3.125000   240.500000       0.000000    0.500000000"
    assert lines[3] == "       12     2.900000   260.000000           -inf    0.000000000"


def test_summary_line():
    ev = {"n_eff": np.array([2.0, 7.5, np.nan, 1.25]), "w_max": np.array([0.6, 0.2, np.nan, 0.9])}
    assert lc.draws_summary_text(ev, 9) == ("the 9 draws' effective number per window: median 2.00, smallest 1.25; 2 windows where one draw outweighs "
                                            "all the others (w_max > 0.5: their intervals are one structure's)\n")
    assert lc.draws_summary_text({"n_eff": np.array([np.nan]), "w_max": np.array([np.nan])}, 4).count("\n") == 1


def test_read_structure_draws_gives_the_record_numbers(tmp_path):
    d = str(tmp_path)
    names = ["S001", "S002", "S003"]
    vs, qs, tc, ac = mc.write_calibration(d, names, n_ranks=2, n_rec=6)
    got = lc.read_structure_draws(d, names, 3, 5, records=True)
    assert len(got) == 5 and got[4] == [1, 3, 6, 8, 10] and np.array_equal(got[0], vs[got[4]])
    assert len(lc.read_structure_draws(d, names, 3, 5)) == 4


# ---- what needs no device -----------------------------------------------------------------------------------------------------
def test_draw_weights_without_draws_is_refused(capsys):
    """before the parameter file is opened: the one named here does not exist"""
    with pytest.raises(SystemExit) as e:
        lc.main(["no_such_file.in", "--cell", "5", "--draw-weights"])
    assert e.value.code == 2 and "--draw-weights needs --draws K" in capsys.readouterr().err


def test_null_handle_needs_no_device():
    lib = lc._lib.load()
    v, g = np.zeros(16), np.array([0.0, 1.0, 4, 0.0, 1.0, 3, 0.0, 1.0, 2])
    p = lc._lib.ptr
    assert lib.htm_forward_locate_draw_evidence(None, 2, p(v), p(v), p(v), p(v), p(g), None, p(v), None) == -1
    assert lib.htm_last_error().decode() == "NULL handle"


# ---- the preconditions of the GPU tests, on the reference alone -----------------------------------------------------------
def _reference_summaries(key, K, which):
    c = mc.marginal_case(key, K, which)
    return [dr.summarise(dr.log_z_ref(c, prior).T) for prior in (True, False)]


@pytest.mark.parametrize("key,K", [p for p in dr.PARITY if p[1] >= 2], ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_tight_draws_share_the_weight_of_a_window(key, K):
    """tight: every window has n_eff >= K / 2 -- a draw that is dropped, doubled, or a padding draw that is counted moves n_eff
    by a share of itself, far more than the tolerance of the GPU test (8e-12 A)"""
    for s in _reference_summaries(key, K, "tight"):
        print(f"{key}, K = {K}, tight: n_eff = {s['n_eff']}, w_max = {s['w_max']}")
        assert np.all(s["n_eff"] >= K / 2), (key, K, s["n_eff"])


@pytest.mark.parametrize("key,K", [p for p in dr.PARITY if p[1] >= 2 and p[0][3] != "amp"],
                         ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_wide_draws_leave_a_window_to_one_draw(key, K):
    """wide, with travel times: one draw outweighs all the others together, n_eff < 2 and w_max > 0.6 (the smallest margin: K = 33
    on 5x3x2, 1.87 and 0.63) -- the running maximum moves and most weights underflow.  With amplitudes alone the wide draws do
    NOT separate (n_eff up to 21.7 of 33: the amplitudes constrain the structure little), so those cases are not claimed here;
    they still run in the parity test."""
    for s in _reference_summaries(key, K, "wide"):
        print(f"{key}, K = {K}, wide: n_eff = {s['n_eff']}, w_max = {s['w_max']}")
        assert np.all(s["n_eff"] < 2.0) and np.all(s["w_max"] > 0.6), (key, K, s["n_eff"], s["w_max"])


def test_excluded_case_has_a_window_without_a_cell():
    c = mc.marginal_case("excluded", 3, "tight")
    z = dr.log_z_ref(c).T
    assert np.isfinite(z[:2]).all() and np.isneginf(z[2]).all()
    s = dr.summarise(z)
    # (event 0 shares its weight among the three draws, n_eff 2.7; event 1 is one draw's, n_eff 1.00001)
    assert list(s["k_max"] >= 0) == [True, True, False] and s["n_eff"][0] >= 1.5
