"""Step 6 of the pipeline on the GPU: the build's counterpart of `hypo_tremor_statistics`
(reference src/hypo_tremor_statistics.f90, src/cls_statistics.f90).

The reference gathers every rank's recorded samples on rank 0, sorts each parameter's column with quick_sort
and prints three elements of it.  Here the three elements come from `htm_quantiles` (exact radix select on the
device, hypotremormcmc_amd/csrc/htm_select.hpp); files, names and formats are the reference's:

    uniform_structure.stat      Vs / Qs                      (src/cls_statistics.f90:394-431)
    station_corrections.stat    t_corr / a_corr per station  (:345-390)
    hypo.stat                   x, y, z per window           (:216-264)
    hypo.stat.removed           ... without double counts    (:120-211)

    python -m hypotremormcmc_amd.statistics <parameter file>      # in the directory of the step-5 outputs
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from . import _lib
from .run_files import Step5Run, read_sample_file  # noqa: F401 (read_sample_file: re-exported)

INT_MAX = 2 ** 31 - 1      # htm_quantiles takes int ranks and counts rows in int

HYPO_HEADER = ("# window ID, x (50%), x (2.5%) x (97.5%), y (50%), y (2.5%), y (97.5%)"
               "z (50 %), z (2.5%), z (97.5%)")
CORR_HEADER = ("# station name, t_corr (50%), t_corr (2.5%) t_corr (97.5%), a_corr (50%), a_corr (2.5%), "
               "a_corr (97.5%)")
VQ_HEADER = "# Vs (50%), Vs (2.5%) Vs (97.5%), Qs (50%), Qs (2.5%), Qs (97.5%)"


def expected_n_mod(n_iter, n_burn, n_procs, n_cool, n_interval) -> int:
    """src/cls_statistics.f90:64 (integer arithmetic, evaluated left to right)"""
    return (n_iter - n_burn) * n_procs * n_cool // n_interval


def ranks(n_mod: int):
    """il, im, iu of src/cls_statistics.f90:229-231: single-precision products truncated to integer"""
    f = np.float32
    return tuple(int(f(c) * f(n_mod)) for c in (0.025, 0.5, 0.975))


def sample_matrix(samples, what, *, n_seq=1, max_lag=1, name="samples", layout="[rows][n_par]", finite=True):
    """x [n_rows][n_par] float64 C-contiguous and n_draws = n_rows // n_seq: what every entry point that takes a sample matrix
    checks before any device call.  `what` says which C entry point counts the rows in int and how ("htm_diagnose takes"),
    `name` and `layout` name the argument.  n_seq None: the rows are no sequences (nothing about n_seq, n_par, max_lag is
    refused; n_draws is n_rows).  Quantiles of NaN are defined: `finite=False`."""
    shape = np.shape(samples)
    if len(shape) == 1:
        shape = (shape[0], 1)
    if len(shape) != 2:
        raise ValueError(f"{name} must be {layout}, got shape {shape}")
    n_rows, n_par = shape
    if n_rows > INT_MAX:      # ctypes would pass it on
        raise ValueError(f"rows = {n_rows} exceeds {INT_MAX}: {what} at most {INT_MAX} rows")
    if n_seq is not None:
        n_seq, max_lag = int(n_seq), int(max_lag)
        if n_seq < 1 or n_par < 1 or max_lag < 1 or max_lag > INT_MAX:
            raise ValueError(f"need n_seq >= 1, n_par >= 1 and 1 <= max_lag <= {INT_MAX} (got {n_seq}, {n_par}, {max_lag})")
        if n_rows % n_seq:
            raise ValueError(f"{n_rows} rows are not {n_seq} sequences of equal length")
    x = np.ascontiguousarray(samples, dtype=np.float64).reshape(shape)
    if finite and not np.isfinite(x).all():
        raise ValueError(f"{name} hold NaN or inf")
    return x, n_rows // (n_seq or 1)


def quantiles(samples: np.ndarray, n_mod: int | None = None, device: int = 0) -> np.ndarray:
    """[n_par][3] = (il-th, im-th, iu-th smallest) of every column of samples [n_rows][n_par], on the GPU.  NaN and inf are
    ordered, not refused: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, NaNs among themselves by payload."""
    x, n_rows = sample_matrix(samples, "htm_quantiles selects over", n_seq=None, finite=False)
    il, im, iu = ranks(n_rows if n_mod is None else n_mod)
    for what, v in (("n_mod", n_mod or 0), ("rank", max(il, im, iu))):
        if v > INT_MAX:        # ctypes.c_int would wrap silently; htm_quantiles counts rows in int
            raise ValueError(f"{what} = {v} exceeds {INT_MAX}: htm_quantiles selects over at most {INT_MAX} rows")
    rk = (C.c_int * 3)(il, im, iu)
    out = np.empty((x.shape[1], 3))
    _lib.check(_lib.load().htm_quantiles(device, _lib.ptr(x), n_rows, x.shape[1], rk, _lib.ptr(out)))
    return out          # columns: il (2.5 %), im (50 %), iu (97.5 %)


def hypo_rows(h):
    """hypo.stat's rows [n_win][9] = (median, 2.5 %, 97.5 %) of x, y, z from `quantiles`' [3 n_win][3] = (2.5 %, median, 97.5 %)
    of the columns x, y, z interleaved per window"""
    return [[h[3 * i + c][j] for c in range(3) for j in (1, 0, 2)] for i in range(len(h) // 3)]


def as_printed(rows):
    """the rows as hypo.stat's F13.6 prints them: the reference re-reads the text it just wrote before removing double counts
    (src/cls_statistics.f90:136-142)"""
    return [[float("%13.6f" % x) for x in r] for r in rows]


def remove_double_counts(win_id, q):
    """src/cls_statistics.f90:150-185.  q[i] = (x, x_lo, x_hi, y, y_lo, y_hi, z, z_lo, z_hi) of window i.
    Repeatedly drops a window whose id follows its predecessor's (in the current list) when both medians lie
    strictly inside the intersection of the two 95 % boxes.  Returns the indices kept."""
    keep = list(range(len(win_id)))
    while True:
        new, flag = [keep[0]], False
        for j in range(1, len(keep)):
            i, ii = keep[j], keep[j - 1]
            drop = False
            if win_id[i] == win_id[ii] + 1:
                inside = True
                for c in range(3):
                    med_i, lo_i, hi_i = q[i][3 * c:3 * c + 3]
                    med_p, lo_p, hi_p = q[ii][3 * c:3 * c + 3]
                    lo, hi = max(lo_i, lo_p), min(hi_i, hi_p)
                    inside = inside and lo < med_i and lo < med_p and hi > med_i and hi > med_p
                drop = inside
            if drop:
                flag = True
            else:
                new.append(i)
        keep = new
        if not flag:
            return keep


class Statistics:
    """`type statistics` of the reference: constructor arguments as src/cls_statistics.f90:50-53."""

    def __init__(self, n_procs, n_iter, n_burn, n_interval, n_cool, station_names, win_id, device=0):
        self.n_procs = int(n_procs)
        self.n_mod = expected_n_mod(int(n_iter), int(n_burn), self.n_procs, int(n_cool), int(n_interval))
        self.station_names = [str(s) for s in station_names]
        self.win_id = [int(w) for w in win_id]
        self.device = device
        if ranks(self.n_mod)[0] < 1:
            raise ValueError(f"n_mod = {self.n_mod}: il = int(0.025 * n_mod) = 0, the reference reads outside its "
                             f"sorted column; record at least 40 samples")

    # -- the three estimators; `*_samples` = all ranks' records stacked in rank order -----------------------
    def _q(self, samples):
        samples = np.asarray(samples, dtype=np.float64)
        if samples.shape[0] != self.n_mod:
            raise ValueError(f"{samples.shape[0]} samples recorded, the reference expects n_mod = {self.n_mod} "
                             f"(= (n_iter - n_burn) * n_procs * n_cool / n_interval)")
        return quantiles(samples, self.n_mod, self.device)

    def estimate_vs_qs(self, vs_samples, qs_samples, out_dir="."):
        v, q = self._q(vs_samples)[0], self._q(qs_samples)[0]
        with open(os.path.join(out_dir, "uniform_structure.stat"), "w") as fh:
            fh.write(VQ_HEADER + "\n")
            fh.write("".join("%13.6f" % x for x in (v[1], v[0], v[2], q[1], q[0], q[2])) + "\n")

    def estimate_corr_factors(self, t_corr_samples, a_corr_samples, out_dir="."):
        t, a = self._q(t_corr_samples), self._q(a_corr_samples)
        with open(os.path.join(out_dir, "station_corrections.stat"), "w") as fh:
            fh.write(CORR_HEADER + "\n")
            for k, name in enumerate(self.station_names):
                fh.write("%12s" % name.strip()[:12] +
                         "".join("%13.6f" % x for x in (t[k][1], t[k][0], t[k][2], a[k][1], a[k][0], a[k][2])) + "\n")

    def estimate_hypo(self, hypo_samples, out_dir="."):
        rows = hypo_rows(self._q(hypo_samples))
        self._write_hypo(os.path.join(out_dir, "hypo.stat"), range(len(rows)), rows)
        keep = remove_double_counts(self.win_id, as_printed(rows))
        self._write_hypo(os.path.join(out_dir, "hypo.stat.removed"), keep, rows)

    def _write_hypo(self, path, idx, rows):
        with open(path, "w") as fh:
            fh.write(HYPO_HEADER + "\n")
            for i in idx:
                fh.write("%9d" % self.win_id[i] + "".join("%13.6f" % x for x in rows[i]) + "\n")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit("USAGE: python -m hypotremormcmc_amd.statistics [parameter file]")
    run = Step5Run.open(argv[0])
    par = run.par
    st = Statistics(run.n_procs, par.get_n_iter(), par.get_n_burn(), par.get_n_interval(), par.get_n_cool(), par.stations, run.win_id, run.device)
    _, s = run.samples(("vs", "qs", "t_corr", "a_corr", "hypo"))
    st.estimate_vs_qs(s["vs"], s["qs"], run.work)
    st.estimate_corr_factors(s["t_corr"], s["a_corr"], run.work)
    st.estimate_hypo(s["hypo"], run.work)


if __name__ == "__main__":
    main()
