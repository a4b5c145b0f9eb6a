"""Step 2 on the HIP path: `hypo_tremor_correlate` (reference src/hypo_tremor_correlate.f90, src/cls_correlator.f90,
src/mod_signal_process.f90) -- the windowed cross-correlations step 3 reads.

    python -m hypotremormcmc_amd.correlate <parameter file>

Same inputs in the working directory (station file, `<sta>.merged.env`: a stream of (time, amplitude) float64 pairs),
same outputs, native little-endian streams as the reference writes them (src/cls_correlator.f90:246-251):

  * `<s1>.<s2>.corr`: per window w (1-based) and lag index j, the triplet (w-1)*t_step_corr + 0.5*t_win_corr,
    (j-n/2-1)*dt, cc -- 24 B per entry;
  * `<s1>.<s2>.max_corr`: (time, max_j cc) per window -- 16 B per entry.

Rules of the reference: dt is the difference of the LAST two times of an envelope file (src/hypo_tremor_correlate.f90:
78-86), a trailing unpaired value is ignored (:71-76), n = nint(t_win_corr/dt), n_step = nint(t_step_corr/dt),
n_win = (n_smp - n) / n_step truncated (src/cls_correlator.f90:78-80; no window when that is not positive), every
station must have the same n_smp and dt (:143-150), and n must be even (:179-182).

The correlograms are computed on the GPU (`htm_xcorr_dev`, one workgroup per window and pair, a direct circular sum
instead of FFTW's r2c / c2r: the values agree with the FFT form to rounding); there is no CPU fallback.  The pairs go
in batches whose correlogram buffer stays under HTM_XCORR_MB MiB of device memory (default 512); a batch holds at
least one pair, and the results do not depend on the batch size.  Deliberate deviation: a window of zero energy gives
an all-zero correlogram and cc_max = 0 (the reference correlates whatever its buffer held last).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys

import numpy as np

from . import _lib
from ._lib import check
from .param import Param
from .run_files import device_from_env

DEFAULT_XCORR_MB = 512


def nint(x: float) -> int:
    """Fortran nint: round half away from zero"""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def read_env(path):
    """-> (times, amplitudes) of a .merged.env stream; a trailing unpaired value is dropped"""
    if not os.path.exists(path):
        raise SystemExit(f"ERROR: cannot open {os.path.basename(path)}")
    v = np.fromfile(path, dtype="<f8")
    v = v[: v.size // 2 * 2].reshape(-1, 2)
    return v[:, 0].copy(), v[:, 1].copy()


def env_dt(times):
    """src/hypo_tremor_correlate.f90:79-85: t1 = 0, then dt = t2 - t1 for every record -- the last two times"""
    if times.size == 0:
        raise SystemExit("ERROR: empty envelope file")
    return float(times[-1] - (times[-2] if times.size > 1 else 0.0))


def window_count(n_smp: int, n: int, n_step: int) -> int:
    """int((n_smp - n) / n_step) with Fortran's truncation toward zero; no window when it is not positive"""
    q = abs(n_smp - n) // n_step
    return max(0, q if n_smp >= n else -q)


def pairs(stations):
    """station pairs in the reference's order, src/cls_correlator.f90:123-133"""
    return [(stations[i], stations[j]) for i in range(len(stations) - 1) for j in range(i + 1, len(stations))]


def window_times(n_win: int, t_step: float, t_win: float):
    """(w-1)*t_step + 0.5*t_win for w = 1..n_win (:246, :251)"""
    return np.array([(w - 1) * t_step + 0.5 * t_win for w in range(1, n_win + 1)])


def write_corr(path, cc, n, dt, t_step, t_win):
    """cc: (n_win, n) correlogram of one pair, row w in the reference's lag order"""
    n_win = cc.shape[0]
    out = np.empty((n_win, n, 3), dtype="<f8")
    out[:, :, 0] = window_times(n_win, t_step, t_win)[:, None]
    out[:, :, 1] = (np.arange(1, n + 1) - n // 2 - 1) * dt
    out[:, :, 2] = cc
    out.tofile(path)


def write_max_corr(path, cc_max, t_step, t_win):
    out = np.empty((cc_max.size, 2), dtype="<f8")
    out[:, 0] = window_times(cc_max.size, t_step, t_win)
    out[:, 1] = cc_max
    out.tofile(path)


def read_corr(path):
    """-> (n_entries, 3) array of a .corr stream"""
    v = np.fromfile(path, dtype="<f8")
    return v[: v.size // 3 * 3].reshape(-1, 3)


def read_max_corr(path):
    v = np.fromfile(path, dtype="<f8")
    return v[: v.size // 2 * 2].reshape(-1, 2)


MAX_WORK_ITEMS = 2 ** 32 - 1    # one launch: the dispatch packet holds the grid in work-items as a uint32


def xc_threads(n: int) -> int:
    """work-items per (window, pair) workgroup of htm_xcorr_dev: n rounded up to whole waves, at most 1024"""
    return min(1024, (n + 63) // 64 * 64)


def batch_pairs(n_win: int, n: int, mb=None) -> int:
    """pairs per batch whose correlograms (and cc_max) fit in HTM_XCORR_MB MiB, at least one, and whose launch of
    n_win * pairs workgroups stays below 2^32 work-items (htm_xcorr_dev refuses a single pair beyond that)"""
    if mb is None:
        mb = float(os.environ.get("HTM_XCORR_MB", DEFAULT_XCORR_MB))
    per_pair = 8 * n_win * (n + 1)
    launch = MAX_WORK_ITEMS // (n_win * xc_threads(n))
    return max(1, min(int(mb * (1 << 20)) // per_pair, launch))


class Envelopes:
    """every station's amplitudes on one device, rows of n_smp samples"""

    def __init__(self, amps, device=0):
        import torch

        self.n_sta, self.n_smp = amps.shape
        self.device = int(device)
        self.dev = torch.device("cuda", self.device)
        self.d_env = torch.from_numpy(np.ascontiguousarray(amps, dtype=np.float64)).to(self.dev)

    def correlate(self, n, n_step, n_win, pair0, n_pairs, d_cc=None, d_cc_max=None):
        """device correlograms [n_win*n][n_pairs] and cc_max [n_win][n_pairs] of pairs pair0 .. pair0+n_pairs-1"""
        import torch

        if d_cc is None:
            d_cc = torch.empty((n_win * n, n_pairs), dtype=torch.float64, device=self.dev)
            d_cc_max = torch.empty((n_win, n_pairs), dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            s = torch.cuda.current_stream().cuda_stream
            check(_lib.load().htm_xcorr_dev(self.device, C.c_void_p(self.d_env.data_ptr()), self.n_smp, self.n_smp,
                                            self.n_sta, n, n_step, n_win, pair0, n_pairs, C.c_void_p(d_cc.data_ptr()),
                                            d_cc.stride(0), C.c_void_p(d_cc_max.data_ptr()), s))
        return d_cc, d_cc_max


def load_envelopes(stations, directory="."):
    """-> (amplitudes (n_sta, n_smp), dt) with the reference's checks of equal n_smp and dt"""
    amps, dt0 = [], None
    for name in stations:
        t, a = read_env(os.path.join(directory, name + ".merged.env"))
        dt = env_dt(t)
        if amps and a.size != amps[0].size:
            raise SystemExit("ERROR: invalid n_smp")
        if dt0 is not None and dt != dt0:
            raise SystemExit("ERROR: invalid dt")
        amps.append(a); dt0 = dt
    return np.stack(amps), dt0


def geometry(t_win, t_step, dt, n_smp):
    """(n, n_step, n_win) of src/cls_correlator.f90:78-80"""
    if t_win < 0.0 or t_step < 0.0:
        raise SystemExit("ERROR: t_win and t_step must be > 0 (init_correlator)")
    n, n_step = nint(t_win / dt), nint(t_step / dt)
    if n_step < 1:
        raise SystemExit("ERROR: t_step_corr is shorter than half a sample")
    if n % 2:
        raise SystemExit("n2 + n2 /= n")
    return n, n_step, window_count(n_smp, n, n_step)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit("USAGE: hypo_tremor_correlate [parameter file]")
    para = Param(argv[0], verb=True, from_where="correlate")
    g = para.values
    amps, dt = load_envelopes(para.stations)
    n, n_step, n_win = geometry(g["t_win_corr"], g["t_step_corr"], dt, amps.shape[1])
    prs = pairs(para.stations)
    print(f" n_win= {n_win} n= {n} pairs= {len(prs)}", flush=True)
    if n_win == 0:
        for s1, s2 in prs:
            open(f"{s1}.{s2}.corr", "wb").close(); open(f"{s1}.{s2}.max_corr", "wb").close()
        return
    env = Envelopes(amps, device=device_from_env())
    b = batch_pairs(n_win, n)
    for p0 in range(0, len(prs), b):
        nb = min(b, len(prs) - p0)
        d_cc, d_mx = env.correlate(n, n_step, n_win, p0, nb)
        cc = d_cc.cpu().numpy().reshape(n_win, n, nb)
        mx = d_mx.cpu().numpy()
        for q in range(nb):
            s1, s2 = prs[p0 + q]
            write_corr(f"{s1}.{s2}.corr", cc[:, :, q], n, dt, g["t_step_corr"], g["t_win_corr"])
            write_max_corr(f"{s1}.{s2}.max_corr", mx[:, q], g["t_step_corr"], g["t_win_corr"])


if __name__ == "__main__":
    main()
