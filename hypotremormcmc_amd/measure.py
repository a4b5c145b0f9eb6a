"""Step 3 on the HIP path: `hypo_tremor_measure` (reference src/hypo_tremor_measure.f90, src/cls_measurer.f90:115-523)
-- the producer of the `detected_win.dat` and `opt_data.NNNNNN.dat` files steps 4 and 5 read.

    python -m hypotremormcmc_amd.measure <parameter file> [--from-envelopes]

Inputs in the working directory: station file, `<sta>.merged.env`, and (default) the `<s1>.<s2>.corr` /
`<s1>.<s2>.max_corr` files of step 2.  As in the reference:

  * dt = record 3 - record 1 of each envelope file; the stations must agree to 1e-8 (:134-147);
    n = nint(t_win_corr/dt), n_step = nint(t_step_corr/dt); n_win = the length of the .max_corr files, equal for
    every pair (:154-184);
  * a pair's threshold is the element of 1-based rank int(n*n_win*alpha) of its first n*n_win .corr values (:225-238)
    -- taken on the GPU by `htm_quantiles_dev`, without sorting; rank 0 is refused (the reference would index out of
    bounds);
  * a pair detects a window when cc_max >= threshold; a window is kept when MORE than n_pair_thred pairs detect it
    (:246-271);
  * the raw envelope windows of the kept windows (rec = 2*j, :340) are measured in one `htm_measure_windows` call
    (optimize_cc and optimize_amp, :405-523, one workgroup per window).

Outputs: `detected_win.dat` (id, (id-1)*t_step + 0.5*t_win), `cc_thred.dat` ("s1   s2", threshold) and
`opt_data.NNNNNN.dat` (x y z t t_stdv amp amp_stdv per station).  `trace.NNNNNN.dat` (:327-386, a plotting aid
nothing reads) is not written.  There is no CPU fallback.

`--from-envelopes` computes each pair batch's correlograms on the device (as `hypotremormcmc_amd.correlate` does,
same kernel, same batches under HTM_XCORR_MB), takes the thresholds and cc_max from device memory and never reads or
writes a .corr file; its outputs are bit-identical to `correlate` followed by plain `measure`.  Deliberate deviation:
a station of zero energy in a window has lag 0 against every station (the reference divides 0 by 0).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

from . import _lib, correlate as corr
from ._lib import check, ptr
from .param import Param
from .run_files import device_from_env

INT_MAX = 2 ** 31 - 1      # htm_quantiles_dev takes int ranks and counts rows in int


def envelope_dt(path):
    """records 1 and 3 of a .merged.env file (src/cls_measurer.f90:135-140)"""
    if not os.path.exists(path):
        raise SystemExit(f"ERROR: {os.path.basename(path)} does not exist")
    v = np.fromfile(path, dtype="<f8", count=3)
    if v.size < 3:
        raise SystemExit(f"ERROR: {os.path.basename(path)} holds fewer than 3 records")
    return float(v[2] - v[0])


def common_dt(stations, directory="."):
    dt, prev = None, None
    for i, s in enumerate(stations):
        dt = envelope_dt(os.path.join(directory, s + ".merged.env"))
        if i > 0 and abs(dt - prev) > 1.0e-8:
            raise SystemExit("invalid delta in envelope file")
        prev = dt
    return dt


def threshold_rank(n: int, n_win: int, alpha: float) -> int:
    """1-based rank of the threshold, int(n*n_win*alpha) (src/cls_measurer.f90:238)"""
    r = int(n * n_win * alpha)
    if n * n_win > INT_MAX:
        raise SystemExit(f"ERROR: {n * n_win} correlation values per pair (n = {n}, n_win = {n_win}) exceed the "
                         f"threshold select's limit of {INT_MAX}; use fewer windows per run")
    if r < 1:
        raise SystemExit(f"ERROR: alpha = {alpha} gives threshold rank {r} of {n * n_win} correlation values; "
                         "the rank must be at least 1")
    if r > n * n_win:
        raise SystemExit(f"ERROR: alpha = {alpha} gives threshold rank {r} beyond the {n * n_win} correlation values")
    return r


def detect(cc_max, thred, n_pair_thred):
    """cc_max (n_win, n_pair), thred (n_pair,) -> 1-based ids of the windows MORE than n_pair_thred pairs detect"""
    n_det = np.count_nonzero(np.asarray(cc_max) >= np.asarray(thred)[None, :], axis=1)
    return [int(w) + 1 for w in np.flatnonzero(n_det > n_pair_thred)]


def measure_windows(x, dt, device=0):
    """x (n_det, n_sta, n) raw windows -> t, t_stdv, amp, amp_stdv, each (n_det, n_sta)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n_det, n_sta, n = x.shape
    out = [np.empty((n_det, n_sta)) for _ in range(4)]
    check(_lib.load().htm_measure_windows(int(device), n_sta, n, float(dt), n_det, ptr(x), *(ptr(o) for o in out)))
    return tuple(out)


def gather_windows(amps, win_id, n, n_step):
    """raw windows of the kept windows: samples (id-1)*n_step .. +n-1 of every station's amplitudes
    (src/cls_measurer.f90:324-341)"""
    x = np.empty((len(win_id), len(amps), n))
    for d, w in enumerate(win_id):
        j1 = (w - 1) * n_step
        for s, a in enumerate(amps):
            if j1 + n > len(a):
                raise SystemExit(f"ERROR: window {w} runs past the end of an envelope file")
            x[d, s] = a[j1:j1 + n]
    return x


def write_detected_win(win_id, t_step, t_win, path="detected_win.dat"):
    with open(path, "w") as f:
        for w in win_id:
            f.write(" %d %.17g\n" % (w, (w - 1) * t_step + 0.5 * t_win))


def write_cc_thred(prs, thred, path="cc_thred.dat"):
    with open(path, "w") as f:
        for (s1, s2), v in zip(prs, thred):
            f.write(" %s   %s %.17g\n" % (s1, s2, v))


def write_opt_data(win_id, sta_x, sta_y, sta_z, t, t_stdv, amp, amp_stdv, directory="."):
    for d, w in enumerate(win_id):
        with open(os.path.join(directory, "opt_data.%06d.dat" % w), "w") as f:
            for s in range(len(sta_x)):
                f.write(" %s\n" % " ".join("%.17g" % v for v in (sta_x[s], sta_y[s], sta_z[s], t[d, s], t_stdv[d, s],
                                                                amp[d, s], amp_stdv[d, s])))


def _thresholds_dev(d_cc, n_mod, nb, rank, device):
    """rank-th smallest of each column of the device buffer [>= n_mod][nb]"""
    import torch

    if not (1 <= rank <= n_mod <= INT_MAX):      # ctypes.c_int would wrap silently
        raise ValueError(f"threshold rank {rank} of {n_mod} values: need 1 <= rank <= n_mod <= {INT_MAX}")
    out = torch.empty((nb, 3), dtype=torch.float64, device=d_cc.device)
    rk = (C.c_int * 3)(rank, rank, rank)
    with torch.cuda.device(d_cc.device):
        s = torch.cuda.current_stream().cuda_stream
        check(_lib.load().htm_quantiles_dev(int(device), C.c_void_p(d_cc.data_ptr()), n_mod, nb, d_cc.stride(0), rk,
                                            C.c_void_p(out.data_ptr()), s))
    return out[:, 0].cpu().numpy()


def scan_files(prs, n, alpha, device=0):
    """thresholds and cc_max of every pair from the .corr / .max_corr files"""
    import torch

    n_win = None
    for s1, s2 in prs:
        path = f"{s1}.{s2}.max_corr"
        if not os.path.exists(path):
            raise SystemExit(f"ERROR: {path} does not exist")
        nw = os.path.getsize(path) // 16
        if n_win is not None and nw != n_win:
            raise SystemExit("ERROR: invalid n_win in corr_max file")
        n_win = nw
    rank = threshold_rank(n, n_win, alpha)
    n_mod = n * n_win
    cc_max = np.empty((n_win, len(prs)))
    thred = np.empty(len(prs))
    b = corr.batch_pairs(n_win, n)
    dev = torch.device("cuda", int(device))
    for p0 in range(0, len(prs), b):
        nb = min(b, len(prs) - p0)
        host = np.empty((n_mod, nb))
        for q in range(nb):
            s1, s2 = prs[p0 + q]
            v = corr.read_corr(f"{s1}.{s2}.corr")
            if v.shape[0] < n_mod:
                raise SystemExit(f"ERROR: {s1}.{s2}.corr holds {v.shape[0]} values, {n_mod} expected")
            host[:, q] = v[:n_mod, 2]
            cc_max[:, q] = corr.read_max_corr(f"{s1}.{s2}.max_corr")[:, 1]
        thred[p0:p0 + nb] = _thresholds_dev(torch.from_numpy(host).to(dev), n_mod, nb, rank, device)
    return thred, cc_max, n_win


def scan_envelopes(env, n, n_step, n_win, n_pairs, alpha, device=0):
    """thresholds and cc_max of every pair from correlograms computed in device memory"""
    rank = threshold_rank(n, n_win, alpha)
    cc_max = np.empty((n_win, n_pairs))
    thred = np.empty(n_pairs)
    b = corr.batch_pairs(n_win, n)
    for p0 in range(0, n_pairs, b):
        nb = min(b, n_pairs - p0)
        d_cc, d_mx = env.correlate(n, n_step, n_win, p0, nb)
        thred[p0:p0 + nb] = _thresholds_dev(d_cc, n * n_win, nb, rank, device)
        cc_max[:, p0:p0 + nb] = d_mx.cpu().numpy()
    return thred, cc_max


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    from_env = "--from-envelopes" in argv
    args = [a for a in argv if a != "--from-envelopes"]
    if len(args) != 1:
        raise SystemExit("USAGE: hypo_tremor_measure [parameter file] [--from-envelopes]")
    para = Param(args[0], verb=True, from_where="measure")
    para.require("t_win_corr", "t_step_corr")
    g = para.values
    device = device_from_env()
    t_win, t_step = g["t_win_corr"], g["t_step_corr"]
    dt = common_dt(para.stations)
    n, n_step = corr.nint(t_win / dt), corr.nint(t_step / dt)
    prs = corr.pairs(para.stations)
    if from_env:
        amps, dt_c = corr.load_envelopes(para.stations)
        n_c, n_step_c, n_win = corr.geometry(t_win, t_step, dt_c, amps.shape[1])
        if (n_c, n_step_c) != (n, n_step):
            raise SystemExit(f"ERROR: the envelopes give n = {n_c}, n_step = {n_step_c} by step 2's rule and {n}, "
                             f"{n_step} by step 3's; run correlate and measure without --from-envelopes")
        env = corr.Envelopes(amps, device=device)
        thred, cc_max = scan_envelopes(env, n, n_step, n_win, len(prs), g["alpha"], device)
    else:
        amps = [corr.read_env(s + ".merged.env")[1] for s in para.stations]
        thred, cc_max, n_win = scan_files(prs, n, g["alpha"], device)
    win_id = detect(cc_max, thred, g["n_pair_thred"])
    print(f" # of detected events: {len(win_id)} out of {n_win}", flush=True)
    write_detected_win(win_id, t_step, t_win)
    write_cc_thred(prs, thred)
    if not win_id:
        return
    x = gather_windows(amps, win_id, n, n_step)
    t, t_stdv, amp, amp_stdv = measure_windows(x, dt, device)
    write_opt_data(win_id, para.sta_x, para.sta_y, para.sta_z, t, t_stdv, amp, amp_stdv)


if __name__ == "__main__":
    main()
