"""Time of the location error ellipsoids (htm_hypo_ellipsoid_dev) on device-resident samples, part by part, with the bytes
each part has to move, and for comparison the same second moments formed with torch on the device (centre, then a batched
einsum).  The parts are timed by ending the call early (HTM_ELL_STOP=mean|moments|finish) and taking differences:

    mean        k_ell_range + k_ell_mean + k_ell_stats     two passes over the samples
    moments     k_ell_moments                              one pass
    finish      k_ell_finish                               the slabs' partial sums
    distances   k_ell_maha + htm_quantiles_dev + k_ell_setq  one pass, d2 written once and read by 16 select passes

    python tools/bench_ellipsoid.py [n_mod n_win n_piv]        # default 80000 1043 2 (3 129 columns, as tools/bench_select.py)
"""
import os
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from hypotremormcmc_amd import _lib

PEAK_BW = 8.0e12        # HBM3E peak of an MI355X, bytes/s


def main(argv):
    n_mod, n_win, n_piv = (int(a) for a in argv) if argv else (80000, 1043, 2)
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(n_mod, 3 * n_win, dtype=torch.float64, device="cuda", generator=g)
    x += 0.3
    piv = torch.randn(n_mod, max(n_piv, 1), dtype=torch.float64, device="cuda", generator=g)
    out = torch.empty(n_win, 22, dtype=torch.float64, device="cuda")
    corr = torch.empty(n_win, 3, max(n_piv, 1), dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    rank = int(np.ceil(0.68 * n_mod))

    def timed(fn, reps=5, warmup=2):
        ms = []
        for rep in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= warmup:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), min(ms), max(ms)

    def call():
        _lib.check(lib.htm_hypo_ellipsoid_dev(0, x.data_ptr(), 3 * n_win, piv.data_ptr() if n_piv else None, max(n_piv, 1), n_mod, n_win,
                                              n_piv, rank, out.data_ptr(), corr.data_ptr() if n_piv else None, s))

    t = {}
    for stop in ("mean", "moments", "finish", None):
        if stop:
            os.environ["HTM_ELL_STOP"] = stop
        else:
            os.environ.pop("HTM_ELL_STOP", None)
        t[stop or "whole"] = timed(call)

    def torch_moments():
        xc = (x - x.mean(dim=0)).view(n_mod, n_win, 3)
        return torch.einsum("iwa,iwb->wab", xc, xc)

    t_torch = timed(torch_moments)
    ref = (torch_moments() / (n_mod - 1)).cpu().numpy()
    o = out.cpu().numpy()
    c = o[:, 3:9]
    cov = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)
    sample = 8.0 * n_mod * (3 * n_win + n_piv)
    d2 = 8.0 * n_mod * n_win
    parts = [("mean", t["mean"][0], 2 * sample), ("moments", t["moments"][0] - t["mean"][0], sample),
             ("finish", t["finish"][0] - t["moments"][0], 0.0), ("distances", t["whole"][0] - t["finish"][0], sample + 17 * d2)]
    print(f"{n_mod} x {n_win} windows ({3 * n_win} columns), {n_piv} pivots, rank {rank}; medians of 5 calls after 2, HIP events around each call")
    for name, ms, nbytes in parts:
        rate = f"{nbytes / 1e9:8.2f} GB algorithmic = {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s" if nbytes else "   (partial sums only)"
        print(f"{name:10s} {ms:9.3f} ms  {rate}")
    for k in ("mean", "moments", "finish", "whole"):
        print(f"call ended after {k:8s} {t[k][0]:9.3f} ms (min {t[k][1]:.3f}, max {t[k][2]:.3f})")
    mm = t["moments"][0]
    print(f"k_ell_range + k_ell_mean + k_ell_stats + k_ell_moments: {3 * sample / 1e9:.2f} GB in {mm:.3f} ms = "
          f"{3 * sample / (mm * 1e-3) / 1e12:.2f} TB/s = {3 * sample / (mm * 1e-3) / PEAK_BW:.3f} of the 8 TB/s peak")
    print(f"torch (x - mean, einsum iwa,iwb->wab)  {t_torch[0]:9.3f} ms (min {t_torch[1]:.3f}, max {t_torch[2]:.3f}); "
          f"largest |cov - torch's| / (sigma_a sigma_b) = {np.max(np.abs(cov - ref) / np.sqrt(np.einsum('waa->wa', ref)[:, :, None] * np.einsum('waa->wa', ref)[:, None, :])):.2e}")
    print(f"q / 3.5058823558 (Gaussian input): median {np.median(o[:, 21]) / 3.5058823558:.4f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
