"""Time of the convergence diagnostics (htm_diagnose_dev: k_diag_mean, k_diag_acov, k_diag_finish) on device-resident
samples, against the fp64 FMA floor of the autocovariances: S n (L + 1) n_par fused multiply-adds at the 78.6 TFLOP/s
(39.3 T FMA/s) fp64 vector peak DESIGN.md uses.

    python tools/bench_diagnose.py [n_rows n_par n_seq max_lag]        # default 80000 3130 20 1000
"""
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from hypotremormcmc_amd import _lib

PEAK_FMA = 78.6e12 / 2


def time_ms(n_rows, n_par, n_seq, max_lag, reps=5, warmup=2, seed=3):
    """milliseconds of `reps` calls after `warmup`, by HIP events around each call; and the out array of the last"""
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n_rows, n_par, dtype=torch.float64, device="cuda", generator=g)
    out = torch.empty(n_par, 4, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ms = []
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.htm_diagnose_dev(0, x.data_ptr(), n_seq, n_rows // n_seq, n_par, n_par, max_lag, out.data_ptr(), None, s))
        e1.record()
        e1.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms, out.cpu().numpy()


def fma_count(n_rows, n_par, n_seq, max_lag):
    n = n_rows // n_seq // 2
    return 2 * n_seq * n * (min(n - 1, max_lag) + 1) * n_par


def main(argv):
    n_rows, n_par, n_seq, max_lag = (int(a) for a in argv) if argv else (80000, 3130, 20, 1000)
    ms, out = time_ms(n_rows, n_par, n_seq, max_lag)
    med = float(np.median(ms))
    floor = 1e3 * fma_count(n_rows, n_par, n_seq, max_lag) / PEAK_FMA
    print(f"{n_rows} x {n_par}, {n_seq} sequences, max_lag {max_lag}: median {med:.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}, "
          f"{len(ms)} calls), fp64 FMA floor {floor:.2f} ms = {floor / med:.2f} of the time; "
          f"R-hat <= {np.nanmax(out[:, 0]):.4f}, ESS >= {np.nanmin(out[:, 1]):.0f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
