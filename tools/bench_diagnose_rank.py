"""Time of the rank-normalised diagnostics (htm_rank.hpp) on device-resident samples, by HIP events around the
_dev calls: htm_rank_normalize_dev split into its three kernels (HTM_RANK_STOP=keys|sort ends every batch after that kernel;
the parts are differences of the three times), the whole htm_diagnose_rank_dev, torch.sort(dim=0) of the same matrix for
comparison, and four times htm_diagnose_dev, which the four R-hat / ESS evaluations inside cannot be faster than.

    python tools/bench_diagnose_rank.py [n_rows n_par n_seq max_lag]        # default 80000 3130 20 1000

The sort's traffic is what k_rank_sort asks of memory: one read of the keys for the 8 histograms, then 8 passes that read
and write them, 17 x 8 B per element, as a fraction of the 8 TB/s HBM peak DESIGN.md uses.
"""
import os
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from hypotremormcmc_amd import _lib

PEAK_BW = 8e12
PARENT_DIAGNOSE_MS = 11.97          # profiles/diagnose_bench.txt


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


def main(argv):
    n_rows, n_par, n_seq, max_lag = (int(a) for a in argv) if argv else (80000, 3130, 20, 1000)
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(n_rows, n_par, dtype=torch.float64, device="cuda", generator=g)
    z = torch.empty_like(x)
    out = torch.empty(n_par, 4, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    normalize = lambda: _lib.check(lib.htm_rank_normalize_dev(0, x.data_ptr(), n_rows, n_par, n_par, 0, z.data_ptr(), n_par, None, s))
    t = {}
    for stop in ("keys", "sort", None):
        if stop:
            os.environ["HTM_RANK_STOP"] = stop
        else:
            os.environ.pop("HTM_RANK_STOP", None)
        t[stop] = timed(normalize)
    keys, sort, zz = t["keys"][0], t["sort"][0] - t["keys"][0], t[None][0] - t["sort"][0]
    whole = timed(lambda: _lib.check(lib.htm_diagnose_rank_dev(0, x.data_ptr(), n_seq, n_rows // n_seq, n_par, n_par, max_lag, out.data_ptr(), s)))
    plain = timed(lambda: _lib.check(lib.htm_diagnose_dev(0, x.data_ptr(), n_seq, n_rows // n_seq, n_par, n_par, max_lag, out.data_ptr(), None, s)))
    del z
    tsort = timed(lambda: torch.sort(x, dim=0))
    o = out.cpu().numpy()
    moved = 17 * 8 * n_rows * n_par
    print(f"{n_rows} x {n_par}, {n_seq} sequences, max_lag {max_lag}, HTM_RANK_MB {os.environ.get('HTM_RANK_MB', '2048 (default)')}; medians of 5 calls after 2")
    print(f"htm_rank_normalize_dev   {t[None][0]:9.2f} ms (min {t[None][1]:.2f}, max {t[None][2]:.2f}): keys {keys:.2f}, sort {sort:.2f}, z {zz:.2f}")
    print(f"torch.sort(dim=0)        {tsort[0]:9.2f} ms (min {tsort[1]:.2f}, max {tsort[2]:.2f}): the transform takes {t[None][0] / tsort[0]:.2f} x, k_rank_sort alone {sort / tsort[0]:.2f} x")
    print(f"k_rank_sort traffic      {moved / 1e9:9.2f} GB in {sort:.2f} ms = {moved / (sort * 1e-3) / 1e12:.2f} TB/s = {moved / (sort * 1e-3) / PEAK_BW:.3f} of 8 TB/s")
    print(f"htm_diagnose_rank_dev    {whole[0]:9.2f} ms (min {whole[1]:.2f}, max {whole[2]:.2f})")
    print(f"htm_diagnose_dev         {plain[0]:9.2f} ms here, {PARENT_DIAGNOSE_MS} ms in profiles/diagnose_bench.txt; four of them {4 * plain[0]:.2f} ms "
          f"({4 * PARENT_DIAGNOSE_MS:.2f} ms) = {4 * plain[0] / whole[0]:.2f} of htm_diagnose_rank_dev")
    print(f"rank R-hat <= {np.nanmax(o[:, :2]):.4f}, bulk-ESS >= {np.nanmin(o[:, 2]):.0f}, tail-ESS >= {np.nanmin(o[:, 3]):.0f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
