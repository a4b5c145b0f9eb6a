"""Time of the stacked density maps (htm_hypo_density_dev) on device-resident samples against two yardsticks: the read floor
(the bytes of hypo read once at the HBM peak) and the naive kernel (HTM_DENSITY_NAIVE=1: one global atomic per sample and
map).  Windows clustered with a standard deviation of `sd` km about centres spread over a 200 x 200 x 60 km box:

    0.5 km cells (400 x 400 x 120: the 2-D maps do not fit the LDS)     run-length + global atomics  |  naive
    4 km cells   (50 x 50 x 15: they fit)                               LDS maps  |  run-length + global atomics  |  naive

each with 1 layer and with 8 layers of neighbouring windows, maps only and with the volume, at sd = 2 km (the set-up of
DESIGN.md §3.9) and at sd = 0.1 km (a converged chain: a window's samples in a handful of cells).  Every path's counts are
compared with the first path's, and the maps' sums with the tally.

    python tools/bench_density.py [n_mod n_win]        # default 40000 1000
    python tools/bench_density.py --once               # one call of each default path, for a kernel trace
"""
import os
import sys

sys.path.insert(0, ".")
import numpy as np
import torch

from hypotremormcmc_amd import _lib

PEAK_BW = 8.0e12        # HBM3E peak of an MI355X, bytes/s
BOX = (200.0, 200.0, 60.0)


def main(argv):
    once = "--once" in argv
    argv = [a for a in argv if a != "--once"]
    n_mod, n_win = (int(a) for a in argv) if argv else (40000, 1000)
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    box = torch.tensor(BOX, dtype=torch.float64, device="cuda")
    centre = (0.1 + 0.8 * torch.rand(n_win, 3, dtype=torch.float64, device="cuda", generator=g)) * box
    noise = torch.randn(n_mod, n_win, 3, dtype=torch.float64, device="cuda", generator=g)
    s = torch.cuda.current_stream().cuda_stream
    floor_ms = 8.0 * n_mod * 3 * n_win / PEAK_BW * 1e3

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

    print(f"{n_mod} x {n_win} windows: {8e-9 * n_mod * 3 * n_win:.2f} GB of samples, read floor {floor_ms:.3f} ms at the 8 TB/s peak; "
          f"medians of 5 calls after 2, HIP events around each call (the call zeroes its outputs: that is in the time)")
    for sd in (2.0, 0.1):
        x = (centre[None] + sd * noise).view(n_mod, 3 * n_win).contiguous()
        for cell in (0.5, 4.0):
            n = [int(round(b / cell)) for b in BOX]
            grid = np.array([0.0, cell, n[0], 0.0, cell, n[1], 0.0, cell, n[2]], dtype=np.float64)
            fits = n[0] * n[1] + n[0] * n[2] + n[1] * n[2] <= 8192
            for n_layer in (1, 8):
                layer = None if n_layer == 1 else (torch.arange(n_win, device="cuda") * n_layer // n_win).to(torch.int32)
                for volume in (False, True):
                    u64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
                    outs = [u64(n_layer, n[1], n[0]), u64(n_layer, n[2], n[0]), u64(n_layer, n[2], n[1]),
                            u64(n_layer, n[2], n[1], n[0]) if volume else None, u64(n_layer, 2)]

                    def call():
                        _lib.check(lib.htm_hypo_density_dev(0, x.data_ptr(), 3 * n_win, n_mod, n_win, layer.data_ptr() if layer is not None else None,
                                                            n_layer, _lib.ptr(grid), *[o.data_ptr() if o is not None else None for o in outs], s))

                    paths = ([("LDS maps", {"HTM_DENSITY_LDS": "1"})] if fits else []) + [("run-length", {"HTM_DENSITY_LDS": "0"}),
                                                                                          ("naive", {"HTM_DENSITY_LDS": "0", "HTM_DENSITY_NAIVE": "1"})]
                    if once:
                        paths = paths[:1]
                    first, line = None, []
                    for name, env in paths:
                        for k in ("HTM_DENSITY_LDS", "HTM_DENSITY_NAIVE"):
                            os.environ.pop(k, None)
                        os.environ.update(env)
                        t = timed(call, 1, 0) if once else timed(call)
                        got = [o.cpu().numpy() for o in outs if o is not None]
                        inside = int(got[-1][:, 0].sum())
                        assert all(int(m.sum()) == inside for m in got[:-1]), "a map's sum is not the tally's inside"
                        assert int(got[-1].sum()) == n_mod * n_win
                        if first is None:
                            first = got
                        assert all(np.array_equal(a, b) for a, b in zip(got, first)), f"{name} counts differ"
                        line.append(f"{name} {t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f}) = {t[0] / floor_ms:6.1f} x floor")
                    for k in ("HTM_DENSITY_LDS", "HTM_DENSITY_NAIVE"):
                        os.environ.pop(k, None)
                    print(f"sd {sd:3.1f} km, cells {cell:3.1f} km ({n[0]} x {n[1]} x {n[2]}), {n_layer} layer(s), "
                          f"{'maps + volume' if volume else 'maps only    '}, {100.0 * (1 - inside / (n_mod * n_win)):4.1f} % outside: " + " | ".join(line), flush=True)
                    del outs
        del x


if __name__ == "__main__":
    main(sys.argv[1:])
