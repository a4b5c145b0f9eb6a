"""Step 1 benchmark on the GPU: htm_convert_dev at 100 Hz, n = 300000 (t_win_conv = 3000 s) over many station-days,
timed with device events; the batched FFT alone (achieved bytes/s against the 6.29 TB/s measured copy rate); and the
program's wall time on SAC files with the share spent reading files and copying to the device.

    python tools/bench_convert.py [--days 60] [--file-days 2] [--out profiles/convert_bench.txt]

Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--days 4 --file-days 0)."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from hypotremormcmc_amd import _lib, convert, synth  # noqa: E402

COPY_TBS = 6.29


def device_run(days, lines):
    import torch

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    c = convert.constants(float(np.float32(0.01)), 3000.0)
    N = int(days * 86400 * 100)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x1 = torch.randn(N, generator=g, device=dev, dtype=torch.float32)
    x2 = torch.randn(N, generator=g, device=dev, dtype=torch.float32)
    n, n2 = c.n, c.n // 2
    last = convert.last_segment(N, n)
    b = convert.batch_segments(n)
    kb = (C.c_int * 4)(*c.k_band)
    out = torch.empty(-(-N // c.n_fac), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream()

    def once():
        for j0 in range(0, last + 1, b):
            j1 = min(last, j0 + b - 1)
            k0, _ = convert.outputs(N, n, c.n_fac, j0, j1)
            off = j0 * n2
            _lib.check(lib.htm_convert_dev(0, C.c_void_p(x1.data_ptr() + 4 * off), C.c_void_p(x2.data_ptr() + 4 * off),
                                           N, n, c.n_fac, c.h, kb, 1.0, 1.0, j0, j1,
                                           C.c_void_p(out.data_ptr() + 8 * k0), C.c_void_p(st.cuda_stream)))

    once()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        once()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = min(times)
    lines.append(f"device: {days} station-days at 100 Hz (N = {N}), n = {n}, {last + 1} segments, {b} per batch")
    lines.append(f"  htm_convert_dev: {ms:.2f} ms per run (best of 3: {', '.join('%.2f' % t for t in times)}),"
                 f" {ms / days:.3f} ms per station-day, {1e3 * ms / (last + 1):.1f} us per segment")
    # the FFT alone: 2 b rows backward, the transform the segment pays twice, plus the packed forward one
    rows = 2 * b
    y = torch.randn(rows, n, 2, generator=g, device=dev, dtype=torch.float64)
    passes = 9                                                          # 300000 = 4 4 2 3 5^5
    for _ in range(2):
        _lib.check(lib.htm_fft_dev(0, C.c_void_p(y.data_ptr()), n, C.c_void_p(y.data_ptr()), n, n, rows, 1,
                                   C.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    e0.record()
    for _ in range(reps):
        _lib.check(lib.htm_fft_dev(0, C.c_void_p(y.data_ptr()), n, C.c_void_p(y.data_ptr()), n, n, rows, 1,
                                   C.c_void_p(st.cuda_stream)))
    e1.record()
    torch.cuda.synchronize()
    fft_ms = e0.elapsed_time(e1) / reps
    moved = passes * rows * n * 32 + (passes % 2) * rows * n * 32       # in place, odd pass count: a final copy
    lines.append(f"  FFT alone: {rows} rows of {n}, {passes} Stockham passes + copy, {fft_ms:.3f} ms,"
                 f" {moved / fft_ms / 1e9:.2f} TB/s of reads and writes ({100 * moved / fft_ms / 1e9 / COPY_TBS:.0f}% of"
                 f" the {COPY_TBS} TB/s copy rate)")


def file_run(days, lines):
    with tempfile.TemporaryDirectory() as d:
        fs = 100.0
        rng = np.random.default_rng(2)
        ids = [f"day{k:03d}" for k in range(int(days))]
        paths = []
        for tid in ids:
            pair = []
            for cmp in ("EH1", "EH2"):
                p = os.path.join(d, "data", "S1", f"{tid}.{cmp}")
                synth.write_sac(p, rng.standard_normal(int(86400 * fs)).astype(np.float32), 1.0 / fs, big_endian=True)
                pair.append(p)
            paths.append(tuple(pair))
        t0 = time.perf_counter()
        st = convert.plan_station("S1", paths, (1.0, 1.0), 3000.0)
        t1 = time.perf_counter()
        stats = {}
        convert.convert_station(st, os.path.join(d, "S1.merged.env"), device=0, stats=stats)
        t2 = time.perf_counter()
        stats = {}
        convert.convert_station(st, os.path.join(d, "S1.merged.env"), device=0, stats=stats)
        t3 = time.perf_counter()
    wall = t3 - t2
    lines.append(f"program: {days} station-days of big-endian SAC files at 100 Hz, second run (the first warms up)")
    lines.append(f"  wall {wall:.3f} s ({wall / days:.3f} s per station-day); headers {t1 - t0:.3f} s;"
                 f" first run {t2 - t1:.3f} s")
    for k in ("read", "upload", "device", "write"):
        lines.append(f"  {k:7s} {stats[k]:.3f} s ({100 * stats[k] / wall:.0f}%)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=float, default=60)
    ap.add_argument("--file-days", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_bench.txt"))
    a = ap.parse_args()
    lines = []
    device_run(a.days, lines)
    if a.file_days:
        file_run(a.file_days, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
