"""Throughput of steps 2 and 3 on the GPU: the correlogram kernel (k_xcorr through htm_xcorr_dev) at 60 stations,
n = 300, n_step = 150 and 4,000 windows; htm_measure_windows on 500 windows; and the drop-in programs,
`measure --from-envelopes` against `correlate` + `measure`, on a smaller set whose .corr files fit a scratch disk."""
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from hypotremormcmc_amd import correlate as corr, measure, synth

ROOT = os.path.abspath(".")
S, n, n_step, n_win = 60, 300, 150, 4000
rng = np.random.default_rng(0)
amps = 1.0 + rng.random((S, n_win * n_step + n))
env = corr.Envelopes(amps)
n_pairs = S * (S - 1) // 2
b = corr.batch_pairs(n_win, n, mb=2048)
bufs = env.correlate(n, n_step, n_win, 0, b)
for rep in range(2):                       # the first pass warms up
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for p0 in range(0, n_pairs, b):
        nb = min(b, n_pairs - p0)
        env.correlate(n, n_step, n_win, p0, nb, bufs[0][:, :nb] if nb == b else None, bufs[1][:, :nb] if nb == b else None)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
pw = n_pairs * n_win
print(f"k_xcorr: {S} stations ({n_pairs} pairs) x {n_win} windows, n {n}, batches of {b} pairs: {1e3 * dt:.1f} ms, "
      f"{pw / dt / 1e6:.2f} M pair-windows/s, {pw * n * n / dt / 1e12:.2f} T fp64 FMA/s", flush=True)

x = 1.0 + rng.random((500, S, n))
measure.measure_windows(x[:8], 1.0)
t0 = time.perf_counter(); measure.measure_windows(x, 1.0); dt = time.perf_counter() - t0
print(f"htm_measure_windows: 500 windows x {S} stations, n {n}: {1e3 * dt:.1f} ms (host to host)", flush=True)

S2, W2 = 16, 500
e = synth.make_tremor_envelopes(S2, W2, n, n_step, [50, 200, 400], rng.integers(-5, 6, S2), 0.3 * rng.standard_normal(S2),
                                noise=0.5, seed=1)
with tempfile.TemporaryDirectory() as d:
    synth.write_envelopes(d, e, t_win_corr=float(n), t_step_corr=float(n_step), alpha=0.999, n_pair_thred=60)
    pe = dict(os.environ, PYTHONPATH=ROOT)

    def run(*args):
        t0 = time.perf_counter()
        subprocess.run([sys.executable, "-m"] + list(args), cwd=d, env=pe, check=True, capture_output=True, timeout=900)
        return time.perf_counter() - t0

    t_c = run("hypotremormcmc_amd.correlate", "tremor.in")
    t_m = run("hypotremormcmc_amd.measure", "tremor.in")
    ref = open(os.path.join(d, "detected_win.dat")).read()
    t_e = run("hypotremormcmc_amd.measure", "tremor.in", "--from-envelopes")
    same = open(os.path.join(d, "detected_win.dat")).read() == ref
    corr_mb = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".corr")) / 2 ** 20
print(f"programs at {S2} stations x {W2} windows, n {n}: correlate {t_c:.2f} s + measure {t_m:.2f} s "
      f"({corr_mb:.0f} MiB of .corr) vs measure --from-envelopes {t_e:.2f} s (process start and torch import "
      f"included); same detected_win.dat: {same}", flush=True)
