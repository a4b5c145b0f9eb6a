"""GPU: step 1 (hypotremormcmc_amd.convert) -- the batched FFT against numpy, htm_convert against the numpy restatement
(tests/convert_restatement.py) at edge shapes, the program end to end on synthetic SAC files, and the pipeline
convert -> correlate -> measure on synthetic tremor."""
import ctypes as C
import dataclasses
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hypotremormcmc_amd import _lib, convert, synth
from hypotremormcmc_amd.correlate import read_env
from hypotremormcmc_amd.select import read_detected_win
from tests import convert_restatement as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _fft(x, ld_in, ld_out, n, batch, direction, out=None, in_place=False):
    lib = _lib.load()
    xi = np.ascontiguousarray(x, dtype=np.complex128)
    if in_place:
        _lib.check(lib.htm_fft(0, xi.ctypes.data_as(_lib.dp), ld_in, xi.ctypes.data_as(_lib.dp), ld_in, n, batch,
                               direction))
        return xi
    _lib.check(lib.htm_fft(0, xi.ctypes.data_as(_lib.dp), ld_in, out.ctypes.data_as(_lib.dp), ld_out, n, batch,
                           direction))
    return out


@pytest.mark.parametrize("n", [4, 8, 12, 20, 28, 44, 4 * 1009, 1 << 16, 60000, 300000, 600000, 4 * 75011])
def test_fft_against_numpy(n):
    rng = np.random.default_rng(n)
    batch = 3
    x = rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))
    for direction in (-1, 1):
        ref = np.fft.fft(x, axis=1) if direction < 0 else np.fft.ifft(x, axis=1) * n
        got = _fft(x, n, n, n, batch, direction, out=np.zeros((batch, n), dtype=np.complex128))
        err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
        assert err <= 1e-12, (n, direction, err)
        inp = _fft(x, n, n, n, batch, direction, in_place=True)
        assert np.array_equal(inp.view(np.float64), got.view(np.float64)), (n, direction)
    # strided rows: the padding between rows is left alone
    ld_in, ld_out = n + 3, n + 5
    xs = np.full((batch, ld_in), 7.0 + 7j)
    xs[:, :n] = x
    out = np.full((batch, ld_out), -3.0 - 1j)
    got = _fft(xs, ld_in, ld_out, n, batch, -1, out=out)
    assert np.all(got[:, n:] == -3.0 - 1j)
    assert np.array_equal(got[:, :n].view(np.float64), _fft(x, n, n, n, batch, -1, in_place=True).view(np.float64))


def _htm_convert(x1, x2, c, fac, j0, j1):
    lib = _lib.load()
    N, n2 = x1.size, c.n // 2
    g0, g1 = j0 * n2, min(N, j1 * n2 + c.n)
    a = np.ascontiguousarray(x1[g0:g1], dtype=np.float32)
    b = np.ascontiguousarray(x2[g0:g1], dtype=np.float32)
    k0, cnt = convert.outputs(N, c.n, c.n_fac, j0, j1)
    out = np.full(cnt, np.nan)
    kb = (C.c_int * 4)(*c.k_band)
    fp = C.POINTER(C.c_float)
    _lib.check(lib.htm_convert(0, a.ctypes.data_as(fp), b.ctypes.data_as(fp), N, c.n, c.n_fac, c.h, kb, fac[0], fac[1],
                               j0, j1, out.ctypes.data_as(_lib.dp)))
    return k0, out


def _tremor(N, dt, seed):
    rng = np.random.default_rng(seed)
    fs = 1.0 / dt
    x1 = 50.0 * synth.band_noise(N, fs, rng, 1.0, min(12.0, 0.5 * fs)) + 3.0 + 1e-4 * np.arange(N)
    x2 = 20.0 * synth.band_noise(N, fs, rng, 0.5, min(9.0, 0.5 * fs)) - 1.0
    return x1.astype(np.float32), x2.astype(np.float32)


def _check_convert(c, N, seed, fac=(1.0, 0.7)):
    """whole record in one call and segment by segment, against the restatement: counts, positions and values"""
    x1, x2 = _tremor(N, c.dt, seed)
    ref = cr.convert(x1, x2, c.n, c.n_fac, c.h, c.k_band, fac)
    last = convert.last_segment(N, c.n)
    k0, got = _htm_convert(x1, x2, c, fac, 0, last)
    assert k0 == 0 and got.size == ref.size == math.ceil(N / c.n_fac)
    scale = np.max(np.abs(ref))
    err = np.max(np.abs(got - ref)) / scale if scale > 0 else np.max(np.abs(got))
    assert err <= 1e-11, err
    pieces = [_htm_convert(x1, x2, c, fac, j, j) for j in range(last + 1)]
    assert [p[0] for p in pieces] == [convert.outputs(N, c.n, c.n_fac, j, j)[0] for j in range(last + 1)]
    assert np.array_equal(np.concatenate([p[1] for p in pieces]), got)
    return err


@pytest.mark.parametrize("r", ["n", "n+n2-1", "n+3n2"])
def test_convert_shapes_100hz(r):
    c = convert.constants(float(np.float32(0.01)), 40.0)
    n2 = c.n // 2
    N = {"n": c.n, "n+n2-1": c.n + n2 - 1, "n+3n2": c.n + 3 * n2}[r]
    _check_convert(c, N, seed=len(r))


@pytest.mark.parametrize("h", [0, 1])
def test_convert_small_half_width(h):
    c = dataclasses.replace(convert.constants(float(np.float32(0.01)), 40.0), h=h)
    _check_convert(c, c.n + 2 * (c.n // 2) + 17, seed=10 + h)


def test_convert_10hz_band_above_nyquist():
    c = convert.constants(float(np.float32(0.1)), 400.0)
    assert c.k_band[2] > c.n // 2
    _check_convert(c, c.n + 5 * (c.n // 2) + 3, seed=3)


def test_convert_20hz():
    c = convert.constants(float(np.float32(0.05)), 3000.0)
    assert (c.h, c.k_band[3]) == (29, c.n // 2)
    _check_convert(c, c.n + c.n // 2 + 1234, seed=4)


def test_convert_100hz_flagship_and_closed_form():
    c = convert.constants(float(np.float32(0.01)), 3000.0)
    assert c.n == 300000
    _check_convert(c, c.n + 2 * (c.n // 2) + 777, seed=5)
    # a sinusoid with a whole number of cycles per segment in the flat band: A (2h / (2h+1))^2 inside every full segment
    n, n2, n4 = c.n, c.n // 2, c.n // 4
    cyc = (c.k_band[1] + c.k_band[2]) // 2
    N = 2 * n
    A = 3.5
    x1 = (A * np.cos(2 * math.pi * cyc * np.arange(N) / n)).astype(np.float32)
    _, got = _htm_convert(x1, np.zeros(N, dtype=np.float32), c, (1.0, 1.0), 0, convert.last_segment(N, n))
    g = np.arange(got.size) * c.n_fac
    inside = (g >= n4) & (g < 2 * n - n4)
    # the kernel reads float32 samples: A cos rounded to float32 carries white rounding noise of ~3e-8 A, so on the
    # device the closed form holds to that; the float64 restatement below holds it to 1e-9
    rel = np.max(np.abs(got[inside] - cr.closed_form(A, c.h))) / cr.closed_form(A, c.h)
    assert rel < 1e-7, rel
    ref = cr.convert(x1, np.zeros(N, dtype=np.float32), n, c.n_fac, c.h, c.k_band, (1.0, 1.0))
    assert np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref))
    x64 = A * np.cos(2 * math.pi * cyc * np.arange(n) / n)
    e = cr.process_segment(x64, np.zeros(n), c.h, c.k_band, (1.0, 1.0))
    assert np.max(np.abs(e[n4:n - n4] - cr.closed_form(A, c.h))) / cr.closed_form(A, c.h) < 1e-9


# ---- edge shapes: the k_cv_* kernels where an index can go wrong ---------------------------------------------------------
# References: the literal transcription of the reference's loops for n <= 40, the vectorised restatement above.  The
# tolerance is the project's 1e-11 of the largest reference value, the scale taken over each segment's kept range:
# an indexing error at these shapes is O(1).  A band without a pass band (expecting zeros) must give exact zeros.

def _noise(N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N).astype(np.float32), (rng.standard_normal(N) * 3 + 5.0).astype(np.float32)


def _check_record(c, x1, x2, fac, tag=""):
    """counts and positions; the whole record in one call, segment by segment, the middle run 1 .. last - 1 and the last
    segment alone, bit-equal where they overlap; every segment's kept range against the reference -> (values, worst
    error as a fraction of 1e-11 of the segment's scale)"""
    N = x1.size
    ref = (cr.convert_literal if c.n <= 40 else cr.convert)(x1, x2, c.n, c.n_fac, c.h, c.k_band, fac)
    assert np.all(np.isfinite(ref))
    last = convert.last_segment(N, c.n)
    k0, got = _htm_convert(x1, x2, c, fac, 0, last)
    assert k0 == 0 and got.size == ref.size == math.ceil(N / c.n_fac)
    pos = [convert.outputs(N, c.n, c.n_fac, j, j) for j in range(last + 1)]
    assert pos[0][0] == 0 and pos[-1][0] + pos[-1][1] == got.size
    worst = 0.0
    for j, (kj, cnt) in enumerate(pos):
        pk, piece = _htm_convert(x1, x2, c, fac, j, j)
        assert (pk, piece.size) == (kj, cnt), (tag, j)
        assert np.array_equal(piece, got[kj:kj + cnt]), (tag, j)
        if cnt == 0:
            continue
        r = ref[kj:kj + cnt]
        scale = np.max(np.abs(r))
        if scale == 0.0:
            assert np.all(piece == 0.0), (tag, j)
        else:
            err = np.max(np.abs(piece - r)) / scale
            worst = max(worst, err / 1e-11)
            assert err <= 1e-11, (tag, j, err)
    if last >= 2:
        km, mid = _htm_convert(x1, x2, c, fac, 1, last - 1)
        assert km == pos[1][0] and mid.size == pos[-1][0] - km
        assert np.array_equal(mid, got[km:km + mid.size]), tag
    kl, tail = _htm_convert(x1, x2, c, fac, last, last)
    assert np.array_equal(tail, got[kl:]), tag
    return got, worst


def _small_bands(n):
    return [(1, 2, max(2, n // 3), max(2, n // 2 - 1)), (0, 0, 0, 0), (2, 2, 2, 2), (1, 1, n // 2, n // 2),
            (0, 0, n // 2 + 1, n + 3)]


@pytest.mark.parametrize("n", [4, 8, 12, 16, 40])
def test_convert_small_grid_against_literal(n):
    """every h in {0, 1, n/4, n/2}, n_fac in {1, 3, n/2}, record length around the segment boundaries and band, the
    degenerate ones included: n below one scan round, 2h == n, n_fac == n/2"""
    n2 = n // 2
    worst, cases = 0.0, 0
    for h in sorted({0, 1, n // 4, n2}):
        for n_fac in sorted({1, 3, n2}):
            if n_fac > n2:
                continue
            for N in (n, n + 1, n + n2 - 1, n + n2, n + 3 * n2 + 1):
                for b, kb in enumerate(_small_bands(n)):
                    c = convert.Constants(1.0, n, n_fac, h, kb)
                    x1, x2 = _noise(N, 100000 * n + 1000 * h + 100 * n_fac + N)
                    got, w = _check_record(c, x1, x2, (1.3, 0.7), tag=(n, h, n_fac, N, kb))
                    if b in (1, 2):
                        assert np.all(got == 0.0), (n, h, n_fac, N, kb)
                    worst = max(worst, w)
                    cases += 1
    print("CONVERT small grid n=%d: %d cases, worst %.3g of 1e-11" % (n, cases, worst))


def _band(n):
    return (max(1, n // 50), n // 20, n // 5, n // 4)


# (n, h): one scan round of 256 and either side of it; a tile of 1024 exactly, 4 past it, two tiles and 4 (h within a
# tile and a halo that spans tiles); 2h == n beyond a tile; 2h == n at kCvMaxH; kCvMaxH with the halo clipped on one side
LARGER = [(252, 5), (252, 126), (256, 5), (256, 128), (260, 5), (260, 130), (1024, 5), (1024, 300), (1028, 5),
          (1028, 300), (2052, 5), (2052, 300), (4100, 2050), (8192, 4096), (12000, 4096)]


@pytest.mark.parametrize("n,h", LARGER)
def test_convert_scan_rounds_tiles_and_wide_windows(n, h):
    n2 = n // 2
    N = n + 2 * n2 + 17
    x1, x2 = _tremor(N, 0.01, seed=n + h)
    worst = 0.0
    for n_fac in (1, 7, n2):
        c = convert.Constants(0.01, n, n_fac, h, _band(n))
        worst = max(worst, _check_record(c, x1, x2, (1.0, 0.7), tag=(n, h, n_fac))[1])
    print("CONVERT n=%d h=%d: worst %.3g of 1e-11" % (n, h, worst))


def test_convert_dev_writes_only_its_outputs():
    """htm_convert_dev on device pointers and a non-default torch stream, into the middle of a buffer filled with a
    sentinel: the 8 doubles on either side keep it, the middle has the bits of the host form"""
    import torch

    lib = _lib.load()
    n, h, n_fac = 1028, 5, 7
    N = n + 3 * (n // 2) + 17
    c = convert.Constants(0.01, n, n_fac, h, _band(n))
    x1, x2 = _tremor(N, 0.01, seed=21)
    last = convert.last_segment(N, n)
    kb = (C.c_int * 4)(*c.k_band)
    stream = torch.cuda.Stream()
    for j0, j1 in ((0, last), (1, last - 1), (last, last)):
        _, want = _htm_convert(x1, x2, c, (1.0, 0.7), j0, j1)
        g0, g1 = j0 * (n // 2), min(N, j1 * (n // 2) + n)
        with torch.cuda.stream(stream):
            d1, d2 = torch.from_numpy(x1[g0:g1].copy()).cuda(), torch.from_numpy(x2[g0:g1].copy()).cuda()
            buf = torch.full((want.size + 16,), -12345.5, dtype=torch.float64, device="cuda")
            _lib.check(lib.htm_convert_dev(0, C.c_void_p(d1.data_ptr()), C.c_void_p(d2.data_ptr()), N, n, n_fac, h, kb,
                                           1.0, 0.7, j0, j1, C.c_void_p(buf.data_ptr() + 8 * 8),
                                           C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            v = buf.cpu().numpy()
        assert np.all(v[:8] == -12345.5) and np.all(v[-8:] == -12345.5), (j0, j1)
        assert np.array_equal(v[8:-8], want), (j0, j1)


DEGENERATE = [(40, 3, 3, (1, 2, 13, 19)), (1028, 5, 7, (10, 30, 200, 257))]


@pytest.mark.parametrize("n,h,n_fac,kb", DEGENERATE)
def test_convert_degenerate_records(n, h, n_fac, kb):
    """All zero: exact zeros.  A constant and a pure ramp are detrended away wherever a segment lies inside the record:
    |out| <= 1e-11 max |x| in the kept ranges of every segment but the last.  The last segment always reads zeros
    beyond N (N - j n/2 < n), so its window holds a step, not a line; there the restatement is the reference.  A
    signal of size 1 on an offset of 1e6: against the restatement at 1e-11 of the largest value."""
    c = convert.Constants(0.01, n, n_fac, h, kb)
    fac = (1.0, 0.7)
    N = n + 3 * (n // 2) + 5
    last = convert.last_segment(N, n)
    z = np.zeros(N, dtype=np.float32)
    got, _ = _check_record(c, z, z, fac, "zero")
    assert np.all(got == 0.0)
    i = np.arange(N, dtype=np.float64)
    k_last = convert.outputs(N, n, n_fac, last, last)[0]
    for name, f1, f2 in (("constant", np.full(N, 1e4), np.full(N, 1e4)), ("ramp", 3.0 * i - 7.0, 11.0 - 2.0 * i)):
        x1, x2 = f1.astype(np.float32), f2.astype(np.float32)
        assert np.array_equal(x1, f1) and np.array_equal(x2, f2), "the record is exact in float32"
        ref = cr.convert(x1, x2, n, n_fac, h, kb, fac)
        _, got = _htm_convert(x1, x2, c, fac, 0, last)
        top = float(np.max(np.abs(got[:k_last]))) / float(max(np.max(np.abs(x1)), np.max(np.abs(x2))))
        err = float(np.max(np.abs(got[k_last:] - ref[k_last:])) / np.max(np.abs(ref[k_last:])))
        print("CONVERT n=%d %s: %.3g of 1e-11 max|x|; last segment %.3g of 1e-11" % (n, name, top / 1e-11, err / 1e-11))
        assert top <= 1e-11, (name, top)
        assert err <= 1e-11, (name, err)
    x1, x2 = _noise(N, n)
    x1, x2 = (x1 + np.float32(1e6)).astype(np.float32), (x2 - np.float32(1e6)).astype(np.float32)
    ref = cr.convert(x1, x2, n, n_fac, h, kb, fac)
    _, got = _htm_convert(x1, x2, c, fac, 0, last)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print("CONVERT n=%d offset 1e6: %.3g of 1e-11" % (n, err / 1e-11))
    assert err <= 1e-11, err


@pytest.mark.parametrize("n,h,n_fac,kb", DEGENERATE)
def test_convert_nan_stays_in_its_segments(n, h, n_fac, kb):
    """one NaN in component 1 at stream sample q: NaN exactly in the kept ranges of the segments that contain q,
    the bits of the clean run everywhere else.  q = n/2 + 3 lies in segments 0 and 1, q = N - 1 in the last alone."""
    c = convert.Constants(0.01, n, n_fac, h, kb)
    fac = (1.0, 0.7)
    n2 = n // 2
    N = n + 3 * n2 + 5
    last = convert.last_segment(N, n)
    x1, x2 = _noise(N, 3 * n)
    _, clean = _htm_convert(x1, x2, c, fac, 0, last)
    assert np.all(np.isfinite(clean))
    for q in (n2 + 3, N - 1):
        y1 = x1.copy()
        y1[q] = np.nan
        _, got = _htm_convert(y1, x2, c, fac, 0, last)
        want_nan = np.zeros(got.size, dtype=bool)
        hit = [j for j in range(last + 1) if j * n2 <= q < j * n2 + n]
        assert hit == ([0, 1] if q == n2 + 3 else [last])
        for j in hit:
            kj, cnt = convert.outputs(N, n, n_fac, j, j)
            want_nan[kj:kj + cnt] = True
        assert np.array_equal(np.isnan(got), want_nan), q
        assert np.array_equal(got[~want_nan], clean[~want_nan]), q


def _run(args, cwd, env=None, timeout=300):
    e = dict(os.environ, PYTHONPATH=ROOT, **(env or {}))
    r = subprocess.run([sys.executable, "-m"] + args, cwd=cwd, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_program_end_to_end(tmp_path):
    fs = [20.0, 50.0, 20.0, 50.0]
    wf = synth.make_tremor_waveforms(fs, 1237.3, [300.0, 800.0], [0, 2, -1, 1], [0.0, 0.2, -0.1, 0.3], level=1.0,
                                     noise=0.5, seed=11)
    ids = ["2020.001", "2020.002", "2020.003"]
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        synth.write_waveforms(str(d), wf, ids, 100.0, big_endian=("W002",))
    _run(["hypotremormcmc_amd.convert", "tremor.in"], a)
    _run(["hypotremormcmc_amd.convert", "tremor.in"], b, env={"HTM_CONVERT_MB": "0.001"})
    for s, name in enumerate(wf.stations):
        raw_a = open(a / f"{name}.merged.env", "rb").read()
        assert raw_a == open(b / f"{name}.merged.env", "rb").read(), name
        t, v = read_env(str(a / f"{name}.merged.env"))
        c = convert.constants(float(np.float32(1.0 / fs[s])), 100.0)
        x1, x2 = wf.data[s]
        ref = cr.convert(x1, x2, c.n, c.n_fac, c.h, c.k_band, (1.0, 1.0))
        assert v.size == ref.size == math.ceil(x1.size / c.n_fac)
        assert np.array_equal(t, np.arange(v.size, dtype=np.float64) * (c.dt * c.n_fac))
        assert np.max(np.abs(v - ref)) <= 1e-11 * np.max(np.abs(ref)), name


def test_pipeline_convert_correlate_measure(tmp_path):
    delay = np.array([0, 3, -2, 1])
    la = np.array([0.0, 0.3, -0.2, 0.1])
    burst_win = [4, 9, 13]
    wf = synth.make_tremor_waveforms([20.0] * 4, 2000.0, [(w - 1) * 100.0 + 50.0 for w in burst_win], delay, la,
                                     width=6.0, level=0.0, noise=1.0, seed=7)
    synth.write_waveforms(str(tmp_path), wf, ["a", "b"], 200.0, big_endian=("W003",), alpha=0.998, n_pair_thred=3)
    _run(["hypotremormcmc_amd.convert", "tremor.in"], tmp_path)
    _run(["hypotremormcmc_amd.correlate", "tremor.in"], tmp_path)
    _run(["hypotremormcmc_amd.measure", "tremor.in"], tmp_path)
    ids, _ = read_detected_win(str(tmp_path / "detected_win.dat"))
    assert ids == burst_win
    for w in ids:
        rows = np.loadtxt(tmp_path / ("opt_data.%06d.dat" % w))
        assert np.all(np.abs(rows[:, 3] - (delay - delay.mean())) <= 1.0), (w, rows[:, 3])
        assert np.all(np.abs(rows[:, 5] - (la - la.mean())) <= 0.02), (w, rows[:, 5])
