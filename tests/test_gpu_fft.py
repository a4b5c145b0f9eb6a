"""GPU: the batched FFT of step 1 (hypotremormcmc_amd/csrc/htm_fft.hpp, fft_run in csrc/htm_steps.hip) against exact
long-double references (tests/fft_restatement.py) at every path of the plan: n = 1 (the copy alone), a lone radix-2
pass, odd lengths (a radix 3, 5 or 7 pass first, without twiddles), mixed lengths, odd and even pass counts, Bluestein on
odd and even n and just above a power of two, one row, three rows and a thousand rows, both directions, in place and
out of place, rows with padding.

The bounds are derived, not fitted.  u = 2^-53; all of them are first order in u and relative in the row 2-norm,
|| got - ref ||_2 / || ref ||_2.

Stockham (the lengths 2^a 3^b 5^c 7^d).  A pass of radix R multiplies R - 1 inputs of each butterfly by a twiddle and
takes an R-point DFT in registers; the exact pass is unitary up to the factor sqrt R, so the relative errors of the
passes add.  Per pass c(R) u = (3 + a(R)) u:
  * 3: a twiddle rounded once from long double is off by at most u / sqrt 2 of its modulus, and a complex product
    formed from four products and two sums is within sqrt 5 u of the exact one; u / sqrt 2 + sqrt 5 u < 3 u.  (The first
    pass has no twiddles; it is charged all the same.)
  * a(2) = 1: one addition per output.
  * a(4) = 2: two levels of additions; the factor +-i is a swap and a sign, exact.
  * odd R: an output is v_0 plus R - 1 products with roots rounded to double, added in sequence: at most (R + 2) u
    sum_r |v_r| <= (R + 2) u sqrt R ||v||_2 per output, so (R + 2) u R ||v||_2 over the R outputs in the 2-norm,
    against ||F_R v||_2 = sqrt R ||v||_2: a(R) = (R + 2) sqrt R.
stockham_bound(n) = u sum over the passes of c(R): 4 u for n = 2, 11.7 u for 3, 26.8 u for 7, 29 u for 2048, 76.6 u for
3000, 118.9 u = 1.3e-14 for 300000.  Contraction into FMAs removes roundings and so only lowers the error.

Bluestein (every other length; m = the smallest power of two >= 2n - 1, w the chirp, B the transform of the wrapped
conjugate chirp divided by m, made once per plan by the same inner transform).  With a = x w padded to m, A = F_m a,
P = A B, c = the backward transform of P and X_k = w_k c_k, and s = stockham_bound(m):
  * a: 3 u ||a|| (a rounded chirp and a product), carried to c unchanged in relative terms;
  * A: s ||A||.  These two reach c multiplied by at most max |B| sqrt m ||A|| = kappa_b ||X||, where
    kappa_b = m max_k |B_k| / sqrt n bounds ||c||_2 / ||X||_2: the convolution of length m carries error in the m - n
    entries the output discards.  Together kappa_b (3 u + s);
  * the product: 3 u, again times kappa_b;
  * the table: ||dB|| <= (s + u) ||B|| with ||B||_2 = sqrt((2n - 1) / m); it meets A entry by entry, so it reaches c
    as at most sqrt m max |A| ||dB|| = rho sqrt((2n - 1) / n) (s + u) ||X|| <= sqrt 2 rho (s + u) ||X||, with
    rho = max |A| / rms(A) of the exact inner transform of the row (fft_restatement.peak_ratio);
  * the backward transform: s ||c|| <= s kappa_b ||X||;   * the last product: 3 u ||X||.
bluestein_bound(n, rho) = kappa_b (2 s + 6 u) + sqrt 2 rho (s + u) + 3 u.  Where sqrt 2 rho = kappa_b this is
kappa_b (3 s + 7 u) + 3 u: three equal transforms.  kappa_b is 2.08 .. 2.29 at the lengths below (computed in long double from
the exact chirp); rho is 1 for an impulse (|A_k| = 1 for every k), the same in both directions for a tone, and 1.7 .. 3.2
for the random rows.  kappa_b and rho come from dft_exact up to m = 4096 and from np.fft in double above (n = 4 * 75011,
m = 2^20): its relative error of ~1e-16 in a ratio of norms is immaterial, and tests/test_convert.py pins np.fft to
dft_exact.  The bounds used lie between 0 (n = 1) and 3.1e-14 (n = 2018, 4 * 75011), all far below the 1e-12 of
test_gpu_convert.py::test_fft_against_numpy.

Structured inputs are checked bin by bin with tol = bound(n) sqrt n, the largest a single bin can be off while the row
stays within the bound: the spectrum of a unit impulse at j is exp(sign 2 pi i j k / n), every twiddle on its own; the
input exp(-sign 2 pi i k0 j / n) (rounded once to double: up to n u / sqrt 2 in a bin, inside n tol since tol >= 4 sqrt 2 u)
gives the line n at k0 and 0 elsewhere, within n tol; backward(forward(x)) = n x within the sum of the two bounds.

A double-precision numpy model of the same pass order, tables and in-register DFTs stays at 0.02 .. 0.11 of
stockham_bound and 0.11 .. 0.15 of one stockham_bound(m) for Bluestein, so a correct kernel has a factor >= 9 of room; a
result above a bound is a finding.  Observed maxima on an MI355X as fractions of the bounds: DESIGN.md §3.5."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from hypotremormcmc_amd import _lib
from tests import fft_restatement as fr

pytestmark = pytest.mark.gpu

STOCKHAM = [1, 2, 3, 5, 6, 7, 9, 10, 14, 15, 16, 21, 25, 27, 30, 35, 49, 64, 105, 125, 210, 243, 343, 1024, 2048, 2401,
            3000]
BLUESTEIN = [11, 13, 22, 23, 26, 33, 97, 129, 1009, 2018]
LONG = [300000, 4 * 75011]          # O(n) references only
LONGEST = 1 << 22                   # the library accepts up to 2^24; there this test took 16.7 s (host copies and
                                    # comparisons of 256 MB rows), so it runs at 2^22 (11 radix-4 passes)

PAD_IN, PAD_OUT = 7.0 + 7j, -3.0 - 1j


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _padded(x, ld, fill):
    p = np.full((x.shape[0], ld), fill, dtype=np.complex128)
    p[:, :x.shape[1]] = x
    return p


def _fft_both_ways(x, direction):
    """rows of x transformed out of place (ld_in = n + 3, ld_out = n + 5) and in place (ld = n + 3): the same bits, the
    input and every padding left alone -> the out-of-place result"""
    lib = _lib.load()
    batch, n = x.shape
    xs, out = _padded(x, n + 3, PAD_IN), np.full((batch, n + 5), PAD_OUT, dtype=np.complex128)
    keep = xs.copy()
    _lib.check(lib.htm_fft(0, xs.ctypes.data_as(_lib.dp), n + 3, out.ctypes.data_as(_lib.dp), n + 5, n, batch, direction))
    assert np.array_equal(_bits(xs), _bits(keep)), "out of place: the input changed"
    assert np.all(out[:, n:] == PAD_OUT), "out of place: padding of the output written"
    _lib.check(lib.htm_fft(0, xs.ctypes.data_as(_lib.dp), n + 3, xs.ctypes.data_as(_lib.dp), n + 3, n, batch, direction))
    assert np.all(xs[:, n:] == PAD_IN), "in place: padding written"
    assert np.array_equal(_bits(xs[:, :n]), _bits(out[:, :n])), "in place and out of place differ"
    return out[:, :n].copy()


def _rel(got, ref):
    """per row || got - ref ||_2 / || ref ||_2, the difference taken in long double"""
    d = np.abs(got.astype(np.clongdouble) - ref)
    return (np.sqrt(np.sum(d * d, axis=1)) / np.sqrt(np.sum(np.abs(ref) ** 2, axis=1))).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(n):
    """three random rows of length n, their exact transforms in both directions and, for a Bluestein length, the peak
    ratios of the rows (forward, backward) and of the exact forward spectrum taken backward; made once, read-only"""
    rng = np.random.default_rng(7000 + n)
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    x.setflags(write=False)
    ref = {d: fr.dft_exact(x, d) for d in (-1, 1)}
    rho = None
    if fr.passes(n) is None:
        rho = {-1: fr.peak_ratio(x, -1), 1: fr.peak_ratio(x, 1), "back": fr.peak_ratio(ref[-1], 1)}
    for a in ref.values():
        a.setflags(write=False)
    return x, ref, rho


def _bounds(n, rho_rows, rows):
    """the bound of each of `rows` rows; rho_rows: their peak ratios, read for a Bluestein length only"""
    if fr.passes(n) is not None:
        return np.full(rows, fr.stockham_bound(n))
    assert len(rho_rows) == rows
    return np.array([fr.bluestein_bound(n, r) for r in rho_rows])


def _assert_rows(tag, n, got, ref, bounds):
    err = _rel(got, ref)
    frac = float(np.max(err / bounds)) if np.all(bounds > 0) else (0.0 if np.all(err == 0) else math.inf)
    print("FFT %s n=%d rows=%d: %.3f of the bound %.3g (max err %.3g)" % (tag, n, got.shape[0], frac, float(np.max(bounds)), float(np.max(err))))
    assert np.all(bounds < 1e-12)
    assert np.all(err <= bounds), (tag, n, err, bounds)
    return frac


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", STOCKHAM + BLUESTEIN)
def test_lengths_against_exact_dft(n, batch):
    x, ref, rho = _case(n)
    for d in (-1, 1):
        got = _fft_both_ways(x[:batch], d)
        _assert_rows("random dir=%+d" % d, n, got, ref[d][:batch], _bounds(n, None if rho is None else rho[d][:batch], batch))


@pytest.mark.parametrize("n", [12, 11])
def test_a_thousand_rows(n):
    """the row index runs far past one workgroup's rows (256 butterflies: 85 rows of n = 12; Bluestein m = 32)"""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((1000, n)) + 1j * rng.standard_normal((1000, n))
    for d in (-1, 1):
        got = _fft_both_ways(x, d)
        rho = None if fr.passes(n) is not None else fr.peak_ratio(x, d)
        _assert_rows("1000 rows dir=%+d" % d, n, got, fr.dft_exact(x, d), _bounds(n, rho, 1000))


def _structured(n):
    """the impulse positions, the tone bins and the peak ratio of each kind of row"""
    js = sorted({0, 1 % n, n - 1})
    ks = sorted({0, 1 % n, n - 1} | ({n // 2} if n % 2 == 0 else set()))
    return js, ks


def _check_structured(n, d, js, ks, got, bounds_imp, bounds_tone, what):
    """rows of got: the transforms of the impulses at js, then of the tones at ks"""
    root_n = math.sqrt(n)
    worst = 0.0
    for r, j in enumerate(js):
        tol = bounds_imp * root_n
        e = float(np.max(np.abs(got[r].astype(np.clongdouble) - fr.impulse_spectrum(n, j, d))))
        worst = max(worst, e / tol if tol > 0 else (0.0 if e == 0 else math.inf))
        assert e <= tol, ("impulse", n, d, j, e, tol)
    for r, k0 in enumerate(ks):
        tol = n * bounds_tone[r] * root_n
        ref = np.zeros(n, dtype=np.complex128)
        ref[k0] = n
        e = float(np.max(np.abs(got[len(js) + r] - ref)))
        worst = max(worst, e / tol if tol > 0 else (0.0 if e == 0 else math.inf))
        assert e <= tol, ("tone", n, d, k0, e, tol)
    print("FFT structured %s n=%d dir=%+d: %.3f of tol" % (what, n, d, worst))


@pytest.mark.parametrize("n", STOCKHAM + BLUESTEIN + LONG)
def test_impulses_tones_and_round_trip(n):
    js, ks = _structured(n)
    blue = fr.passes(n) is None
    # a tone's inner row x w is the same in both directions (conj of the backward input is the forward input)
    rho_tone = fr.peak_ratio(np.array([fr.tone(n, k0, -1) for k0 in ks]), -1) if blue else None
    b_imp = fr.bound(n, 1.0)
    b_tone = _bounds(n, rho_tone, len(ks))
    assert b_imp < 1e-12 and np.all(b_tone < 1e-12)
    for d in (-1, 1):
        rows = np.zeros((len(js) + len(ks), n), dtype=np.complex128)
        for r, j in enumerate(js):
            rows[r, j] = 1.0
        for r, k0 in enumerate(ks):
            rows[len(js) + r] = fr.tone(n, k0, d).astype(np.complex128)
        got = _fft_both_ways(rows, d)
        _check_structured(n, d, js, ks, got, b_imp, b_tone, "batch")
    # backward(forward(x)) = n x
    if n in LONG:
        rng = np.random.default_rng(n)
        x = rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))
        rf = rb = None
    else:
        x, ref, rho = _case(n)
        rf, rb = (rho[-1], rho["back"]) if blue else (None, None)
    fwd = _fft_both_ways(x, -1)
    back = _fft_both_ways(fwd, 1)
    if blue and rf is None:
        rf, rb = fr.peak_ratio(x, -1), fr.peak_ratio(fwd, 1)
    bsum = _bounds(n, rf, x.shape[0]) + _bounds(n, rb, x.shape[0])
    _assert_rows("round trip", n, back, n * x.astype(np.clongdouble), bsum)


def test_longest_length_impulses_and_tones():
    """n = 2^22, one row, through htm_fft_dev on torch's current stream (in place and out of place): impulses at 0, 1 and
    n - 1 and tones at 0, 1, n/2 and n - 1, both directions.  The references are the long-double roots rounded once to
    double (u / sqrt 2 per entry, added to the tolerance)."""
    import torch

    n = LONGEST
    lib = _lib.load()
    c, s = fr.roots(n)
    try:
        w = np.empty(n, dtype=np.complex128)          # exp(-2 pi i q / n)
        w.real, w.imag = c, -s
    finally:
        fr.roots.cache_clear()
    del c, s
    ones = np.ones(n, dtype=np.complex128)
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.complex128)
    bound = fr.stockham_bound(n)
    assert bound < 1e-12
    tol = bound * math.sqrt(n) + fr.U
    stream = torch.cuda.current_stream()

    def run(x, d, in_place=False):
        t = torch.from_numpy(x).cuda()
        o = t if in_place else torch.empty_like(t)
        _lib.check(lib.htm_fft_dev(0, C.c_void_p(t.data_ptr()), n, C.c_void_p(o.data_ptr()), n, n, 1, d,
                                   C.c_void_p(stream.cuda_stream)))
        return o.cpu().numpy()

    worst = 0.0
    for d in (-1, 1):
        wd = w if d < 0 else np.conj(w)               # exp(d 2 pi i q / n)
        for j, ref in ((0, ones), (1, wd), (n - 1, np.conj(wd))):
            x = np.zeros(n, dtype=np.complex128)
            x[j] = 1.0
            e = float(np.max(np.abs(run(x, d) - ref)))
            worst = max(worst, e / tol)
            assert e <= tol, ("impulse", d, j, e, tol)
        for k0, x in ((0, ones), (1, np.conj(wd)), (n // 2, alt), (n - 1, wd)):
            got = run(x, d)
            line = got[k0]
            got[k0] = 0.0
            e = max(float(np.max(np.abs(got))), abs(line - n))
            worst = max(worst, e / (n * tol))
            assert e <= n * tol, ("tone", d, k0, e, n * tol)
    a, b = run(w, -1), run(w, -1, in_place=True)
    assert np.array_equal(_bits(a), _bits(b)), "in place and out of place differ"
    print("FFT structured n=%d: %.3g of tol" % (n, worst))
