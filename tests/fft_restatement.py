"""Exact references and error bounds for the tests of the batched FFT (hypotremormcmc_amd/csrc/htm_fft.hpp):
    X[k] = sum_j x[j] exp(sign 2 pi i j k / n),   sign = -1 forward, +1 backward, unnormalised in both directions.

Everything here is np.longdouble (64-bit significand on x86, unit roundoff 2^-64 = 5.4e-20, 2000 times finer than the
u = 2^-53 the bounds are stated in).  The roots exp(2 pi i q / n) come from one table per n indexed by (j k) mod n in
integers, so the argument of cos and sin never exceeds pi / 4 (n a multiple of 8) or pi; pi is a long-double literal.
The derivation of the bounds is in the docstring of tests/test_gpu_fft.py."""
from __future__ import annotations

import functools
import math

import numpy as np

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288419716939937510")
U = 2.0 ** -53
CHUNK = 1 << 21            # entries of the DFT matrix held at once (40 bytes each with the index: ~85 MB)


@functools.lru_cache(maxsize=4)
def roots(n):
    """(cos, sin) of 2 pi q / n, q = 0 .. n-1, long double, read-only.  q above n/2 mirrors n - q; where 8 divides n
    only the first octant is evaluated, so the axes and diagonals are exact."""
    c, s = np.empty(n, dtype=LD), np.empty(n, dtype=LD)
    if n % 8 == 0:
        e = n // 8
        a = 2 * PI * np.arange(e + 1).astype(LD) / LD(n)
        c[:e + 1], s[:e + 1] = np.cos(a), np.sin(a)
        c[0], s[0] = 1, 0
        c[e] = s[e] = np.sqrt(LD(0.5))
        q = np.arange(e + 1, 2 * e + 1)                      # pi/2 - theta
        c[q], s[q] = s[2 * e - q], c[2 * e - q]
        q = np.arange(2 * e + 1, 4 * e + 1)                  # pi - theta
        c[q], s[q] = -c[4 * e - q], s[4 * e - q]
    else:
        a = 2 * PI * np.arange(n // 2 + 1).astype(LD) / LD(n)
        c[:n // 2 + 1], s[:n // 2 + 1] = np.cos(a), np.sin(a)
        c[0], s[0] = 1, 0
        if n % 2 == 0:
            c[n // 2], s[n // 2] = -1, 0
    q = np.arange(n // 2 + 1, n)
    c[q], s[q] = c[n - q], -s[n - q]
    c.setflags(write=False)
    s.setflags(write=False)
    return c, s


def _split(x):
    x = np.asarray(x)
    return np.real(x).astype(LD), np.imag(x).astype(LD)


def dft_exact(x, sign):
    """direct O(n^2) DFT of the rows of x (complex, double or long double) -> np.clongdouble of the same shape.  The
    matrix is built a block of output bins at a time (CHUNK entries), over the columns where x is not zero."""
    x = np.asarray(x)
    one = x.ndim == 1
    xr, xi = _split(np.atleast_2d(x))
    n = xr.shape[1]
    c, s = roots(n)
    nz = np.flatnonzero(np.any((xr != 0) | (xi != 0), axis=0))
    out = np.zeros(xr.shape, dtype=np.clongdouble)
    if nz.size:
        ar, ai = np.ascontiguousarray(xr[:, nz].T), np.ascontiguousarray(xi[:, nz].T)
        step = max(1, CHUNK // nz.size)
        for k0 in range(0, n, step):
            k = np.arange(k0, min(n, k0 + step), dtype=np.int64)
            q = (k[:, None] * nz[None, :].astype(np.int64)) % n
            tr, ti = c[q], s[q]
            if sign < 0:
                ti = -ti
            out[:, k0:k0 + k.size] = ((tr @ ar - ti @ ai) + 1j * (tr @ ai + ti @ ar)).T
    return out[0] if one else out


def impulse_spectrum(n, j, sign, k0=0, k1=None):
    """bins [k0, k1) of the transform of the unit impulse at j: exp(sign 2 pi i j k / n), np.clongdouble"""
    k1 = n if k1 is None else k1
    c, s = roots(n)
    q = (np.arange(k0, k1, dtype=np.int64) * int(j)) % n
    return c[q] + 1j * (s[q] if sign > 0 else -s[q])


def tone(n, k0, sign, j0=0, j1=None):
    """samples [j0, j1) of the input whose transform of direction `sign` is the single line n at bin k0:
    x[j] = exp(-sign 2 pi i k0 j / n), np.clongdouble (the caller rounds it to double once)"""
    return impulse_spectrum(n, k0, -sign, j0, j1)


def passes(n):
    """the library's pass list: radix 4 while it divides, then one 2, then 3s, 5s, 7s; None where another prime is
    left (Bluestein)"""
    r = []
    while n % 4 == 0:
        r.append(4)
        n //= 4
    if n % 2 == 0:
        r.append(2)
        n //= 2
    for p in (3, 5, 7):
        while n % p == 0:
            r.append(p)
            n //= p
    return r if n == 1 else None


def inner_length(n):
    """Bluestein's inner length: the smallest power of two >= 2n - 1"""
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return m


def pass_cost(R):
    """c(R) of the module docstring of tests/test_gpu_fft.py, in units of u"""
    a = {2: 1.0, 4: 2.0}.get(R)
    if a is None:
        a = (R + 2) * math.sqrt(R)
    return 3.0 + a


def stockham_bound(n):
    """relative 2-norm error of one Stockham transform of length n, first order in u"""
    p = passes(n)
    if p is None:
        raise ValueError("n = %d is a Bluestein length" % n)
    return U * sum(pass_cost(R) for R in p)


def chirp(n):
    """w[j] = exp(-pi i (j^2 mod 2n) / n), j < n, as (cos, sin) long double"""
    c, s = roots(2 * n)
    q = np.array([(j * j) % (2 * n) for j in range(n)], dtype=np.int64)
    return c[q], -s[q]


def _transform_m(a):
    """forward transform of rows of length m (a power of two): exact up to m = 4096, np.fft in double above (its
    relative error, ~1e-16, does not matter for a ratio of norms; tests/test_convert.py pins np.fft to dft_exact)"""
    m = a.shape[-1]
    if m <= 4096:
        return dft_exact(a, -1)
    return np.fft.fft(np.asarray(a, dtype=np.complex128), axis=-1)


@functools.lru_cache(maxsize=None)
def kappa(n):
    """kappa_b = m max_k |B_k| / sqrt(n), B = the forward transform of the wrapped conjugate chirp divided by m"""
    m = inner_length(n)
    wc, ws = chirp(n)
    b = np.zeros(m, dtype=np.clongdouble)
    b[:n] = wc - 1j * ws
    b[m - n + 1:] = b[1:n][::-1]
    return float(np.max(np.abs(_transform_m(b[None, :]))) / math.sqrt(n))


def peak_ratio(x, sign):
    """per row of x: max |A| / rms(A) of the inner forward transform A of a = x w (conj(x) w for sign = +1) padded
    to m, as Bluestein forms it"""
    x = np.atleast_2d(np.asarray(x))
    n = x.shape[1]
    m = inner_length(n)
    wc, ws = chirp(n)
    a = np.zeros((x.shape[0], m), dtype=np.clongdouble)
    a[:, :n] = (np.conj(x) if sign > 0 else x).astype(np.clongdouble) * (wc + 1j * ws)
    A = np.abs(_transform_m(a)).astype(np.float64)
    return np.max(A, axis=1) / np.sqrt(np.mean(A * A, axis=1))


def bluestein_bound(n, rho=None):
    """relative 2-norm error of one Bluestein transform of length n, first order in u; rho = peak_ratio of the row
    (None: sqrt(2) rho = kappa_b, three equal transforms: kappa_b (3 stockham_bound(m) + 7 u) + 3 u)"""
    sb = stockham_bound(inner_length(n))
    kb = kappa(n)
    if rho is None:
        rho = kb / math.sqrt(2.0)
    return kb * (2 * sb + 6 * U) + math.sqrt(2.0) * rho * (sb + U) + 3 * U


def bound(n, rho=None):
    return stockham_bound(n) if passes(n) is not None else bluestein_bound(n, rho)
