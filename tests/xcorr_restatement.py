"""A numpy restatement of steps 2 and 3 of the reference pipeline, line by line, for the tests of
hypotremormcmc_amd.correlate / .measure.  np.fft.rfft / irfft mirror FFTW's r2c / c2r (irfft's 1/n is the reference's
`/ n` of src/cls_correlator.f90:234-235; where the reference does not divide, the product is multiplied back by n),
and `maxloc` takes the first maximum as Fortran's does."""
from __future__ import annotations

import math

import numpy as np


def taper(x):
    """src/mod_signal_process.f90:10-26"""
    n = x.size
    nleng = int(n * 0.05)
    out = np.array(x, dtype=np.float64)
    for i in range(1, nleng + 1):
        fac = 0.5 * (1.0 - math.cos((i - 1) * math.pi / nleng))
        out[i - 1] = x[i - 1] * fac
        out[n - i] = x[n - i] * fac
    return out


def prep_correlate(x):
    """src/cls_correlator.f90:207-212 (zero energy -> zeros: this build's rule)"""
    x = taper(np.asarray(x, dtype=np.float64))
    x = x - np.sum(x) / x.size
    l = math.sqrt(np.sum(x ** 2))
    return x / l if l != 0.0 else np.zeros_like(x)


def circ_fft(ri, rj):
    """natural-order circular correlation sum_m ri[m] rj[m+k], as c2r(conj(r2c(ri)) r2c(rj)) / n"""
    n = ri.size
    return np.fft.irfft(np.conj(np.fft.rfft(ri)) * np.fft.rfft(rj), n)


def circ_direct(ri, rj):
    n = ri.size
    return np.array([sum(ri[m] * rj[(m + k) % n] for m in range(n)) for k in range(n)])


def circ_exact(ri, rj):
    """the same circular correlation summed in long double (each lag exact to a few units of 2^-64 relative to
    sum |ri rj|), rounded once to float64"""
    n = ri.size
    a, b = np.asarray(ri, dtype=np.longdouble), np.asarray(rj, dtype=np.longdouble)
    out = np.empty(n, dtype=np.longdouble)
    step = max(1, (1 << 21) // n)
    m = np.arange(n)
    for k0 in range(0, n, step):
        k = np.arange(k0, min(n, k0 + step))
        out[k] = np.sum(a[None, :] * b[(m[None, :] + k[:, None]) % n], axis=1)
    return out.astype(np.float64)


def reference_order(c):
    """cc(1:n/2) = r2(n/2+1:n), cc(n/2+1:n) = r2(1:n/2) (src/cls_correlator.f90:234-235): lag j - n/2 at j"""
    n = c.size
    return np.concatenate([c[n // 2:], c[:n // 2]])


def correlate(amps, n, n_step, n_win):
    """-> cc (n_win, n_pair, n) in the reference's lag order, cc_max (n_win, n_pair); pairs in station-file order"""
    n_sta = amps.shape[0]
    prs = [(i, j) for i in range(n_sta - 1) for j in range(i + 1, n_sta)]
    cc = np.empty((n_win, len(prs), n))
    for w in range(n_win):
        r = [prep_correlate(amps[s, w * n_step:w * n_step + n]) for s in range(n_sta)]
        for p, (i, j) in enumerate(prs):
            cc[w, p] = reference_order(circ_fft(r[i], r[j]))
    return cc, cc.max(axis=2)


def threshold(values, alpha):
    """src/cls_measurer.f90:237-238: sort, take element int(n*n_win*alpha) (1-based)"""
    v = np.sort(np.asarray(values).ravel())
    return v[int(v.size * alpha) - 1]


def optimize_cc(x, dt, circ=None):
    """src/cls_measurer.f90:463-523 for one window x (n_sta, n); -> t, t_stdv, lag matrix, and the relative gap of
    each pair's two largest correlation values (near-ties can pick another lag under other rounding).  circ: the
    natural-order circular correlation (default the FFT form, c2r(conj(r2c(ri)) r2c(rj)) / n, times n)"""
    n_sta, n = x.shape
    r = []
    for i in range(n_sta):
        l = np.sum(x[i] ** 2)
        r.append(taper(x[i]) / l if l != 0.0 else np.zeros(n))     # zero energy -> lag 0: this build's rule
    lag = np.zeros((n_sta, n_sta))
    gap = np.full((n_sta, n_sta), np.inf)
    for i in range(n_sta - 1):
        for j in range(i + 1, n_sta):
            c = circ_fft(r[i], r[j]) * n if circ is None else circ(r[i], r[j])
            il = int(np.argmax(c)) + 1                               # maxloc: first maximum, 1-based
            lag[i, j] = (il - 1) * dt if il <= n // 2 else (il - n - 1) * dt
            lag[j, i] = -lag[i, j]
            top = np.sort(c)[-2:]
            if np.any(c):           # all zeros (a zero-energy station): index 0 under any rounding, no near-tie
                gap[i, j] = abs(top[1] - top[0]) / max(abs(top[1]), 1e-300)
    t = [0.0] * n_sta
    for i in range(n_sta):
        for j in range(n_sta):
            t[i] = t[i] - lag[i, j]
        t[i] = t[i] / n_sta
    ts = [0.0] * n_sta
    for i in range(n_sta):
        for j in range(n_sta):
            if i == j:
                continue
            ts[i] = ts[i] + (t[j] - t[i] - lag[i, j]) ** 2
    ts = [math.sqrt(v / (n_sta - 2)) for v in ts]
    return np.array(t), np.array(ts), lag, gap


def nint(v):
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def optimize_amp(x, t, dt):
    """src/cls_measurer.f90:405-459"""
    n_sta, n = x.shape
    x2 = np.zeros((n_sta, n))
    for i in range(n_sta):
        it = nint(t[i] / dt)
        for j in range(n):
            if 0 <= j + it < n:
                x2[i, j] = x[i, j + it]
    sxx = np.sum(x2 ** 2, axis=1)
    rel = np.zeros((n_sta, n_sta))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n_sta - 1):
            for j in range(i + 1, n_sta):
                sxy = np.sum(x2[i] * x2[j])
                if sxy < 0.0:
                    return np.zeros(n_sta), np.zeros(n_sta)
                rel[i, j] = float(np.log(np.float64(sxy) / sxx[i]))
                rel[j, i] = -rel[i, j]
    amp = [0.0] * n_sta
    for i in range(n_sta):
        for j in range(n_sta):
            amp[i] = amp[i] - rel[i, j]
        amp[i] = amp[i] / n_sta
    sd = [0.0] * n_sta
    with np.errstate(invalid="ignore"):
        for i in range(n_sta):
            for j in range(n_sta):
                if i == j:
                    continue
                sd[i] = sd[i] + (amp[j] - amp[i] - rel[i, j]) ** 2
    return np.array(amp), np.sqrt(np.array(sd) / (n_sta - 2))


def measure(x, dt, circ=None):
    """one window: t, t_stdv, amp, amp_stdv, lag matrix, top-two gaps"""
    t, ts, lag, gap = optimize_cc(x, dt, circ)
    a, asd = optimize_amp(x, t, dt)
    return t, ts, a, asd, lag, gap
