"""Plain-numpy restatement of the convergence diagnostics: split R-hat and effective sample size after
Vehtari et al. 2021 / Stan, without rank normalisation.  It shares no code with the product.

Input: x [M*N][n_par], sequence m in rows m*N .. m*N + N - 1.  n = N // 2; sequence m gives two split sequences, its
first n and its last n draws (an odd N drops the middle draw): S = 2M sequences, tot = S n draws.  Per split sequence:
the mean mu_s and the biased autocovariance g_s[t] = (1/n) sum_i (x_i - mu_s)(x_{i+t} - mu_s), t = 0..L,
L = min(n - 1, max_lag); acov = mean over s of g_s.  The mean is taken twice, the second time of the residuals about the
first, so that it is the mean rounded once also for a column with a large offset (a plain sum of n values near 1e3
carries n u 1e3, which the centred products do not forgive)."""
import numpy as np


def split_sequences(x, n_seq):
    """[S][n][n_par]"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    N = x.shape[0] // n_seq
    assert N * n_seq == x.shape[0] and N >= 4
    n = N // 2
    seqs = []
    for m in range(n_seq):
        seqs.append(x[m * N:m * N + n])
        seqs.append(x[m * N + N - n:m * N + N])
    return np.stack(seqs)


def diagnose(x, n_seq, max_lag=1000):
    """out [n_par][4] = (rhat, ess, tau, lags), acov [(L+1)][n_par], min_abs_pair [n_par] = the smallest |P_k| among
    the pair sums the Geyer scan of the column looked at (inf for a constant column), lags_used [n_par] = the number
    of lags it looked at."""
    xs = split_sequences(x, n_seq)
    S, n, n_par = xs.shape
    L = min(n - 1, int(max_lag))
    tot = S * n
    mu = xs.mean(axis=1)
    mu = mu + (xs - mu[:, None, :]).mean(axis=1)
    xc = xs - mu[:, None, :]
    acov = np.empty((L + 1, n_par))
    for t in range(L + 1):
        g = (xc[:, :n - t] * xc[:, t:]).sum(axis=1) / n          # [S][n_par]
        acov[t] = g.mean(axis=0)
    out = np.full((n_par, 4), np.nan)
    min_abs = np.full(n_par, np.inf)
    lags_used = np.zeros(n_par, dtype=int)
    for p in range(n_par):
        W = acov[0, p] * n / (n - 1)
        if not W > 0:
            continue
        Bn = mu[:, p].var(ddof=1)
        vp = (n - 1) / n * W + Bn
        rho = 1 - (W - acov[:, p] * n / (n - 1)) / vp
        total, prev, lags, k = 0.0, np.inf, -1, 0
        while 2 * k + 1 <= L:
            P = rho[2 * k] + rho[2 * k + 1]
            min_abs[p] = min(min_abs[p], abs(P))
            lags_used[p] = 2 * k + 2
            if P < 0:
                lags = 2 * k
                break
            P = min(P, prev)
            total += P
            prev = P
            k += 1
        tau = max(-1 + 2 * total, 1 / np.log10(tot))
        out[p] = (np.sqrt(vp / W), tot / tau, tau, lags)
    return out, acov, min_abs, lags_used
