// htm_diag.hpp -- convergence diagnostics of recorded samples: split R-hat and effective sample size per parameter
// (Vehtari et al. 2021 / Stan, without rank normalisation -- with it: htm_rank.hpp, which runs these kernels on the normal
// scores; definitions: DESIGN.md §3.6).
//
// Layout: samples are [M*N][ld] row-major, sequence m in rows m*N .. m*N + N - 1, parameter p in column p.  As in
// k_select, lane <-> column, so every load is a coalesced 512-B row segment.  A sequence gives two split sequences
// of n = N/2 draws (its first n and its last n rows), S = 2M in all.
//
//   k_diag_mean    mean of every (split sequence, column): a sum, then the mean of the residuals added to it
//   k_diag_acov    sum_i (x_i - mu)(x_{i+t} - mu) for a block of KB consecutive lags per thread, register-blocked:
//                  KB accumulators and a window of the KB values x[i+t0 .. i+t0+KB-1] that slides one row per step, so
//                  a step is two loads and KB fma.  A workgroup's waves take neighbouring lag blocks of one column group
//                  (they stream the same rows); the split sequences are cut into slabs, and a thread adds its slab's
//                  sequences in ascending order into the same accumulators.
//   k_diag_finish  one lane per column: adds the slabs in ascending order, then R-hat, rho and the Geyer scan
//
// No atomics: every sum has one fixed order, so two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace htm {

constexpr int kDiagRG = 4;        // row groups (waves) per workgroup of k_diag_mean
constexpr int kDiagLW = 4;        // lag blocks (waves) per workgroup of k_diag_acov

// first row of split sequence s: even s = the first n rows of sequence s/2, odd s = its last n rows
__device__ __forceinline__ long diag_row0(long s, long N, long n) { return (s >> 1) * N + ((s & 1) ? N - n : 0); }

// grid.x = column groups x S (column group fastest); mean [S][n_par]
__global__ __launch_bounds__(64 * kDiagRG) void k_diag_mean(const double *x, long N, long n, long n_par, long ld,
                                                            long n_cg, double *mean)
{
    __shared__ double part[kDiagRG][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long s = blockIdx.x / n_cg, p = (blockIdx.x % n_cg) * 64 + lane;
    const bool live = p < n_par;
    const double *xs = x + diag_row0(s, N, n) * ld + p;
    // pass 0 sums the values (m = 0), pass 1 the residuals about that mean: the result is the mean rounded once,
    // whatever the column's offset
    double m = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        double a = 0.0;
        if (live) {
#pragma unroll 8
            for (long i = g; i < n; i += kDiagRG) a += xs[i * ld] - m;
        }
        part[g][lane] = a;
        __syncthreads();
        double t = part[0][lane];
#pragma unroll
        for (int gg = 1; gg < kDiagRG; ++gg) t += part[gg][lane];
        m = m + t / (double)n;
        __syncthreads();
    }
    if (live && g == 0) mean[s * n_par + p] = m;
}

// KB steps i .. i + KB - 1 of one thread: acc[k] += (x[i+j] - mu) (x[i+j+t0+k] - mu).  win[(j + k) % KB] holds
// x[i + j + t0 + k] - mu at step j, and step j's slot is refilled with row i + j + t0 + KB.  The loads come kDiagLC
// steps at a time, one chunk ahead of the fma that use them (the scheduling barriers keep the compiler from hoisting
// all 2 KB loads, which spills).  GUARD: rows at or beyond n count as 0, so a lag's sum ends where its pairs end.
constexpr int kDiagLC = 4;
template <int KB, bool GUARD>
__device__ __forceinline__ void diag_steps(const double *xs, unsigned lane, long ld, double mu, long i, long t0, long n,
                                           double (&acc)[KB], double (&win)[KB])
{
    double la[kDiagLC], lw[kDiagLC];
    auto load = [&](int c) {
        // the lane's byte offset, opaque to the optimiser: kept as a 32-bit offset beside the scalar row address, not
        // folded into one 64-bit vector address per row
        unsigned lb = lane * 8u;
        asm volatile("" : "+v"(lb));
#pragma unroll
        for (int j = 0; j < kDiagLC; ++j) {
            const long ra = i + c * kDiagLC + j, rw = ra + t0 + KB;
            la[j] = !GUARD || ra < n ? *(const double *)((const char *)(xs + ra * ld) + lb) : mu;
            lw[j] = !GUARD || rw < n ? *(const double *)((const char *)(xs + rw * ld) + lb) : mu;
        }
    };
    load(0);
#pragma unroll
    for (int c = 0; c < KB / kDiagLC; ++c) {
        double ca[kDiagLC], cw[kDiagLC];
#pragma unroll
        for (int j = 0; j < kDiagLC; ++j) { ca[j] = la[j] - mu; cw[j] = lw[j] - mu; }
        if (c + 1 < KB / kDiagLC) load(c + 1);
#pragma unroll
        for (int j = 0; j < kDiagLC; ++j) {
            const int jj = c * kDiagLC + j;
#pragma unroll
            for (int k = 0; k < KB; ++k) acc[k] = fma(ca[j], win[(jj + k) % KB], acc[k]);
            win[jj] = cw[j];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// grid.x = slabs of seq_per_slab split sequences x column groups x lag workgroups (lag workgroup fastest);
// part [slab][L+1][n_par] = this slab's sum over its sequences and over i of (x_i - mu)(x_{i+t} - mu).
// Consecutive workgroup ids go round the 8 XCDs, each with an L2 of its own; the ids are renumbered (a bijection) so
// that the lag workgroups of one column group and slab, which stream the same rows, share an XCD.  Speed only.
template <int KB>
__global__ __launch_bounds__(64 * kDiagLW, 2) void k_diag_acov(const double *x, long N, long n, long n_par, long ld, int L,
                                                            int S, int seq_per_slab, long n_lagwg, long n_cg,
                                                            const double *mean, double *part)
{
    const long q8 = gridDim.x / 8, r8 = gridDim.x % 8, xcd = blockIdx.x % 8;
    const long wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + blockIdx.x / 8;
    const long slab = wg / (n_lagwg * n_cg);
    // w is the wave's, so row addresses and loop bounds stay scalar and a load is scalar row base + lane offset
    const unsigned lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long t0 = ((wg % n_lagwg) * kDiagLW + w) * KB;
    const long p0 = (wg / n_lagwg % n_cg) * 64, p = p0 + lane;
    if (t0 > L || p >= n_par) return;
    const int s0 = (int)slab * seq_per_slab, s1 = min(S, s0 + seq_per_slab);
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = 0.0;
    for (int s = s0; s < s1; ++s) {
        const double mu = mean[(long)s * n_par + p];
        const double *xs = x + diag_row0(s, N, n) * ld + p0;
        double win[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) win[k] = t0 + k < n ? (xs + (t0 + k) * ld)[lane] - mu : 0.0;
        long i = 0;
        for (; i + t0 + 2 * KB <= n; i += KB) diag_steps<KB, false>(xs, lane, ld, mu, i, t0, n, acc, win);   // every row exists
        for (; i + t0 < n; i += KB) diag_steps<KB, true>(xs, lane, ld, mu, i, t0, n, acc, win);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k)
        if (t0 + k <= L) part[(slab * (L + 1) + t0 + k) * n_par + p] = acc[k];
}

// out [n_par][4] = {rhat, ess, tau, lags}; acov [(L+1)][n_par] or NULL; tau_min = 1 / log10(S n)
__global__ __launch_bounds__(64) void k_diag_finish(const double *part, const double *mean, long n, long n_par, int L, int S,
                                                    int n_slab, double tau_min, double *out, double *acov)
{
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p >= n_par) return;
    const double dn = (double)n, dS = (double)S;
    auto ac = [&](int t) {
        double a = part[(long)t * n_par + p];
        for (int g = 1; g < n_slab; ++g) a += part[((long)g * (L + 1) + t) * n_par + p];
        return a / dn / dS;
    };
    double mm = 0.0;
    for (int s = 0; s < S; ++s) mm += mean[(long)s * n_par + p];
    mm /= dS;
    double bn = 0.0;
    for (int s = 0; s < S; ++s) {
        const double d = mean[(long)s * n_par + p] - mm;
        bn += d * d;
    }
    bn /= dS - 1.0;
    const double a0 = ac(0);
    const double W = a0 * dn / (dn - 1.0);
    const double vp = (dn - 1.0) / dn * W + bn;
    const bool ok = W > 0.0;                     // false for a constant column (and for NaN)
    double sum = 0.0, prev = INFINITY;
    int lags = -1;
    bool done = !ok;
    for (int t = 0; t <= L; t += 2) {
        const double at = t == 0 ? a0 : ac(t);
        if (acov) acov[(long)t * n_par + p] = at;
        if (t + 1 > L) break;                    // a last lag without a partner is not used
        const double au = ac(t + 1);
        if (acov) acov[(long)(t + 1) * n_par + p] = au;
        if (!done) {
            const double r0 = 1.0 - (W - at * dn / (dn - 1.0)) / vp;
            const double r1 = 1.0 - (W - au * dn / (dn - 1.0)) / vp;
            double P = r0 + r1;
            if (P < 0.0) {
                done = true;
                lags = t;
            } else {
                P = fmin(P, prev);
                sum += P;
                prev = P;
            }
        }
        if (done && !acov) break;
    }
    double *o = out + p * 4;
    if (!ok) {
        o[0] = o[1] = o[2] = o[3] = NAN;
        return;
    }
    const double tau = fmax(-1.0 + 2.0 * sum, tau_min);
    o[0] = sqrt(vp / W);
    o[1] = dS * dn / tau;
    o[2] = tau;
    o[3] = (double)lags;
}

}  // namespace htm
