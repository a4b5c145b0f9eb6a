// htm_xcorr.hpp -- steps 2 and 3 of the reference pipeline on the GPU: the windowed cross-correlations of
// `hypo_tremor_correlate` (src/cls_correlator.f90:205-232, src/mod_signal_process.f90) and the per-window lag and
// amplitude measurement of `hypo_tremor_measure` (src/cls_measurer.f90:405-523).
//
// The reference takes every circular correlation as c2r(conj(r2c(r_i)) * r2c(r_j)) with FFTW.  At n ~ 300 samples a
// direct sum is as cheap per pair as the FFT, so both kernels use the direct form
//     cc[k] = sum_m r_i[m] * r_j[(m + k) mod n]          (k = natural lag, 0 .. n-1)
// summed serially in m by one thread per lag, with both windows in LDS (2n doubles, 64 KB at n = 4096).  The two
// windows are prepared in registers first (at most kXcPer samples per thread and station), so the block sums of the
// preparation need no LDS beyond the two windows.  See DESIGN.md §3.4.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

namespace htm {

constexpr int kXcMaxN = 4096;          // longest window (samples)
constexpr int kXcMaxThreads = 1024;    // one thread per lag, up to this many
constexpr int kXcPer = kXcMaxN / kXcMaxThreads;

// threads per workgroup for windows of n samples: whole waves, one lag per thread up to 1024 lags
__host__ __device__ inline int xc_threads(int n)
{
    const int t = (n + 63) / 64 * 64;
    return t < kXcMaxThreads ? t : kXcMaxThreads;
}

// cosine taper of src/mod_signal_process.f90:17-22 at 0-based sample m: nleng = int(0.05 n) samples at each end,
// fac = 0.5 (1 - cos((i-1) pi / nleng)) for the 1-based sample i and its mirror n-i+1
__device__ __forceinline__ double xc_taper(int m, int n, int nleng)
{
    const int q = m < nleng ? m : (m >= n - nleng ? n - 1 - m : -1);
    if (q < 0) return 1.0;
    return 0.5 * (1.0 - cos((double)q * M_PI / (double)nleng));
}

// sums of a and b over the workgroup (every thread gets the same two values); scratch >= 2 * waves doubles
__device__ __forceinline__ void xc_block_sum2(double &a, double &b, double *scratch)
{
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { scratch[2 * w] = a; scratch[2 * w + 1] = b; }
    __syncthreads();
    a = 0.0; b = 0.0;
    for (int k = 0; k < nw; ++k) { a += scratch[2 * k]; b += scratch[2 * k + 1]; }
    __syncthreads();
}

// natural lag k of the circular correlation of the windows a and b (LDS), serial in m
__device__ __forceinline__ double xc_lag(const double *a, const double *b, int n, int k)
{
    double acc = 0.0;
    int m = 0;
    const int lim = n - k;
    for (; m < lim; ++m) acc = fma(a[m], b[m + k], acc);
    for (; m < n; ++m) acc = fma(a[m], b[m + k - n], acc);
    return acc;
}

// pair p (0-based) of the station-file order (0,1), (0,2), ..., (1,2), ... of n_sta stations
__device__ __forceinline__ void xc_pair(int p, int n_sta, int &i, int &j)
{
    int off = 0;
    i = 0;
    while (off + (n_sta - 1 - i) <= p) { off += n_sta - 1 - i; ++i; }
    j = i + 1 + (p - off);
}

// ---- step 2: one workgroup per (window, pair), window-major --------------------------------------------------------
// Window w of station s is env[s * ld_env + w * n_step + m], m < n.  Preparation as src/cls_correlator.f90:207-223:
// taper, subtract sum/n, divide by sqrt(sum x^2) -- a window with zero energy becomes all zeros (the reference keeps
// whatever its buffer held last).  Output order as :234-235: row j of the pair's column holds lag
// j - n/2, so negative lags come first; cc_max[w][p] = max_j cc.
__global__ __launch_bounds__(kXcMaxThreads) void k_xcorr(const double *env, long ld_env, int n_sta, int n, int n_step,
                                                         int n_win, int pair0, int n_pairs, double *cc, long ld_cc,
                                                         double *cc_max)
{
    extern __shared__ double xc_lds[];
    double *ra = xc_lds, *rb = xc_lds + n;
    const long blk = blockIdx.x;
    const int w = (int)(blk / n_pairs), p = (int)(blk % n_pairs);
    if (w >= n_win) return;
    int si, sj;
    xc_pair(pair0 + p, n_sta, si, sj);
    const int nleng = (int)(n * 0.05);
    const double *xa = env + (size_t)si * ld_env + (size_t)w * n_step;
    const double *xb = env + (size_t)sj * ld_env + (size_t)w * n_step;
    double va[kXcPer], vb[kXcPer];
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int u = 0; u < kXcPer; ++u) {
        const int m = threadIdx.x + u * blockDim.x;
        va[u] = 0.0; vb[u] = 0.0;
        if (m < n) {
            const double f = xc_taper(m, n, nleng);
            va[u] = xa[m] * f; vb[u] = xb[m] * f;
            sa += va[u]; sb += vb[u];
        }
    }
    xc_block_sum2(sa, sb, xc_lds);
    const double ma = sa / n, mb = sb / n;
    double qa = 0.0, qb = 0.0;
#pragma unroll
    for (int u = 0; u < kXcPer; ++u) {
        const int m = threadIdx.x + u * blockDim.x;
        if (m < n) {
            va[u] = va[u] - ma; vb[u] = vb[u] - mb;
            qa += va[u] * va[u]; qb += vb[u] * vb[u];
        }
    }
    xc_block_sum2(qa, qb, xc_lds);
    const double la = sqrt(qa), lb = sqrt(qb);
#pragma unroll
    for (int u = 0; u < kXcPer; ++u) {
        const int m = threadIdx.x + u * blockDim.x;
        if (m < n) {
            ra[m] = la != 0.0 ? va[u] / la : 0.0;
            rb[m] = lb != 0.0 ? vb[u] / lb : 0.0;
        }
    }
    __syncthreads();
    double best = -INFINITY;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const double v = xc_lag(ra, rb, n, k);
        const int j = k < n / 2 ? k + n / 2 : k - n / 2;
        cc[((size_t)w * n + j) * ld_cc + p] = v;
        best = fmax(best, v);
    }
    for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o));
    __syncthreads();                     // every lag is done with ra / rb: reuse them as scratch
    if ((threadIdx.x & 63) == 0) xc_lds[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) best = fmax(best, xc_lds[k]);
        cc_max[(size_t)w * ld_cc + p] = best;
    }
}

// ---- step 3: one workgroup per detected window -----------------------------------------------------------------------
// x[win][s][m] raw envelope samples; ws[win] = n_sta * n_sta + n_sta doubles of workspace.
// optimize_cc (src/cls_measurer.f90:463-523): r = taper(x) / sum(x^2) (no demean; a station with zero energy gives
// r = 0, hence lag 0 against every station); the FIRST maximum of each pair's correlation in natural order; lag =
// idx dt for idx < n/2, (idx - n) dt otherwise; t and t_stdv summed serially in j by one lane per station.
// optimize_amp (:405-459): shift by nint(t/dt) (round half away from zero), sxx, sxy serially in the sample order,
// rel = log(sxy / sxx(i)); any sxy < 0 zeroes amp and amp_stdv of the whole window.
__global__ __launch_bounds__(kXcMaxThreads) void k_measure(const double *x, int n_sta, int n, double dt, int n_det,
                                                           double *ws, double *t, double *t_stdv, double *amp,
                                                           double *amp_stdv)
{
    extern __shared__ double xc_lds[];
    double *ra = xc_lds, *rb = xc_lds + n;
    const int win = blockIdx.x;
    if (win >= n_det) return;
    const int S = n_sta;
    const double *xw = x + (size_t)win * S * n;
    double *mat = ws + (size_t)win * ((size_t)S * S + S);      // lag(i,j), then rel(i,j), upper triangle i < j
    double *sv = mat + (size_t)S * S;                           // sum x^2 per station, then sxx
    double *tw = t + (size_t)win * S, *tsw = t_stdv + (size_t)win * S;
    double *aw = amp + (size_t)win * S, *asw = amp_stdv + (size_t)win * S;
    const int nleng = (int)(n * 0.05);
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        double l = 0.0;
        for (int m = 0; m < n; ++m) l += xw[(size_t)s * n + m] * xw[(size_t)s * n + m];
        sv[s] = l;
    }
    __syncthreads();
    for (int i = 0; i < S - 1; ++i) {
        for (int j = i + 1; j < S; ++j) {
            const double li = sv[i], lj = sv[j];
            for (int m = threadIdx.x; m < n; m += blockDim.x) {
                const double f = xc_taper(m, n, nleng);
                ra[m] = li != 0.0 ? xw[(size_t)i * n + m] * f / li : 0.0;
                rb[m] = lj != 0.0 ? xw[(size_t)j * n + m] * f / lj : 0.0;
            }
            __syncthreads();
            double best = -INFINITY;
            int bi = 0x7fffffff;
            for (int k = threadIdx.x; k < n; k += blockDim.x) {
                const double v = xc_lag(ra, rb, n, k);
                if (bi == 0x7fffffff || v > best) { best = v; bi = k; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(best, o);
                const int oi = __shfl_xor(bi, o);
                if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
            }
            __syncthreads();             // the windows are no longer read: their LDS holds the wave maxima
            if ((threadIdx.x & 63) == 0) { ra[2 * (threadIdx.x >> 6)] = best; ra[2 * (threadIdx.x >> 6) + 1] = (double)bi; }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int k = 1; k < (int)(blockDim.x >> 6); ++k) {
                    const double ov = ra[2 * k];
                    const int oi = (int)ra[2 * k + 1];
                    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
                }
                mat[(size_t)i * S + j] = bi < n / 2 ? (double)bi * dt : (double)(bi - n) * dt;
            }
            __syncthreads();
        }
    }
    // t(i) = -sum_j lag(i,j) / n_sta, lag(j,i) = -lag(i,j), lag(i,i) = 0
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        double a = 0.0;
        for (int j = 0; j < S; ++j) a = a - (j > i ? mat[(size_t)i * S + j] : (j < i ? -mat[(size_t)j * S + i] : 0.0));
        tw[i] = a / S;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        double a = 0.0;
        for (int j = 0; j < S; ++j) {
            if (j == i) continue;
            const double lag = j > i ? mat[(size_t)i * S + j] : -mat[(size_t)j * S + i];
            const double d = tw[j] - tw[i] - lag;
            a = a + d * d;
        }
        tsw[i] = sqrt(a / (S - 2));
    }
    __syncthreads();
    // optimize_amp: x2(:,i) = x(m + it_i) where 0 <= m + it_i < n, else 0
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        const int it = (int)round(tw[i] / dt);
        double a = 0.0;
        for (int m = 0; m < n; ++m) {
            const int q = m + it;
            const double v = (q >= 0 && q < n) ? xw[(size_t)i * n + q] : 0.0;
            a = a + v * v;
        }
        sv[i] = a;
    }
    __syncthreads();
    int neg = 0;
    for (int pq = threadIdx.x; pq < S * S; pq += blockDim.x) {
        const int i = pq / S, j = pq % S;
        if (j <= i) continue;
        const int iti = (int)round(tw[i] / dt), itj = (int)round(tw[j] / dt);
        double a = 0.0;
        for (int m = 0; m < n; ++m) {
            const int qi = m + iti, qj = m + itj;
            const double vi = (qi >= 0 && qi < n) ? xw[(size_t)i * n + qi] : 0.0;
            const double vj = (qj >= 0 && qj < n) ? xw[(size_t)j * n + qj] : 0.0;
            a = a + vi * vj;
        }
        if (a < 0.0) neg = 1;
        mat[(size_t)i * S + j] = log(a / sv[i]);
    }
    if (__syncthreads_or(neg)) {
        for (int i = threadIdx.x; i < S; i += blockDim.x) { aw[i] = 0.0; asw[i] = 0.0; }
        return;
    }
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        double a = 0.0;
        for (int j = 0; j < S; ++j) a = a - (j > i ? mat[(size_t)i * S + j] : (j < i ? -mat[(size_t)j * S + i] : 0.0));
        aw[i] = a / S;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        double a = 0.0;
        for (int j = 0; j < S; ++j) {
            if (j == i) continue;
            const double rel = j > i ? mat[(size_t)i * S + j] : -mat[(size_t)j * S + i];
            const double d = aw[j] - aw[i] - rel;
            a = a + d * d;
        }
        asw[i] = sqrt(a / (S - 2));
    }
}

}  // namespace htm
