// htm_convert.hpp -- step 1 of the reference pipeline on the GPU: the smoothed, merged envelopes of
// `hypo_tremor_convert` (src/cls_convertor.f90:84-443, src/mod_signal_process.f90:10-26).
//
// A station's record of N samples is cut into segments of n samples every n2 = n/2 (segment j covers stream samples
// [j n2, j n2 + n), samples at or beyond N read as 0).  Per segment, as the reference does per component:
//   k_cv_detrend   the least-squares line in the 1-based index, both components (one workgroup per segment);
//   k_cv_pack      x - line, tapered, the two components packed as one complex row z = x1 + i x2;
//   (forward FFT of z, htm_fft.hpp)
//   k_cv_spectrum  the two spectra separated, X1 = (Z[k] + conj Z[n-k]) / 2, X2 = (Z[k] - conj Z[n-k]) / 2i, weighted
//                  by the band and doubled up to bin n/2: Y[0] = 0, Y[k] = 2 w(k) X[k] for 1 <= k <= n/2, 0 above;
//   (backward FFT of Y1 and Y2)
//   k_cv_smooth    e = |y / n|, the two box smoothings of half width h with the reference's windows, the merge
//                  sqrt((e1 fac1)^2 + (e2 fac2)^2), and only the kept, decimated samples written out.
// The box sums come from per-tile prefix sums in LDS (tiles of kCvTile outputs with a halo of h on each side), not
// from the reference's serial recurrence.  See DESIGN.md §3.5.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

#include "htm_fft.hpp"
#include "htm_xcorr.hpp"

namespace htm {

constexpr int kCvThreads = 256;
constexpr int kCvTile = 1024;           // smoothed outputs per workgroup
constexpr int kCvMaxH = 4096;           // half width: 2 (kCvTile + 2h) doubles of LDS stay within 160 KiB
constexpr int kCvSumThreads = 1024;

// sample m (0-based, segment-local) of component c of segment s; chunk sample 0 is stream sample j0 n2
__device__ __forceinline__ double cv_sample(const float *x, long s, long m, int n2, long n_valid)
{
    const long q = s * n2 + m;
    return q < n_valid ? (double)x[q] : 0.0;
}

// coef[4 s + 2 c + {0, 1}] = (a, b) of src/cls_convertor.f90:368-394 for component c of segment s: the mean first,
// then sxy = sum (x_i - mean)(i - xbar); sxx = n (n^2 - 1) / 12 = sum (i - xbar)^2
__global__ __launch_bounds__(kCvSumThreads) void k_cv_detrend(const float *x1, const float *x2, long n_valid, int n,
                                                             double *coef)
{
    __shared__ double scratch[2 * (kCvSumThreads / 64)];
    const long s = blockIdx.x;
    const int n2 = n / 2;
    double a = 0.0, b = 0.0;
    for (int m = threadIdx.x; m < n; m += blockDim.x) {
        a += cv_sample(x1, s, m, n2, n_valid);
        b += cv_sample(x2, s, m, n2, n_valid);
    }
    xc_block_sum2(a, b, scratch);
    const double ym1 = a / n, ym2 = b / n, xm = 0.5 * (1.0 + (double)n);
    a = 0.0; b = 0.0;
    for (int m = threadIdx.x; m < n; m += blockDim.x) {
        const double d = (double)(m + 1) - xm;
        a += (cv_sample(x1, s, m, n2, n_valid) - ym1) * d;
        b += (cv_sample(x2, s, m, n2, n_valid) - ym2) * d;
    }
    xc_block_sum2(a, b, scratch);
    if (threadIdx.x == 0) {
        const double sxx = (double)n * ((double)n * (double)n - 1.0) / 12.0;
        const double s1 = a / sxx, s2 = b / sxx;
        coef[4 * s + 0] = s1; coef[4 * s + 1] = ym1 - s1 * xm;
        coef[4 * s + 2] = s2; coef[4 * s + 3] = ym2 - s2 * xm;
    }
}

// z[s][m] = ((x1 - a1 i - b1) f, (x2 - a2 i - b2) f), i = m + 1, f = the taper of src/mod_signal_process.f90:17-22
__global__ __launch_bounds__(kCvThreads) void k_cv_pack(const float *x1, const float *x2, long n_valid, int n,
                                                       const double *coef, double2 *z, long total)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long s = g / n;
    const int m = (int)(g - s * n);
    const double f = xc_taper(m, n, (int)(n * 0.05)), i = (double)(m + 1);
    const double *c = coef + 4 * s;
    const double v1 = cv_sample(x1, s, m, n / 2, n_valid) - (c[0] * i + c[1]);
    const double v2 = cv_sample(x2, s, m, n / 2, n_valid) - (c[2] * i + c[3]);
    z[g] = make_double2(v1 * f, v2 * f);
}

// band weight of src/cls_convertor.f90:309-338 at 0-based bin k, edges k1..k4 = nint(f_i / df)
__device__ __forceinline__ double cv_weight(int k, const int4 kb)
{
    if (k < kb.x) return 0.0;
    if (k < kb.y) return 0.5 * (1.0 - cos((double)(k - kb.x) * M_PI / (double)(kb.y - kb.x)));
    if (k < kb.z) return 1.0;
    if (k < kb.w) return 0.5 * (1.0 + cos((double)(k - kb.z) * M_PI / (double)(kb.w - kb.z)));
    return 0.0;
}

// y[2 s + c][k] = Y_c[k] of segment s (src/cls_convertor.f90:344-364) from the packed spectrum z[s]
__global__ __launch_bounds__(kCvThreads) void k_cv_spectrum(const double2 *z, int n, int4 kb, double2 *y, long total)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long s = g / n;
    const int k = (int)(g - s * n);
    double2 y1 = make_double2(0.0, 0.0), y2 = y1;
    if (k >= 1 && k <= n / 2) {
        const double2 p = z[s * n + k], q = c_conj(z[s * n + (n - k)]);
        const double w = cv_weight(k, kb);
        const double2 d = c_sub(p, q);                           // 2 i X2
        y1 = c_add(p, q);                                        // 2 X1
        y2 = make_double2(d.y, -d.x);                            // 2 X2
        y1.x *= w; y1.y *= w; y2.x *= w; y2.y *= w;
    }
    y[(2 * s) * n + k] = y1;
    y[(2 * s + 1) * n + k] = y2;
}

// Box smoothing of src/cls_convertor.f90:281-305 with half width h, 1-based i of n:
//   i <= h: sum x[1 .. i+h] / (i+h);  h < i <= n-h: sum x[i-h+1 .. i+h] / (2h+1);  i > n-h: sum x[i-h+1 .. n] / (n+h-i+1)
// i.e. the sum of x over [max(1, i-h+1), min(n, i+h)] with the reference's divisor.  One workgroup per (segment,
// tile); a tile is kCvTile consecutive outputs of [lo, hi), its inputs [t0 - h, t1 + h) are prefix-summed in LDS.
//   FINAL = false: the inputs are e = |y / n| of the complex rows y[2 s + c]; every output i in [0, n) is written to
//                  e1[(2 s + c) n + i].
//   FINAL = true:  the inputs are e1; outputs cover the kept range of segment j = j0 + s (first [0, n - n4), middle
//                  [n4, n - n4), last [n4, N - j n2)); where the stream sample g = j n2 + i is a multiple of n_fac,
//                  out[g / n_fac - k_base] = sqrt((v1 fac1)^2 + (v2 fac2)^2).
template <bool FINAL>
__global__ __launch_bounds__(kCvThreads) void k_cv_smooth(const double2 *y, const double *e1, double *e_out, int n, int h,
                                                         int tiles, long j0, long j_last, long n_total, int n_fac,
                                                         long k_base, double fac1, double fac2, double *out)
{
    extern __shared__ double cv_lds[];
    __shared__ double wsum[2 * (kCvThreads / 64)];
    const long s = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x - s * tiles);
    const int n2 = n / 2, n4 = n / 4;
    const long j = j0 + s;
    int lo = 0, hi = n;
    if (FINAL) {
        lo = j == 0 ? 0 : n4;
        hi = j == j_last ? (int)(n_total - j * n2) : n - n4;
    }
    const int t0 = lo + t * kCvTile;
    if (t0 >= hi) return;
    const int t1 = min(t0 + kCvTile, hi);
    const int r0 = max(0, t0 - h), r1 = min(n, t1 + h), L = r1 - r0;
    double *p1 = cv_lds, *p2 = cv_lds + L;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double carry1 = 0.0, carry2 = 0.0;
    for (int base = 0; base < L; base += blockDim.x) {
        const int m = base + threadIdx.x;
        double v1 = 0.0, v2 = 0.0;
        if (m < L) {
            if (FINAL) {
                v1 = e1[(2 * s) * n + r0 + m];
                v2 = e1[(2 * s + 1) * n + r0 + m];
            } else {
                const double2 a = y[(2 * s) * n + r0 + m], b = y[(2 * s + 1) * n + r0 + m];
                const double ax = a.x / n, ay = a.y / n, bx = b.x / n, by = b.y / n;
                v1 = sqrt(ax * ax + ay * ay);
                v2 = sqrt(bx * bx + by * by);
            }
        }
        for (int d = 1; d < 64; d <<= 1) {                       // inclusive scan within the wave
            const double u1 = __shfl_up(v1, d), u2 = __shfl_up(v2, d);
            if (lane >= d) { v1 += u1; v2 += u2; }
        }
        if (lane == 63) { wsum[2 * wv] = v1; wsum[2 * wv + 1] = v2; }
        __syncthreads();
        double o1 = carry1, o2 = carry2;
        for (int k = 0; k < nw; ++k) {
            if (k < wv) { o1 += wsum[2 * k]; o2 += wsum[2 * k + 1]; }
            carry1 += wsum[2 * k]; carry2 += wsum[2 * k + 1];
        }
        if (m < L) { p1[m] = o1 + v1; p2[m] = o2 + v2; }
        __syncthreads();
    }
    for (int i = t0 + threadIdx.x; i < t1; i += blockDim.x) {
        const int a = max(0, i - h + 1), b = min(n - 1, i + h);       // window [a, b], empty when h = 0
        double s1 = p1[b - r0], s2 = p2[b - r0];
        if (a > r0) { s1 -= p1[a - 1 - r0]; s2 -= p2[a - 1 - r0]; }
        const int i1 = i + 1;
        const double div = (double)(i1 <= h ? i1 + h : (i1 > n - h ? n + h - i1 + 1 : 2 * h + 1));
        const double v1 = s1 / div, v2 = s2 / div;
        if (!FINAL) {
            e_out[(2 * s) * n + i] = v1;
            e_out[(2 * s + 1) * n + i] = v2;
        } else {
            const long g = j * n2 + i;
            if (g % n_fac == 0) {
                const double q1 = v1 * fac1, q2 = v2 * fac2;
                out[g / n_fac - k_base] = sqrt(q1 * q1 + q2 * q2);
            }
        }
    }
}

}  // namespace htm
