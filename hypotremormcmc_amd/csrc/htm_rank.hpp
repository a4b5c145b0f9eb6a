// htm_rank.hpp -- rank normalisation of recorded samples: the average rank of every element within its column and its
// normal score z = Phi^-1((r - 3/8) / (R + 1/4)) (Vehtari et al. 2021; definitions: DESIGN.md §3.7).  With the folded form
// |x - med| and two tail indicators it gives, through the unchanged kernels of htm_diag.hpp, the rank-normalised R-hat,
// the bulk-ESS and the tail-ESS.
//
// Layout: samples are [R][ld] row-major, parameter p in column p.  A batch of nb columns is ranked at a time (the host
// sizes nb by HTM_RANK_MB); its keys live column-major, keys [nb][R], in two buffers the sort goes to and fro between.
//
//   k_rank_keys       LDS tile transpose (64 rows x 64 columns) of the batch into keys: the order-preserving integer image of
//                     htm_select.hpp (sel_key) of x, -0.0 first made +0.0, or of |x - med| when folded
//   k_rank_sort       one workgroup of kRankWaves waves per column: a stable least-significant-digit radix sort, 8 passes of
//                     8 bits.  All 8 histograms are counted in one first sweep (a digit's histogram does not depend on the
//                     order).  A pass scatters tile by tile, kRankTile = 1024 consecutive elements, element <-> thread: the
//                     lanes of a wave that hold the same digit find each other with 8 wave ballots, a lane's offset within its
//                     digit is the count of such lanes below it, the waves' counts per digit are laid end to end in LDS by
//                     one thread per digit, which also moves the digit's running start on.  Integer LDS atomics only (exact,
//                     order-free), and a position depends on nothing but the element's index: two runs give the same bits.
//   k_rank_z          lane <-> column, so reads of x and writes of z are coalesced row segments: lower and upper bound of the
//                     element's key in its sorted column give lo = #{<} and hi = #{<=}, r = (lo + hi + 1) / 2 exactly, ties
//                     included; z by rank_ndtri
//   k_rank_thresholds med, q05, q95 of every column from six order statistics (two calls of htm_quantiles_dev)
//   k_rank_indicator  [x <= q05] or [x >= q95] as 0.0 / 1.0
//   k_rank_combine    out [n_par][4] = {rhat(z), rhat(zf), ess(z), min(ess(I05), ess(I95))}
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "htm_select.hpp"      // sel_key

namespace htm {

constexpr int kRankWaves = 16;                   // waves per workgroup of k_rank_sort
constexpr int kRankTile = 64 * kRankWaves;       // elements per scatter tile: 1024
constexpr int kRankZRows = 256;                  // rows per workgroup of k_rank_z and k_rank_indicator

// Phi^-1 by Wichura's algorithm AS 241 (PPND16, Applied Statistics 37 (1988) 477-484; relative accuracy about 1e-16), 0 < p < 1.
// The rational functions are evaluated by Horner's rule without fused multiply-adds.
__device__ __forceinline__ double rank_ndtri(double p)
{
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                              4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = sqrt(-log(q <= 0.0 ? p : 1.0 - p));
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                 5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// the key of an element: -0.0 and +0.0 are one value; folded: the image of |x - med|
__device__ __forceinline__ unsigned long long rank_key(double v, bool fold, double med)
{
    if (fold) v = fabs(v - med);
    if (v == 0.0) v = 0.0;
    return sel_key(v);
}

// grid.x = row tiles x column tiles of the batch (row tile fastest); columns c0 .. c0 + nb - 1 of x; med [n_par] or NULL
__global__ __launch_bounds__(256) void k_rank_keys(const double *x, long R, long ld, long c0, long nb, long n_rt, const double *med,
                                                   unsigned long long *keys)
{
    __shared__ unsigned long long tile[64][65];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long r0 = (blockIdx.x % n_rt) * 64, b0 = (blockIdx.x / n_rt) * 64;
    {
        const long b = b0 + lane;
        if (b < nb) {
            const double m = med ? med[c0 + b] : 0.0;
            for (int rr = g; rr < 64 && r0 + rr < R; rr += 4) tile[rr][lane] = rank_key(x[(r0 + rr) * ld + c0 + b], med != nullptr, m);
        }
    }
    __syncthreads();
    if (r0 + lane < R)
        for (int cc = g; cc < 64 && b0 + cc < nb; cc += 4) keys[(size_t)(b0 + cc) * R + r0 + lane] = tile[lane][cc];
}

// For an active lane: the active lanes of its wave that hold the same 8-bit digit.  Every lane of the wave must call it.
__device__ __forceinline__ unsigned long long rank_match(unsigned dig, bool active)
{
    unsigned long long m = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (dig >> b) & 1u;
        const unsigned long long v = __ballot(active && bit);
        m &= bit ? v : ~v;
    }
    return m;
}

// grid.x = columns of the batch; a [nb][R] holds the keys and receives them sorted, b [nb][R] is the other buffer
__global__ __launch_bounds__(kRankTile) void k_rank_sort(unsigned long long *a, unsigned long long *b, long R)
{
    __shared__ int hist[8][256];              // first the counts, then the exclusive prefix = where the digit's next tile starts
    __shared__ int cnt[kRankWaves][256];      // a tile's count per wave and digit, then that wave's start; all zero between tiles
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long *src = a + (size_t)blockIdx.x * R, *dst = b + (size_t)blockIdx.x * R;
    for (int k = tid; k < 8 * 256; k += kRankTile) (&hist[0][0])[k] = 0;
    for (int k = tid; k < kRankWaves * 256; k += kRankTile) (&cnt[0][0])[k] = 0;
    __syncthreads();
    for (long base = 0; base < R; base += kRankTile) {
        const long i = base + tid;
        const bool active = i < R;
        const unsigned long long key = active ? src[i] : 0ull;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const unsigned dig = (unsigned)(key >> (8 * p)) & 255u;
            const unsigned long long m = rank_match(dig, active);
            if (active && (m & below) == 0ull) atomicAdd(&hist[p][dig], __popcll(m));
        }
    }
    __syncthreads();
    if (w < 8) {
        // wave w turns hist[w] into its exclusive prefix sum: four consecutive digits per lane
        int v[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = hist[w][4 * lane + k]; s += v[k]; }
        int incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        int run = incl - s;
#pragma unroll
        for (int k = 0; k < 4; ++k) { hist[w][4 * lane + k] = run; run += v[k]; }
    }
    __syncthreads();
    for (int p = 0; p < 8; ++p) {
        for (long base = 0; base < R; base += kRankTile) {
            const long i = base + tid;
            const bool active = i < R;
            const unsigned long long key = active ? src[i] : 0ull;
            const unsigned dig = (unsigned)(key >> (8 * p)) & 255u;
            const unsigned long long m = rank_match(dig, active);
            const int before = __popcll(m & below);
            const bool leader = active && before == 0;
            if (leader) cnt[w][dig] = __popcll(m);
            __syncthreads();
            if (tid < 256) {
                // digit tid: the waves' elements follow each other in wave order from the digit's running start
                int c[kRankWaves];
#pragma unroll
                for (int ww = 0; ww < kRankWaves; ++ww) c[ww] = cnt[ww][tid];
                int run = hist[p][tid];
#pragma unroll
                for (int ww = 0; ww < kRankWaves; ++ww) { cnt[ww][tid] = c[ww] ? run : 0; run += c[ww]; }   // nobody clears a start without elements
                hist[p][tid] = run;
            }
            __syncthreads();
            const int pos = active ? cnt[w][dig] + before : 0;
            __builtin_amdgcn_wave_barrier();          // every lane of the wave has read its start before the leader clears it
            if (leader) cnt[w][dig] = 0;
            if (active) dst[pos] = key;
        }
        __syncthreads();                              // the pass's stores are visible to the whole workgroup
        unsigned long long *t = src; src = dst; dst = t;
    }
}

// grid.x = column groups of the batch x row chunks of kRankZRows (column group fastest); sorted [nb][R]; z, ranks: row stride ld_z
__global__ __launch_bounds__(256) void k_rank_z(const double *x, long R, long ld, long c0, long nb, long n_cg, const double *med,
                                                const unsigned long long *sorted, double *z, double *ranks, long ld_z)
{
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long b = (blockIdx.x % n_cg) * 64 + lane, r0 = (blockIdx.x / n_cg) * kRankZRows;
    if (b >= nb) return;
    const double m = med ? med[c0 + b] : 0.0, dR = (double)R + 0.25;
    const unsigned long long *s = sorted + (size_t)b * R;
    for (long i = r0 + g; i < min(R, r0 + kRankZRows); i += 4) {
        const unsigned long long key = rank_key(x[i * ld + c0 + b], med != nullptr, m);
        long lo = 0, n = R;                           // lo = #{keys < key}
        while (n > 0) {
            const long h = n >> 1;
            if (s[lo + h] < key) { lo += h + 1; n -= h + 1; } else n = h;
        }
        long hi = lo + 1;                             // hi = #{keys <= key}: s[lo] is the key itself
        if (hi < R && s[hi] == key) {
            n = R - hi;
            while (n > 0) {
                const long h = n >> 1;
                if (s[hi + h] <= key) { hi += h + 1; n -= h + 1; } else n = h;
            }
        }
        const double r = (double)(lo + hi + 1) * 0.5;
        z[i * ld_z + c0 + b] = rank_ndtri((r - 0.375) / dR);
        if (ranks) ranks[i * ld_z + c0 + b] = r;
    }
}

// qa [n_par][3] = the order statistics (R+1)/2, R/2+1, k05+1; qb [n_par][3] = min(k05+2, R), k95+1, min(k95+2, R) (1-based);
// thr [3][n_par] = med, q05, q95.  q = a + g (b - a): one multiply and two adds (the unit is compiled without contraction).
__global__ __launch_bounds__(64) void k_rank_thresholds(const double *qa, const double *qb, long n_par, double g05, double g95,
                                                        double *thr)
{
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p >= n_par) return;
    thr[p] = 0.5 * (qa[p * 3] + qa[p * 3 + 1]);
    const double a05 = qa[p * 3 + 2], b05 = qb[p * 3], a95 = qb[p * 3 + 1], b95 = qb[p * 3 + 2];
    thr[n_par + p] = a05 + g05 * (b05 - a05);
    thr[2 * n_par + p] = a95 + g95 * (b95 - a95);
}

// med [n_par] alone, for htm_rank_normalize_dev's folded form: qa [n_par][3], its first two entries as above
__global__ __launch_bounds__(64) void k_rank_median(const double *qa, long n_par, double *med)
{
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p < n_par) med[p] = 0.5 * (qa[p * 3] + qa[p * 3 + 1]);
}

// grid.x = column groups x row chunks of kRankZRows (column group fastest); ind [R][n_par] = upper ? [x >= q] : [x <= q]
__global__ __launch_bounds__(256) void k_rank_indicator(const double *x, long R, long n_par, long ld, long n_cg, const double *q,
                                                        int upper, double *ind)
{
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long p = (blockIdx.x % n_cg) * 64 + lane, r0 = (blockIdx.x / n_cg) * kRankZRows;
    if (p >= n_par) return;
    const double t = q[p];
    for (long i = r0 + g; i < min(R, r0 + kRankZRows); i += 4) {
        const double v = x[i * ld + p];
        ind[i * n_par + p] = (upper ? v >= t : v <= t) ? 1.0 : 0.0;
    }
}

// d [4][n_par][4]: htm_diagnose_dev's out for z, zf, I05, I95; out [n_par][4] = {rhat_bulk, rhat_folded, ess_bulk, ess_tail}
__global__ __launch_bounds__(64) void k_rank_combine(const double *d, long n_par, double *out)
{
    const long p = (long)blockIdx.x * 64 + threadIdx.x;
    if (p >= n_par) return;
    const double e05 = d[(2 * n_par + p) * 4 + 1], e95 = d[(3 * n_par + p) * 4 + 1];
    out[p * 4] = d[p * 4];
    out[p * 4 + 1] = d[(n_par + p) * 4];
    out[p * 4 + 2] = d[p * 4 + 1];
    out[p * 4 + 3] = isnan(e05) || isnan(e95) ? NAN : fmin(e05, e95);
}

}  // namespace htm
