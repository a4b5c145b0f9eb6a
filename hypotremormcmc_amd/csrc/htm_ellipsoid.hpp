// htm_ellipsoid.hpp -- per-window location error ellipsoids of recorded samples: the 3 x 3 posterior covariance of every
// window's (x, y, z), its principal axes, the correlation of x, y, z with up to four pivot columns (vs, qs) and the squared
// Mahalanobis distance of every sample, whose rank-th smallest scales the ellipsoid to hold exactly `rank` samples
// (definitions: DESIGN.md §3.8).
//
// Layout: hypo is [n_mod][ld] row-major, one recorded model per row, window w in columns 3w, 3w+1, 3w+2 (the record of
// hypo.RR.out); pivots [n_mod][ld_piv] pair with it row by row.
//
//   k_ell_range    per row slab and column (hypo and pivot columns alike): sum, min, max; lane <-> column, a wave per column
//                  group and slab, the waves of a workgroup on neighbouring column groups of the same rows
//   k_ell_mean     per row slab and column: the sum of the residuals about the mean of the first pass
//   k_ell_stats    one lane per column: mean = first mean + mean residual (rounded about once whatever the offset), min, max;
//                  min == max marks a constant column (exact, order-free), whose mean is that value
//   k_ell_moments  per row slab and window: the six centred second moments of (x, y, z), the 3 n_piv cross moments with the
//                  pivots and the pivots' own.  A wave owns 64 consecutive windows = 192 consecutive doubles of a row, which
//                  it loads as three coalesced 512-B segments; the three coordinates of a window arrive in three lanes and
//                  are brought to lane <-> window through the wave's own LDS tile (ds_write_b64 of column l, ds_read_b64 at
//                  3 l + k: 6 dwords apart, conflict-free over a 32-lane half).  kEllU rows are in flight per thread.  A pivot
//                  value is row-uniform: a scalar load.
//   k_ell_slabs    one lane per sum and window: adds the slabs' moments in ascending order
//   k_ell_finish   one lane per window: covariance, cyclic Jacobi with a fixed sweep count, eigenvalues descending, largest
//                  component of every axis positive, correlations
//   k_ell_maha     d2 [n_mod][batch] of a batch of windows, in the eigenbasis; loads as k_ell_moments, stores coalesced
//   k_ell_setq     the batch's order statistic of d2 (htm_quantiles_dev) into out
//
// No atomics: a thread adds its rows in ascending order and the slabs are added in ascending order, so two runs give the
// same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace htm {

constexpr int kEllWG = 4;         // column or window groups (waves) per workgroup of the streaming kernels
constexpr int kEllU = 8;          // rows in flight per thread
constexpr int kEllOut = 22;       // doubles per window of out: mean[3], cov[6], lambda[3], V[9], q
constexpr int kEllSweeps = 8;     // Jacobi sweeps
constexpr int kEllMaxPiv = 4;

// the sample columns the mean kernels see as one index space: 3 n_win hypo columns, then n_piv pivot columns; the pivots are
// a column group of their own (lane l < n_piv)
struct EllCols {
    const double *hypo, *piv;
    long ld, ld_piv, n_hc, n_hcg;     // n_hc = 3 n_win, n_hcg = its column groups
    int n_piv;
};
__device__ __forceinline__ const double *ell_col(const EllCols &c, long cg, int lane, long *stride, long *col)
{
    if (cg < c.n_hcg) {
        const long p = cg * 64 + lane;
        *stride = c.ld;
        *col = p;
        return p < c.n_hc ? c.hypo + p : nullptr;
    }
    *stride = c.ld_piv;
    *col = c.n_hc + lane;
    return lane < c.n_piv ? c.piv + lane : nullptr;
}

// grid = (column groups / kEllWG, slabs): a wave takes one column group and the slab's rows in ascending order, the waves of a
// workgroup neighbouring column groups of the same rows; part [slab][3][n_col] = sum, min, max of the slab's rows
__global__ __launch_bounds__(64 * kEllWG) void k_ell_range(EllCols c, long n_mod, long slab_rows, double *part)
{
    const int lane = threadIdx.x & 63;
    const long cg = (long)blockIdx.x * kEllWG + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    long stride, col;
    const double *x = ell_col(c, cg, lane, &stride, &col);
    if (cg >= c.n_hcg + (c.n_piv > 0) || !x) return;
    const long row0 = (long)blockIdx.y * slab_rows, row1 = min(n_mod, row0 + slab_rows), n_col = c.n_hc + c.n_piv;
    double s = 0.0, mn = INFINITY, mx = -INFINITY;
#pragma unroll 8
    for (long i = row0; i < row1; ++i) {
        const double v = x[i * stride];
        s += v;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    double *o = part + (long)blockIdx.y * 3 * n_col + col;
    o[0] = s;
    o[n_col] = mn;
    o[2 * n_col] = mx;
}

// the mean of the first pass: the slabs' sums added in ascending order
__device__ __forceinline__ double ell_mean0(const double *part, long n_col, long col, int n_slab, long n_mod)
{
    double s = part[col];
    for (int g = 1; g < n_slab; ++g) s += part[(long)g * 3 * n_col + col];
    return s / (double)n_mod;
}

// grid as k_ell_range; res [slab][n_col] = the slab's sum of residuals about ell_mean0
__global__ __launch_bounds__(64 * kEllWG) void k_ell_mean(EllCols c, long n_mod, long slab_rows, const double *part, int n_slab,
                                                           double *res)
{
    const int lane = threadIdx.x & 63;
    const long cg = (long)blockIdx.x * kEllWG + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    long stride, col;
    const double *x = ell_col(c, cg, lane, &stride, &col);
    if (cg >= c.n_hcg + (c.n_piv > 0) || !x) return;
    const long row0 = (long)blockIdx.y * slab_rows, row1 = min(n_mod, row0 + slab_rows), n_col = c.n_hc + c.n_piv;
    const double m = ell_mean0(part, n_col, col, n_slab, n_mod);
    double a = 0.0;
#pragma unroll 8
    for (long i = row0; i < row1; ++i) a += x[i * stride] - m;
    res[(long)blockIdx.y * n_col + col] = a;
}

// one lane per column; stats [3][n_col] = mean, min, max
__global__ __launch_bounds__(64) void k_ell_stats(const double *part, const double *res, long n_col, int n_slab, long n_mod,
                                                  double *stats)
{
    const long col = (long)blockIdx.x * 64 + threadIdx.x;
    if (col >= n_col) return;
    double r = res[col], mn = part[n_col + col], mx = part[2 * n_col + col];
    for (int g = 1; g < n_slab; ++g) {
        r += res[(long)g * n_col + col];
        mn = fmin(mn, part[((long)g * 3 + 1) * n_col + col]);
        mx = fmax(mx, part[((long)g * 3 + 2) * n_col + col]);
    }
    const double m = ell_mean0(part, n_col, col, n_slab, n_mod) + r / (double)n_mod;
    stats[col] = mn == mx ? mn : m;
    stats[n_col + col] = mn;
    stats[2 * n_col + col] = mx;
}

// Rows r .. r + U - 1 of the wave's 192 columns (base = hypo + the group's first column; columns at or beyond n_live are not
// read and count as 0): three coalesced loads per row, then through the wave's tile [U][192] to v[u][k] = coordinate k of
// the lane's window.  The LDS serves a wave's operations in order; the fences keep the compiler from moving them.
template <int U>
__device__ __forceinline__ void ell_fetch(const double *base, long ld, long r, int lane, int n_live, double *tile, double (&v)[U][3])
{
    double t[U][3];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < 3; ++i) t[u][i] = i * 64 + lane < n_live ? (base + (r + u) * ld)[i * 64 + lane] : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < 3; ++i) tile[u * 192 + i * 64 + lane] = t[u][i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[u][k] = tile[u * 192 + 3 * lane + k];
}

// accumulators of k_ell_moments: [0..5] xx, xy, xz, yy, yz, zz; [6 + 3k + a] coordinate a with pivot k; [6 + 3 NPIV + k] pivot k
constexpr int ell_nacc(int n_piv) { return 6 + 4 * n_piv; }

template <int NPIV, int U>
__device__ __forceinline__ void ell_add_rows(const double (&v)[U][3], const double (&mu)[3], const double *piv, long ld_piv, long r,
                                             const double *pm, double (&acc)[ell_nacc(NPIV)])
{
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const double dx = v[u][0] - mu[0], dy = v[u][1] - mu[1], dz = v[u][2] - mu[2];
        acc[0] = fma(dx, dx, acc[0]);
        acc[1] = fma(dx, dy, acc[1]);
        acc[2] = fma(dx, dz, acc[2]);
        acc[3] = fma(dy, dy, acc[3]);
        acc[4] = fma(dy, dz, acc[4]);
        acc[5] = fma(dz, dz, acc[5]);
#pragma unroll
        for (int k = 0; k < NPIV; ++k) {
            const double dp = piv[(r + u) * ld_piv + k] - pm[k];
            acc[6 + 3 * k] = fma(dx, dp, acc[6 + 3 * k]);
            acc[7 + 3 * k] = fma(dy, dp, acc[7 + 3 * k]);
            acc[8 + 3 * k] = fma(dz, dp, acc[8 + 3 * k]);
            acc[6 + 3 * NPIV + k] = fma(dp, dp, acc[6 + 3 * NPIV + k]);
        }
    }
}

// grid = (window groups / kEllWG, slabs); part [slab][ell_nacc(NPIV)][n_win]; stats as k_ell_stats wrote them
template <int NPIV>
__global__ __launch_bounds__(64 * kEllWG) void k_ell_moments(const double *hypo, long ld, const double *piv, long ld_piv, long n_mod,
                                                             long n_win, long slab_rows, const double *stats, double *part)
{
    __shared__ double tiles[kEllWG][kEllU * 192];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long grp = (long)blockIdx.x * kEllWG + wv, w = grp * 64 + lane;
    if (grp * 64 >= n_win) return;
    const bool live = w < n_win;
    const long c0 = grp * 192;
    const int n_live = (int)min(192L, 3 * n_win - c0);
    double mu[3], pm[NPIV > 0 ? NPIV : 1], acc[ell_nacc(NPIV)];
#pragma unroll
    for (int k = 0; k < 3; ++k) mu[k] = live ? stats[3 * w + k] : 0.0;
#pragma unroll
    for (int k = 0; k < NPIV; ++k) pm[k] = stats[3 * n_win + k];
#pragma unroll
    for (int a = 0; a < ell_nacc(NPIV); ++a) acc[a] = 0.0;
    const long row0 = (long)blockIdx.y * slab_rows, row1 = min(n_mod, row0 + slab_rows);
    double *tile = tiles[wv];
    long r = row0;
    for (; r + kEllU <= row1; r += kEllU) {
        double v[kEllU][3];
        ell_fetch<kEllU>(hypo + c0, ld, r, lane, n_live, tile, v);
        ell_add_rows<NPIV, kEllU>(v, mu, piv, ld_piv, r, pm, acc);
    }
    for (; r < row1; ++r) {
        double v[1][3];
        ell_fetch<1>(hypo + c0, ld, r, lane, n_live, tile, v);
        ell_add_rows<NPIV, 1>(v, mu, piv, ld_piv, r, pm, acc);
    }
    if (live) {
#pragma unroll
        for (int a = 0; a < ell_nacc(NPIV); ++a) part[((long)blockIdx.y * ell_nacc(NPIV) + a) * n_win + w] = acc[a];
    }
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix, r the third index: A <- J^T A J, V <- V J.  An
// off-diagonal element that is exactly 0 is left alone; nothing else depends on the data.  Plain products and sums (no fma):
// two equal rows then cancel exactly.
__host__ __device__ __forceinline__ void ell_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                                    double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0;
    v1p = a1; v1q = b1;
    v2p = a2; v2q = b2;
}

// swaps eigenpairs i and j (lam and column of V) when lam_i < lam_j
__host__ __device__ __forceinline__ void ell_order(double &li, double &lj, double &v0i, double &v0j, double &v1i, double &v1j,
                                                   double &v2i, double &v2j)
{
    if (li < lj) {
        double t;
        t = li; li = lj; lj = t;
        t = v0i; v0i = v0j; v0j = t;
        t = v1i; v1i = v1j; v1j = t;
        t = v2i; v2i = v2j; v2j = t;
    }
}

// the component of largest magnitude positive (the first of equal magnitudes decides)
__host__ __device__ __forceinline__ void ell_sign(double &v0, double &v1, double &v2)
{
    double big = v0;
    if (fabs(v1) > fabs(big)) big = v1;
    if (fabs(v2) > fabs(big)) big = v2;
    if (big < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
}

// cov = xx, xy, xz, yy, yz, zz; lam descending; V row-major, column k = unit axis k
__host__ __device__ __forceinline__ void ell_eigen(const double *cov, double *lam, double *V)
{
    double a00 = cov[0], a01 = cov[1], a02 = cov[2], a11 = cov[3], a12 = cov[4], a22 = cov[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kEllSweeps; ++sweep) {
        ell_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
        ell_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        ell_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    ell_order(a00, a11, v00, v01, v10, v11, v20, v21);
    ell_order(a11, a22, v01, v02, v11, v12, v21, v22);
    ell_order(a00, a11, v00, v01, v10, v11, v20, v21);
    ell_sign(v00, v10, v20);
    ell_sign(v01, v11, v21);
    ell_sign(v02, v12, v22);
    lam[0] = a00; lam[1] = a11; lam[2] = a22;
    V[0] = v00; V[1] = v01; V[2] = v02;
    V[3] = v10; V[4] = v11; V[5] = v12;
    V[6] = v20; V[7] = v21; V[8] = v22;
}

// one lane per item (sum a of window w: item a n_win + w); part [n_slab][n_items] -> sum [n_items], the slabs in ascending order
__global__ __launch_bounds__(64) void k_ell_slabs(const double *part, long n_items, int n_slab, double *sum)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_items) return;
    double s = part[i];
    for (int g = 1; g < n_slab; ++g) s += part[(long)g * n_items + i];
    sum[i] = s;
}

// one lane per window; mom [ell_nacc(n_piv)][n_win] as k_ell_slabs wrote it; out [n_win][kEllOut] but for q;
// piv_corr [n_win][3][n_piv]
__global__ __launch_bounds__(64) void k_ell_finish(const double *mom, const double *stats, long n_mod, long n_win, int n_piv,
                                                   double *out, double *piv_corr)
{
    const long w = (long)blockIdx.x * 64 + threadIdx.x;
    if (w >= n_win) return;
    const long n_col = 3 * n_win + n_piv;
    auto msum = [&](int a) { return mom[(long)a * n_win + w]; };
    const double dn = (double)(n_mod - 1);
    double *o = out + w * kEllOut;
    bool cst[3];
    bool degenerate = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = stats[3 * w + k];
        cst[k] = stats[n_col + 3 * w + k] == stats[2 * n_col + 3 * w + k];
        degenerate |= cst[k];
    }
    double m[6], cov[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        m[a] = msum(a);
        cov[a] = m[a] / dn;
        o[3 + a] = cov[a];
    }
    double lam[3], V[9];
    ell_eigen(cov, lam, V);
    degenerate |= !(lam[2] > 0.0);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[9 + k] = degenerate ? NAN : lam[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) o[12 + k] = degenerate ? NAN : V[k];
    const double maa[3] = {m[0], m[3], m[5]};
    for (int k = 0; k < n_piv; ++k) {
        const double mkk = msum(6 + 3 * n_piv + k);
        const bool pc = stats[n_col + 3 * n_win + k] == stats[2 * n_col + 3 * n_win + k];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double mak = msum(6 + 3 * k + a);
            piv_corr[(w * 3 + a) * n_piv + k] = pc || cst[a] ? NAN : mak / (sqrt(maa[a]) * sqrt(mkk));
        }
    }
}

// grid = (window groups of the batch / kEllWG, row slabs); windows w0 .. w0 + nb - 1 (w0 a multiple of 64);
// d2 [n_mod][ld_d2], column j = window w0 + j: sum_k ((x - mean) . v_k)^2 / lambda_k.  A degenerate window (NaN axes) is left
// out: its column is set to 0 and its q to NaN (k_ell_setq).
__global__ __launch_bounds__(64 * kEllWG) void k_ell_maha(const double *hypo, long ld, long n_mod, long n_win, long w0, long nb,
                                                          long slab_rows, const double *out, double *d2, long ld_d2)
{
    __shared__ double tiles[kEllWG][kEllU * 192];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long grp = (long)blockIdx.x * kEllWG + wv, j = grp * 64 + lane, w = w0 + j;
    if (grp * 64 >= nb) return;
    const bool live = j < nb;
    const long c0 = 3 * (w0 + grp * 64);
    const int n_live = (int)min(192L, 3 * n_win - c0);
    double mu[3] = {0.0, 0.0, 0.0}, lam[3] = {1.0, 1.0, 1.0}, V[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool degenerate = true;
    if (live) {
        const double *o = out + w * kEllOut;
        degenerate = isnan(o[9]);
        if (!degenerate) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { mu[k] = o[k]; lam[k] = o[9 + k]; }
#pragma unroll
            for (int k = 0; k < 9; ++k) V[k] = o[12 + k];
        }
    }
    auto dist = [&](const double (&x)[3]) {
        const double dx = x[0] - mu[0], dy = x[1] - mu[1], dz = x[2] - mu[2];
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p = dx * V[k] + dy * V[3 + k] + dz * V[6 + k];
            d += p * p / lam[k];
        }
        return d;
    };
    const long row0 = (long)blockIdx.y * slab_rows, row1 = min(n_mod, row0 + slab_rows);
    double *tile = tiles[wv];
    long r = row0;
    for (; r + kEllU <= row1; r += kEllU) {
        double v[kEllU][3];
        ell_fetch<kEllU>(hypo + c0, ld, r, lane, n_live, tile, v);
        if (live) {
#pragma unroll
            for (int u = 0; u < kEllU; ++u) d2[(r + u) * ld_d2 + j] = degenerate ? 0.0 : dist(v[u]);
        }
    }
    for (; r < row1; ++r) {
        double v[1][3];
        ell_fetch<1>(hypo + c0, ld, r, lane, n_live, tile, v);
        if (live) d2[r * ld_d2 + j] = degenerate ? 0.0 : dist(v[0]);
    }
}

// q [nb][3] as htm_quantiles_dev wrote it (the same rank three times)
__global__ __launch_bounds__(64) void k_ell_setq(const double *q, long w0, long nb, double *out)
{
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= nb) return;
    double *o = out + (w0 + j) * kEllOut;
    o[21] = isnan(o[9]) ? NAN : q[3 * j];
}

}  // namespace htm
