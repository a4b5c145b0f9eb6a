// htm_steps.hip -- the C ABI (include/htm_hip.h) of the pipeline's other steps: step 1 (htm_fft*, htm_convert*), steps 2 and 3
// (htm_xcorr*, htm_measure_windows), step 4 (htm_select_regress), the convergence diagnostics (htm_diagnose*, htm_rank_normalize*), step 6
// (htm_quantiles*), the error ellipsoids (htm_hypo_ellipsoid*), the density maps (htm_hypo_density*).  None touches a forward or a chain set; host idioms: htm_steps_host.hpp.
#include "htm_steps_host.hpp"

#include <dlfcn.h>

#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "htm_convert.hpp"
#include "htm_density.hpp"
#include "htm_diag.hpp"
#include "htm_ellipsoid.hpp"
#include "htm_rank.hpp"
#include "htm_select.hpp"
#include "htm_xcorr.hpp"

using namespace htm;

namespace {
// what both forms of the select refuse before any device call
int select_check(const void *samples, const void *out, long n_mod, long n_par, long ld, const int *ranks_1based)
{
    if (!samples || !out || !ranks_1based) return fail(HTM_EINVAL, "NULL argument");
    if (n_mod < 1 || n_par < 1 || ld < n_par) return fail(HTM_EINVAL, "bad shape (n_mod %ld, n_par %ld, ld %ld)", n_mod, n_par, ld);
    // the select kernels count rows in int (LDS counters, the slab histogram's atomics) and take int ranks
    if (n_mod > INT_MAX) return fail(HTM_EINVAL, "n_mod %ld exceeds %d rows per column", n_mod, INT_MAX);
    for (int r = 0; r < 3; ++r)
        if (ranks_1based[r] < 1 || ranks_1based[r] > n_mod)
            return fail(HTM_EINVAL, "rank %d outside 1..%ld (the reference would index outside its sorted column)", ranks_1based[r], n_mod);
    return HTM_OK;
}
}  // namespace

extern "C" {

int htm_quantiles_dev(int device, const double *d_samples, long n_mod, long n_par, long ld, const int ranks_1based[3],
                      double *d_out, void *hip_stream)
{
    int rc = select_check(d_samples, d_out, n_mod, n_par, ld, ranks_1based);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    const dim3 grid((unsigned)((n_par + 63) / 64)), block(64 * kSelRG);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const char *force = getenv("HTM_SELECT_SLABS");
    // small sets: one launch, a column group per workgroup; large sets: row slabs over the whole chip, a launch per digit
    long slabs = 1;
    if ((double)n_mod * (double)n_par >= (double)(1 << 22)) {
        slabs = std::max(1L, std::min((n_mod + 255) / 256, (long)(2048 / grid.x)));
        slabs = std::min(slabs, 1024L);
    }
    if (force) slabs = std::max(1L, std::min(atol(force), std::min(n_mod, 65535L)));
    if (slabs <= 1 && !force) {
        hipLaunchKernelGGL(k_select, grid, block, 0, st, d_samples, n_mod, n_par, ld,
                           ranks_1based[0] - 1, ranks_1based[1] - 1, ranks_1based[2] - 1, d_out);
        HIPCHK(hipGetLastError());
        return HTM_OK;
    }
    // workspace: three histograms, two prefix/remaining states (stream-ordered allocation keeps the call asynchronous)
    const size_t hist_n = (size_t)grid.x * kSelHistPerGroup, st_n = (size_t)n_par * kSelRanks;
    StreamBuf ws;
    SelWork w;
    if ((rc = ws.alloc(st, [&](StreamBuf &b) {
            for (int k = 0; k < 3; ++k) b.take(w.hist[k], hist_n);
            for (int k = 0; k < 2; ++k) {
                b.take(w.prefix[k], st_n);
                b.take(w.remaining[k], st_n);
            }
        }))) return rc;
    HIPCHK(hipMemsetAsync(ws.data(), 0, ws.bytes(), st));
    const long slab_rows = (n_mod + slabs - 1) / slabs;
    const dim3 grid2(grid.x, (unsigned)slabs);
    int pass = 0;
    for (int shift = 60; shift >= 0; shift -= 4, ++pass)
        hipLaunchKernelGGL(k_select_pass, grid2, block, 0, st, d_samples, n_mod, n_par, ld, ranks_1based[0] - 1,
                           ranks_1based[1] - 1, ranks_1based[2] - 1, shift, pass, slab_rows, w, (double *)nullptr);
    hipLaunchKernelGGL(k_select_pass, grid, block, 0, st, d_samples, n_mod, n_par, ld, ranks_1based[0] - 1,
                       ranks_1based[1] - 1, ranks_1based[2] - 1, -4, pass, slab_rows, w, d_out);
    HIPCHK(hipGetLastError());
    return ws.release();
}

int htm_quantiles(int device, const double *samples, long n_mod, long n_par, const int ranks_1based[3], double *out)
{
    int rc = select_check(samples, out, n_mod, n_par, n_par, ranks_1based);      // the ranks too: not after the upload
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevPool pool;
    double *d_x = nullptr, *d_o = nullptr;
    if ((rc = pool.upload(&d_x, samples, (size_t)n_mod * n_par)) || (rc = pool.alloc(&d_o, (size_t)n_par * 3))) return rc;
    if ((rc = htm_quantiles_dev(device, d_x, n_mod, n_par, n_par, ranks_1based, d_o, nullptr))) return rc;
    return pool.download(out, d_o, (size_t)n_par * 3, "the select kernels or their");
}

// ---- convergence diagnostics (htm_diag.hpp) ---------------------------------------------------------------------
namespace {
// shapes both forms refuse before any device call
int diag_check(long n_seq, long n_draws, long n_par, int max_lag)
{
    if (n_draws < 4 || n_seq < 1 || n_par < 1 || max_lag < 1)
        return fail(HTM_EINVAL, "bad shape (n_seq %ld, n_draws %ld, n_par %ld, max_lag %d): need n_draws >= 4, the others >= 1",
                    n_seq, n_draws, n_par, max_lag);
    if (n_seq > INT_MAX / n_draws) return fail(HTM_EINVAL, "n_seq * n_draws = %ld * %ld exceeds %d rows", n_seq, n_draws, INT_MAX);
    return HTM_OK;
}
}  // namespace

int htm_diagnose_dev(int device, const double *d_samples, long n_seq, long n_draws, long n_par, long ld, int max_lag,
                     double *d_out, double *d_acov, void *hip_stream)
{
    if (!d_samples || !d_out) return fail(HTM_EINVAL, "NULL argument");
    int rc = diag_check(n_seq, n_draws, n_par, max_lag);
    if (rc) return rc;
    if (ld < n_par) return fail(HTM_EINVAL, "bad shape (n_par %ld, ld %ld)", n_par, ld);
    const long n = n_draws / 2, S = 2 * n_seq;
    const int L = (int)std::min(n - 1, (long)max_lag);
    // lags per thread: HTM_DIAG_LAGS=16|32 picks the other instantiation (tests, tools/bench_diagnose.py)
    int kb = 32;
    if (const char *e = getenv("HTM_DIAG_LAGS")) {
        kb = atoi(e);
        if (kb != 16 && kb != 32) return fail(HTM_EINVAL, "HTM_DIAG_LAGS = %s: 16 or 32", e);
    }
    const long n_cg = (n_par + 63) / 64, n_blk = L / kb + 1, n_lagwg = (n_blk + kDiagLW - 1) / kDiagLW;
    if (n_cg > INT_MAX / S || n_cg > INT_MAX / n_lagwg)
        return fail(HTM_EINVAL, "n_par %ld, %ld split sequences, %d lags need more than 2^32 - 1 work-items in one launch", n_par, S, L + 1);
    // slabs of split sequences: waves enough to fill the chip many times over, so that the last round of workgroups costs
    // little; a workspace of at most 256 MiB or half the samples' size
    long slabs = std::min(S, (65536 + n_cg * n_blk - 1) / (n_cg * n_blk));
    const double lag_bytes = (double)(L + 1) * (double)n_par * sizeof(double);
    const double ws_cap = std::max((double)(256L << 20), (double)(n_seq * n_draws) * (double)n_par * sizeof(double) / 2);
    slabs = std::max(1L, std::min(slabs, (long)(ws_cap / lag_bytes)));
    if (const char *e = getenv("HTM_DIAG_SLABS")) slabs = std::max(1L, std::min(atol(e), S));
    const long seq_per_slab = (S + slabs - 1) / slabs;
    slabs = (S + seq_per_slab - 1) / seq_per_slab;          // no empty slab
    if (n_cg * n_lagwg > INT_MAX / slabs || n_cg * S * 64 * kDiagRG > kMaxWorkItems || n_cg * n_lagwg * slabs * 64 * kDiagLW > kMaxWorkItems)
        return fail(HTM_EINVAL, "n_par %ld, %ld split sequences, %d lags need more than 2^32 - 1 work-items in one launch", n_par, S, L + 1);
    if ((rc = use_device(device))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // workspace: the means [S][n_par], the slabs' lag sums [slabs][L+1][n_par] (stream-ordered, as htm_quantiles_dev's)
    StreamBuf ws;
    double *d_mean = nullptr, *d_part = nullptr;
    if ((rc = ws.alloc(st, [&](StreamBuf &b) { b.take(d_mean, (size_t)S * n_par); b.take(d_part, (size_t)slabs * (L + 1) * n_par); }))) return rc;
    hipLaunchKernelGGL(k_diag_mean, dim3((unsigned)(n_cg * S)), dim3(64 * kDiagRG), 0, st, d_samples, n_draws, n, n_par, ld, n_cg, d_mean);
    const dim3 grid((unsigned)(n_cg * n_lagwg * slabs)), block(64 * kDiagLW);
    if (kb == 16)
        hipLaunchKernelGGL(k_diag_acov<16>, grid, block, 0, st, d_samples, n_draws, n, n_par, ld, L, (int)S, (int)seq_per_slab, n_lagwg, n_cg, d_mean, d_part);
    else
        hipLaunchKernelGGL(k_diag_acov<32>, grid, block, 0, st, d_samples, n_draws, n, n_par, ld, L, (int)S, (int)seq_per_slab, n_lagwg, n_cg, d_mean, d_part);
    hipLaunchKernelGGL(k_diag_finish, dim3((unsigned)n_cg), dim3(64), 0, st, d_part, d_mean, n, n_par, L, (int)S, (int)slabs,
                       1.0 / std::log10((double)S * (double)n), d_out, d_acov);
    HIPCHK(hipGetLastError());
    return ws.release();
}

int htm_diagnose(int device, const double *samples, long n_seq, long n_draws, long n_par, int max_lag, double *out, double *acov)
{
    if (!samples || !out) return fail(HTM_EINVAL, "NULL argument");
    int rc = diag_check(n_seq, n_draws, n_par, max_lag);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    const long L = std::min(n_draws / 2 - 1, (long)max_lag);
    const size_t on = (size_t)n_par * 4, an = (size_t)(L + 1) * n_par;
    DevPool pool;
    double *d_x = nullptr, *d_o = nullptr, *d_a = nullptr;
    if ((rc = pool.upload(&d_x, samples, (size_t)n_seq * n_draws * n_par)) || (rc = pool.alloc(&d_o, on)) || (acov && (rc = pool.alloc(&d_a, an))))
        return rc;
    if ((rc = htm_diagnose_dev(device, d_x, n_seq, n_draws, n_par, n_par, max_lag, d_o, d_a, nullptr))) return rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(HTM_EHIP, "the diagnostics kernels failed");
    if ((rc = pool.download(out, d_o, on, "the diagnostics'")) || (acov && (rc = pool.download(acov, d_a, an, "the autocovariances'")))) return rc;
    return HTM_OK;
}

// ---- rank-normalised diagnostics (htm_rank.hpp) ---------------------------------------------------
namespace {
// columns per batch: the two key buffers [nb][R] stay under HTM_RANK_MB MiB (default 2048; at least one column), and no
// launch of a batch goes beyond 2^32 - 1 work-items
int rank_batch(long R, long n_par, long *nb_out)
{
    double mb;
    if (int rc = env_mib("HTM_RANK_MB", 2048.0, &mb)) return rc;
    const double cols = mb * 1048576.0 / (2.0 * sizeof(unsigned long long) * (double)R);
    long nb = cols >= (double)n_par ? n_par : std::max(1L, (long)cols);
    nb = std::min(nb, 1L << 21);                           // k_rank_sort: nb workgroups of kRankTile = 1024 threads
    const long n_rt = (R + 63) / 64, n_cg = (nb + 63) / 64, n_rc = (R + kRankZRows - 1) / kRankZRows;
    if (n_rt * n_cg * 256 > kMaxWorkItems || n_cg * n_rc * 256 > kMaxWorkItems)
        return fail(HTM_EINVAL, "%ld rows x %ld columns per batch need more than 2^32 - 1 work-items in one launch", R, nb);
    *nb_out = nb;
    return HTM_OK;
}

int rank_shape_check(long n_rows, long n_par, long ld, long ld_z)
{
    if (n_rows < 2 || n_par < 1 || ld < n_par || ld_z < n_par)
        return fail(HTM_EINVAL, "bad shape (n_rows %ld, n_par %ld, ld %ld, ld_z %ld): need n_rows >= 2, n_par >= 1, ld and ld_z >= n_par",
                    n_rows, n_par, ld, ld_z);
    if (n_rows > INT_MAX) return fail(HTM_EINVAL, "n_rows %ld exceeds %d rows per column", n_rows, INT_MAX);
    return HTM_OK;
}

// d_med [n_par]: the medians of a folded transform, NULL for the plain one.  HTM_RANK_STOP=keys|sort ends every batch after
// that kernel (tools/bench_diagnose_rank.py times the three parts by it; z is then not written).
int rank_normalize_batches(const double *d_x, long R, long n_par, long ld, const double *d_med, double *d_z, long ld_z,
                           double *d_ranks, long nb, hipStream_t st)
{
    int stop = 3;
    if (const char *e = getenv("HTM_RANK_STOP")) stop = !strcmp(e, "keys") ? 1 : !strcmp(e, "sort") ? 2 : 3;
    StreamBuf ws;
    unsigned long long *ka = nullptr, *kb = nullptr;
    if (int rc = ws.alloc(st, [&](StreamBuf &b) { b.take(ka, (size_t)nb * R); b.take(kb, (size_t)nb * R); })) return rc;
    const long n_rt = (R + 63) / 64, n_rc = (R + kRankZRows - 1) / kRankZRows;
    for (long c0 = 0; c0 < n_par; c0 += nb) {
        const long n = std::min(nb, n_par - c0), n_cg = (n + 63) / 64;
        hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)(n_rt * n_cg)), dim3(256), 0, st, d_x, R, ld, c0, n, n_rt, d_med, ka);
        if (stop >= 2) hipLaunchKernelGGL(k_rank_sort, dim3((unsigned)n), dim3(kRankTile), 0, st, ka, kb, R);
        if (stop >= 3)
            hipLaunchKernelGGL(k_rank_z, dim3((unsigned)(n_cg * n_rc)), dim3(256), 0, st, d_x, R, ld, c0, n, n_cg, d_med,
                               (const unsigned long long *)ka, d_z, d_ranks, ld_z);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HTM_EHIP, "a rank kernel's launch failed: %s", hipGetErrorString(e));
    return ws.release();
}
}  // namespace

int htm_rank_normalize_dev(int device, const double *d_samples, long n_rows, long n_par, long ld, int fold, double *d_z, long ld_z,
                           double *d_ranks, void *hip_stream)
{
    if (!d_samples || !d_z) return fail(HTM_EINVAL, "NULL argument");
    int rc = rank_shape_check(n_rows, n_par, ld, ld_z);
    if (rc) return rc;
    long nb = 0;
    if ((rc = rank_batch(n_rows, n_par, &nb))) return rc;
    if ((rc = use_device(device))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!fold) return rank_normalize_batches(d_samples, n_rows, n_par, ld, nullptr, d_z, ld_z, d_ranks, nb, st);
    // the medians: the order statistics (R+1)/2 and R/2+1 (the third rank is not used)
    StreamBuf ws;
    double *d_q = nullptr, *d_med = nullptr;
    if ((rc = ws.alloc(st, [&](StreamBuf &b) { b.take(d_q, 3 * (size_t)n_par); b.take(d_med, (size_t)n_par); }))) return rc;
    const int rk[3] = {(int)((n_rows + 1) / 2), (int)(n_rows / 2 + 1), 1};
    if ((rc = htm_quantiles_dev(device, d_samples, n_rows, n_par, ld, rk, d_q, hip_stream))) return rc;
    hipLaunchKernelGGL(k_rank_median, dim3((unsigned)((n_par + 63) / 64)), dim3(64), 0, st, (const double *)d_q, n_par, d_med);
    if ((rc = rank_normalize_batches(d_samples, n_rows, n_par, ld, d_med, d_z, ld_z, d_ranks, nb, st))) return rc;
    return ws.release();
}

int htm_rank_normalize(int device, const double *samples, long n_rows, long n_par, int fold, double *z, double *ranks)
{
    if (!samples || !z) return fail(HTM_EINVAL, "NULL argument");
    int rc = rank_shape_check(n_rows, n_par, n_par, n_par);
    if (rc) return rc;
    long nb = 0;
    if ((rc = rank_batch(n_rows, n_par, &nb))) return rc;
    if ((rc = use_device(device))) return rc;
    const size_t n = (size_t)n_rows * n_par;
    DevPool pool;
    double *d_x = nullptr, *d_z = nullptr, *d_r = nullptr;
    if ((rc = pool.upload(&d_x, samples, n)) || (rc = pool.alloc(&d_z, n)) || (ranks && (rc = pool.alloc(&d_r, n))))
        return rc;
    if ((rc = htm_rank_normalize_dev(device, d_x, n_rows, n_par, n_par, fold, d_z, n_par, d_r, nullptr))) return rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(HTM_EHIP, "the rank kernels failed");
    if ((rc = pool.download(z, d_z, n, "the z scores'")) || (ranks && (rc = pool.download(ranks, d_r, n, "the ranks'")))) return rc;
    return HTM_OK;
}

int htm_diagnose_rank_dev(int device, const double *d_samples, long n_seq, long n_draws, long n_par, long ld, int max_lag, double *d_out,
                          void *hip_stream)
{
    if (!d_samples || !d_out) return fail(HTM_EINVAL, "NULL argument");
    int rc = diag_check(n_seq, n_draws, n_par, max_lag);
    if (rc) return rc;
    if (ld < n_par) return fail(HTM_EINVAL, "bad shape (n_par %ld, ld %ld)", n_par, ld);
    const long R = n_seq * n_draws, n_cg = (n_par + 63) / 64, n_rc = (R + kRankZRows - 1) / kRankZRows;
    // the launches of this function's own kernels and the widest one of htm_diagnose_dev (k_diag_mean), before any device call
    if (n_cg > INT_MAX / (2 * n_seq) || n_cg * 2 * n_seq * 64 * kDiagRG > kMaxWorkItems || n_cg * n_rc * 256 > kMaxWorkItems)
        return fail(HTM_EINVAL, "n_par %ld, %ld rows in %ld sequences need more than 2^32 - 1 work-items in one launch", n_par, R, n_seq);
    long nb = 0;
    if ((rc = rank_batch(R, n_par, &nb))) return rc;
    if ((rc = use_device(device))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // workspace: one [R][n_par] matrix that holds z, zf, I05 and I95 in turn; the six order statistics, the three thresholds and
    // the four results of htm_diagnose_dev per column
    StreamBuf ws;
    double *d_m = nullptr, *d_qa = nullptr, *d_qb = nullptr, *d_thr = nullptr, *d_d = nullptr;
    if ((rc = ws.alloc(st, [&](StreamBuf &b) {
            b.take(d_m, (size_t)R * n_par);
            b.take(d_qa, 3 * (size_t)n_par);
            b.take(d_qb, 3 * (size_t)n_par);
            b.take(d_thr, 3 * (size_t)n_par);
            b.take(d_d, 16 * (size_t)n_par);
        }))) return rc;
    // h = (R - 1) p, k = floor(h), g = h - k; the quantile is x_(k+1) + g (x_(min(k+2, R)) - x_(k+1))
    const double h05 = (double)(R - 1) * 0.05, h95 = (double)(R - 1) * 0.95;
    const long k05 = (long)std::floor(h05), k95 = (long)std::floor(h95);
    const int ra[3] = {(int)((R + 1) / 2), (int)(R / 2 + 1), (int)(k05 + 1)};
    const int rb[3] = {(int)std::min(k05 + 2, R), (int)(k95 + 1), (int)std::min(k95 + 2, R)};
    if ((rc = htm_quantiles_dev(device, d_samples, R, n_par, ld, ra, d_qa, hip_stream))) return rc;
    if ((rc = htm_quantiles_dev(device, d_samples, R, n_par, ld, rb, d_qb, hip_stream))) return rc;
    hipLaunchKernelGGL(k_rank_thresholds, dim3((unsigned)n_cg), dim3(64), 0, st, (const double *)d_qa, (const double *)d_qb, n_par,
                       h05 - (double)k05, h95 - (double)k95, d_thr);
    for (int part = 0; part < 4; ++part) {
        if (part < 2) {
            rc = rank_normalize_batches(d_samples, R, n_par, ld, part ? d_thr : nullptr, d_m, n_par, nullptr, nb, st);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(k_rank_indicator, dim3((unsigned)(n_cg * n_rc)), dim3(256), 0, st, d_samples, R, n_par, ld, n_cg,
                               (const double *)(d_thr + (part - 1) * n_par), part - 2, d_m);
        }
        if ((rc = htm_diagnose_dev(device, d_m, n_seq, n_draws, n_par, n_par, max_lag, d_d + (size_t)part * n_par * 4, nullptr, hip_stream)))
            return rc;
    }
    hipLaunchKernelGGL(k_rank_combine, dim3((unsigned)n_cg), dim3(64), 0, st, (const double *)d_d, n_par, d_out);
    if (hipGetLastError() != hipSuccess) return fail(HTM_EHIP, "a rank kernel's launch failed");
    return ws.release();
}

int htm_diagnose_rank(int device, const double *samples, long n_seq, long n_draws, long n_par, int max_lag, double *out)
{
    if (!samples || !out) return fail(HTM_EINVAL, "NULL argument");
    int rc = diag_check(n_seq, n_draws, n_par, max_lag);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevPool pool;
    double *d_x = nullptr, *d_o = nullptr;
    if ((rc = pool.upload(&d_x, samples, (size_t)n_seq * n_draws * n_par)) || (rc = pool.alloc(&d_o, (size_t)n_par * 4)))
        return rc;
    if ((rc = htm_diagnose_rank_dev(device, d_x, n_seq, n_draws, n_par, n_par, max_lag, d_o, nullptr))) return rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(HTM_EHIP, "the diagnostics kernels failed");
    return pool.download(out, d_o, (size_t)n_par * 4, "the rank diagnostics'");
}

// ---- location error ellipsoids (htm_ellipsoid.hpp) ----------------------------------------------------
namespace {
struct EllPlan { long slabs, slab_rows, nb; };

// what both forms refuse before any device call, and the launch plan: row slabs of the streaming kernels, windows per batch
int ell_plan(const double *hypo, const double *pivots, long n_mod, long n_win, int n_piv, long rank, long ld, long ld_piv,
             const double *out, const double *piv_corr, EllPlan *p)
{
    if (!hypo || !out || (n_piv > 0 && (!pivots || !piv_corr))) return fail(HTM_EINVAL, "NULL argument");
    if (n_mod < 4 || n_win < 1 || n_piv < 0 || n_piv > kEllMaxPiv)
        return fail(HTM_EINVAL, "bad shape (n_mod %ld, n_win %ld, n_piv %d): need n_mod >= 4, n_win >= 1, 0 <= n_piv <= %d", n_mod, n_win,
                    n_piv, kEllMaxPiv);
    // htm_quantiles_dev counts rows in int and takes int ranks
    if (n_mod > INT_MAX) return fail(HTM_EINVAL, "n_mod %ld exceeds %d rows per column", n_mod, INT_MAX);
    if (rank < 1 || rank > n_mod) return fail(HTM_EINVAL, "rank %ld outside 1..%ld", rank, n_mod);
    if (n_win > INT_MAX / 3) return fail(HTM_EINVAL, "n_win %ld needs more than 2^32 - 1 work-items in one launch", n_win);
    if (ld < 3 * n_win || ld_piv < n_piv)
        return fail(HTM_EINVAL, "bad row stride (ld %ld < 3 n_win = %ld or ld_piv %ld < n_piv = %d)", ld, 3 * n_win, ld_piv, n_piv);
    double mb;
    if (int rc = env_mib("HTM_ELLIPSOID_MB", 1024.0, &mb)) return rc;
    // windows per batch: d2 [n_mod][nb] under the cap, a multiple of 64 and at least one wave's 64
    const long n_grp = (n_win + 63) / 64;
    const double cap = mb * 1048576.0 / (sizeof(double) * (double)n_mod) / 64.0;
    p->nb = 64 * (cap >= (double)n_grp ? n_grp : std::max(1L, (long)cap));
    // row slabs: waves enough to fill the chip several times over, of at least 256 rows; HTM_ELL_SLABS forces the count
    long slabs = std::max(1L, std::min((4096 + n_grp - 1) / n_grp, (n_mod + 255) / 256));
    if (const char *e = getenv("HTM_ELL_SLABS")) slabs = std::max(1L, std::min(atol(e), n_mod));
    slabs = std::min(slabs, 65535L);
    p->slab_rows = (n_mod + slabs - 1) / slabs;
    p->slabs = (n_mod + p->slab_rows - 1) / p->slab_rows;          // no empty slab
    const long n_cg = (3 * n_win + 63) / 64 + (n_piv > 0), n_wg = (n_grp + kEllWG - 1) / kEllWG;
    if ((n_cg + kEllWG - 1) / kEllWG * p->slabs * 64 * kEllWG > kMaxWorkItems || n_wg * p->slabs * 64 * kEllWG > kMaxWorkItems)
        return fail(HTM_EINVAL, "n_win %ld in %ld row slabs needs more than 2^32 - 1 work-items in one launch", n_win, p->slabs);
    return HTM_OK;
}

}  // namespace

int htm_hypo_ellipsoid_dev(int device, const double *d_hypo, long ld, const double *d_pivots, long ld_piv, long n_mod, long n_win,
                           int n_piv, long rank_1based, double *d_out, double *d_piv_corr, void *hip_stream)
{
    EllPlan pl;
    int rc = ell_plan(d_hypo, d_pivots, n_mod, n_win, n_piv, rank_1based, ld, ld_piv, d_out, d_piv_corr, &pl);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const long n_col = 3 * n_win + n_piv, n_hcg = (3 * n_win + 63) / 64, n_cg = n_hcg + (n_piv > 0), n_grp = (n_win + 63) / 64;
    const int nacc = ell_nacc(n_piv), n_slab = (int)pl.slabs;
    // workspace (stream-ordered, as htm_quantiles_dev's): stats [3][n_col], the slabs' sum/min/max [slabs][3][n_col] and
    // residual sums [slabs][n_col], the slabs' moments [slabs][nacc][n_win] and their sums [nacc][n_win], d2 [n_mod][nb], its
    // order statistics [nb][3]
    const size_t sum_n = (size_t)nacc * n_win;
    StreamBuf ws;
    double *d_stats = nullptr, *d_rng = nullptr, *d_res = nullptr, *d_mom = nullptr, *d_sum = nullptr, *d_d2 = nullptr, *d_q = nullptr;
    if ((rc = ws.alloc(st, [&](StreamBuf &b) {
            b.take(d_stats, 3 * (size_t)n_col);
            b.take(d_rng, (size_t)pl.slabs * 3 * n_col);
            b.take(d_res, (size_t)pl.slabs * n_col);
            b.take(d_mom, (size_t)pl.slabs * sum_n);
            b.take(d_sum, sum_n);
            b.take(d_d2, (size_t)n_mod * pl.nb);
            b.take(d_q, 3 * (size_t)pl.nb);
        }))) return rc;
    // HTM_ELL_STOP=mean|moments|finish ends the call after that part (tools/bench_ellipsoid.py times the parts by it)
    int stop = 4;
    if (const char *e = getenv("HTM_ELL_STOP")) stop = !strcmp(e, "mean") ? 1 : !strcmp(e, "moments") ? 2 : !strcmp(e, "finish") ? 3 : 4;
    const EllCols cols{d_hypo, d_pivots, ld, ld_piv, 3 * n_win, n_hcg, n_piv};
    const dim3 grid_c((unsigned)((n_cg + kEllWG - 1) / kEllWG), (unsigned)pl.slabs), grid_w((unsigned)((n_grp + kEllWG - 1) / kEllWG), (unsigned)pl.slabs);
    hipLaunchKernelGGL(k_ell_range, grid_c, dim3(64 * kEllWG), 0, st, cols, n_mod, pl.slab_rows, d_rng);
    hipLaunchKernelGGL(k_ell_mean, grid_c, dim3(64 * kEllWG), 0, st, cols, n_mod, pl.slab_rows, (const double *)d_rng, n_slab, d_res);
    hipLaunchKernelGGL(k_ell_stats, dim3((unsigned)((n_col + 63) / 64)), dim3(64), 0, st, (const double *)d_rng, (const double *)d_res,
                       n_col, n_slab, n_mod, d_stats);
    if (stop >= 2) {
        auto moments = [&](auto npiv) {
            hipLaunchKernelGGL(k_ell_moments<decltype(npiv)::value>, grid_w, dim3(64 * kEllWG), 0, st, d_hypo, ld, d_pivots, ld_piv, n_mod,
                               n_win, pl.slab_rows, (const double *)d_stats, d_mom);
        };
        switch (n_piv) {
        case 0: moments(Int<0>()); break;
        case 1: moments(Int<1>()); break;
        case 2: moments(Int<2>()); break;
        case 3: moments(Int<3>()); break;
        default: moments(Int<4>()); break;
        }
    }
    if (stop >= 3) {
        hipLaunchKernelGGL(k_ell_slabs, dim3((unsigned)((sum_n + 63) / 64)), dim3(64), 0, st, (const double *)d_mom, (long)sum_n, n_slab, d_sum);
        hipLaunchKernelGGL(k_ell_finish, dim3((unsigned)n_grp), dim3(64), 0, st, (const double *)d_sum, (const double *)d_stats, n_mod, n_win,
                           n_piv, d_out, d_piv_corr);
    }
    if (hipGetLastError() != hipSuccess) return fail(HTM_EHIP, "an ellipsoid kernel's launch failed");
    const int rk[3] = {(int)rank_1based, (int)rank_1based, (int)rank_1based};
    for (long w0 = 0; stop >= 4 && w0 < n_win; w0 += pl.nb) {
        const long nb = std::min(pl.nb, n_win - w0), nb_grp = (nb + 63) / 64;
        hipLaunchKernelGGL(k_ell_maha, dim3((unsigned)((nb_grp + kEllWG - 1) / kEllWG), (unsigned)pl.slabs), dim3(64 * kEllWG), 0, st, d_hypo,
                           ld, n_mod, n_win, w0, nb, pl.slab_rows, (const double *)d_out, d_d2, pl.nb);
        if ((rc = htm_quantiles_dev(device, d_d2, n_mod, nb, pl.nb, rk, d_q, hip_stream))) return rc;
        hipLaunchKernelGGL(k_ell_setq, dim3((unsigned)nb_grp), dim3(64), 0, st, (const double *)d_q, w0, nb, d_out);
    }
    if (hipGetLastError() != hipSuccess) return fail(HTM_EHIP, "an ellipsoid kernel's launch failed");
    return ws.release();
}

int htm_hypo_ellipsoid(int device, const double *hypo, const double *pivots, long n_mod, long n_win, int n_piv, long rank_1based,
                       double *out, double *piv_corr)
{
    EllPlan pl;
    int rc = ell_plan(hypo, pivots, n_mod, n_win, n_piv, rank_1based, 3 * n_win, n_piv, out, piv_corr, &pl);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevPool pool;
    const size_t on = (size_t)n_win * kEllOut, cn = (size_t)n_win * 3 * n_piv;
    double *d_x = nullptr, *d_p = nullptr, *d_o = nullptr, *d_c = nullptr;
    if ((rc = pool.upload(&d_x, hypo, (size_t)n_mod * 3 * n_win)) || (rc = pool.alloc(&d_o, on)) ||
        (n_piv > 0 && ((rc = pool.upload(&d_p, pivots, (size_t)n_mod * n_piv)) || (rc = pool.alloc(&d_c, cn)))))
        return rc;
    if ((rc = htm_hypo_ellipsoid_dev(device, d_x, 3 * n_win, d_p, n_piv, n_mod, n_win, n_piv, rank_1based, d_o, d_c, nullptr))) return rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(HTM_EHIP, "the ellipsoid kernels failed");
    if ((rc = pool.download(out, d_o, on, "the ellipsoids'")) || (n_piv > 0 && (rc = pool.download(piv_corr, d_c, cn, "the pivot correlations'"))))
        return rc;
    return HTM_OK;
}

// ---- stacked density maps (htm_density.hpp) ------------------------------------------------------------
namespace {
struct DensPlan {
    MapGrid g;
    long slabs, slab_rows, nxy, nxz, nyz, nvol;      // nvol = 0 without the volume
    int path;                                         // 0 plain, 1 LDS, 2 naive
};

// what both forms refuse before any device call, and the launch plan: the grid, the counting path, the row slabs
int dens_plan(const double *hypo, long ld, long n_mod, long n_win, const int *layer, int n_layer, const double *grid9,
              const unsigned long long *xy, const unsigned long long *xz, const unsigned long long *yz, const unsigned long long *vol,
              const unsigned long long *tally, DensPlan *p)
{
    if (!hypo || !grid9 || !xy || !xz || !yz || !tally) return fail(HTM_EINVAL, "NULL argument");
    if (n_mod < 1 || n_win < 1 || n_layer < 1)
        return fail(HTM_EINVAL, "bad shape (n_mod %ld, n_win %ld, n_layer %d): need n_mod >= 1, n_win >= 1, n_layer >= 1", n_mod, n_win, n_layer);
    if (!layer && n_layer != 1) return fail(HTM_EINVAL, "n_layer %d without a layer per window: NULL puts every window in layer 0 of 1", n_layer);
    if (n_win > INT_MAX / 3) return fail(HTM_EINVAL, "n_win %ld needs more than 2^32 - 1 work-items in one launch", n_win);
    if (ld < 3 * n_win) return fail(HTM_EINVAL, "bad row stride (ld %ld < 3 n_win = %ld)", ld, 3 * n_win);
    if (int rc = map_grid_parse(grid9, &p->g)) return rc;
    p->nxy = (long)p->g.ny * p->g.nx;
    p->nxz = (long)p->g.nz * p->g.nx;
    p->nyz = (long)p->g.nz * p->g.ny;
    p->nvol = vol ? p->nxy * p->g.nz : 0;
    const long cells = p->nxy + p->nxz + p->nyz + p->nvol;
    if (cells > INT_MAX / n_layer)
        return fail(HTM_EINVAL, "%d layers of %ld cells: more than 2^31 - 1 counters", n_layer, cells);
    // the counting path: the LDS maps where a layer's three 2-D maps fit; HTM_DENSITY_LDS=0|1 forbids or forces them,
    // HTM_DENSITY_NAIVE=1 is the yardstick of tools/bench_density.py
    const bool fits = p->nxy + p->nxz + p->nyz <= kDensLdsCells;
    p->path = fits ? 1 : 0;
    if (const char *e = getenv("HTM_DENSITY_LDS")) {
        if (strcmp(e, "0") && strcmp(e, "1")) return fail(HTM_EINVAL, "HTM_DENSITY_LDS = %s: 0 or 1", e);
        p->path = e[0] == '1';
        if (p->path && !fits)
            return fail(HTM_EINVAL, "HTM_DENSITY_LDS = 1, but the grid's 2-D maps hold %ld cells: the LDS path takes %d", p->nxy + p->nxz + p->nyz,
                        kDensLdsCells);
    }
    if (const char *e = getenv("HTM_DENSITY_NAIVE"))
        if (!strcmp(e, "1")) p->path = 2;
    // row slabs: the plain kernel's as ell_plan's (4096 waves); the LDS kernel's workgroups each add their counters to the global
    // maps, so it takes as few as keep every CU busy (512 workgroups).  HTM_DENSITY_SLABS forces the count.  A slab is at most
    // kDensMaxSlabRows rows, whatever is forced.
    const long n_grp = (n_win + 63) / 64, n_wg = p->path == 1 ? n_grp : (n_grp + kDensWG - 1) / kDensWG;
    long slabs = std::max(1L, std::min(((p->path == 1 ? 512 : 4096) + n_grp - 1) / n_grp, (n_mod + 255) / 256));
    if (const char *e = getenv("HTM_DENSITY_SLABS")) slabs = std::max(1L, std::min(atol(e), n_mod));
    slabs = std::max(slabs, (n_mod + kDensMaxSlabRows - 1) / kDensMaxSlabRows);
    if (slabs > 65535L) {
        if ((n_mod + 65534L) / 65535L > kDensMaxSlabRows) return fail(HTM_EINVAL, "n_mod %ld needs more than 2^32 - 1 work-items in one launch", n_mod);
        slabs = 65535L;
    }
    p->slab_rows = (n_mod + slabs - 1) / slabs;
    p->slabs = (n_mod + p->slab_rows - 1) / p->slab_rows;          // no empty slab
    if (n_wg * p->slabs * 64 * kDensWG > kMaxWorkItems)
        return fail(HTM_EINVAL, "n_win %ld in %ld row slabs needs more than 2^32 - 1 work-items in one launch", n_win, p->slabs);
    return HTM_OK;
}

}  // namespace

int htm_hypo_density_dev(int device, const double *d_hypo, long ld, long n_mod, long n_win, const int *d_layer, int n_layer,
                         const double *grid9, unsigned long long *d_xy, unsigned long long *d_xz, unsigned long long *d_yz,
                         unsigned long long *d_vol, unsigned long long *d_tally, void *hip_stream)
{
    DensPlan pl;
    int rc = dens_plan(d_hypo, ld, n_mod, n_win, d_layer, n_layer, grid9, d_xy, d_xz, d_yz, d_vol, d_tally, &pl);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const size_t u = sizeof(unsigned long long);
    HIPCHK(hipMemsetAsync(d_xy, 0, (size_t)n_layer * pl.nxy * u, st));
    HIPCHK(hipMemsetAsync(d_xz, 0, (size_t)n_layer * pl.nxz * u, st));
    HIPCHK(hipMemsetAsync(d_yz, 0, (size_t)n_layer * pl.nyz * u, st));
    if (d_vol) HIPCHK(hipMemsetAsync(d_vol, 0, (size_t)n_layer * pl.nvol * u, st));
    HIPCHK(hipMemsetAsync(d_tally, 0, (size_t)n_layer * 2 * u, st));
    const long n_grp = (n_win + 63) / 64;
    const dim3 grid((unsigned)((n_grp + kDensWG - 1) / kDensWG), (unsigned)pl.slabs), grid_lds((unsigned)n_grp, (unsigned)pl.slabs), block(64 * kDensWG);
    const DensOut o{d_xy, d_xz, d_yz, d_vol, d_tally};
    if (pl.path == 1)
        hipLaunchKernelGGL(k_dens_lds, grid_lds, block, 0, st, d_hypo, ld, n_mod, n_win, pl.slab_rows, d_layer, n_layer, pl.g, o);
    else if (pl.path == 2)
        hipLaunchKernelGGL(k_dens_plain<true>, grid, block, 0, st, d_hypo, ld, n_mod, n_win, pl.slab_rows, d_layer, n_layer, pl.g, o);
    else
        hipLaunchKernelGGL(k_dens_plain<false>, grid, block, 0, st, d_hypo, ld, n_mod, n_win, pl.slab_rows, d_layer, n_layer, pl.g, o);
    if (hipGetLastError() != hipSuccess) return fail(HTM_EHIP, "the density kernel's launch failed");
    return HTM_OK;
}

int htm_hypo_density(int device, const double *hypo, long n_mod, long n_win, const int *layer, int n_layer, const double *grid9,
                     unsigned long long *xy, unsigned long long *xz, unsigned long long *yz, unsigned long long *vol,
                     unsigned long long *tally)
{
    DensPlan pl;
    int rc = dens_plan(hypo, 3 * n_win, n_mod, n_win, layer, n_layer, grid9, xy, xz, yz, vol, tally, &pl);
    if (rc) return rc;
    double mb;
    if ((rc = env_mib("HTM_DENSITY_MB", 1024.0, &mb))) return rc;
    if ((rc = use_device(device))) return rc;
    // the rows go to the device in batches under HTM_DENSITY_MB MiB (one row at the least); the batches' counts are added here
    const double cap = mb * 1048576.0 / (sizeof(double) * 3.0 * (double)n_win);
    const long rows = cap >= (double)n_mod ? n_mod : std::max(1L, (long)cap);
    const size_t on[5] = {(size_t)n_layer * pl.nxy, (size_t)n_layer * pl.nxz, (size_t)n_layer * pl.nyz, (size_t)n_layer * pl.nvol, (size_t)n_layer * 2};
    unsigned long long *host[5] = {xy, xz, yz, vol, tally}, *dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevPool pool;
    double *d_x = nullptr;
    int *d_l = nullptr;
    if ((rc = pool.alloc(&d_x, (size_t)rows * 3 * n_win)) || (layer && (rc = pool.upload(&d_l, layer, (size_t)n_win)))) return rc;
    for (int k = 0; k < 5; ++k)
        if (host[k] && (rc = pool.alloc(&dev[k], on[k]))) return rc;
    std::vector<unsigned long long> part;
    for (long r0 = 0; r0 < n_mod; r0 += rows) {
        const long nr = std::min(rows, n_mod - r0);
        HIPCHK(hipMemcpy(d_x, hypo + (size_t)r0 * 3 * n_win, (size_t)nr * 3 * n_win * sizeof(double), hipMemcpyHostToDevice));
        if ((rc = htm_hypo_density_dev(device, d_x, 3 * n_win, nr, n_win, d_l, n_layer, grid9, dev[0], dev[1], dev[2], dev[3], dev[4], nullptr)))
            return rc;
        if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(HTM_EHIP, "the density kernel failed");
        for (int k = 0; k < 5; ++k) {
            if (!host[k]) continue;
            if (r0 == 0) {
                if ((rc = pool.download(host[k], dev[k], on[k], "the density maps'"))) return rc;
                continue;
            }
            part.resize(on[k]);
            if ((rc = pool.download(part.data(), dev[k], on[k], "the density maps'"))) return rc;
            for (size_t i = 0; i < on[k]; ++i) host[k][i] += part[i];
        }
    }
    return HTM_OK;
}

int htm_select_regress(int device, int n_sta, int n_win, const double *sta_x, const double *sta_y, const double *sta_z,
                       double z_guess, const double *t, const double *t_err, const double *a, const double *a_err, double *out)
{
    if (!sta_x || !sta_y || !sta_z || !t || !t_err || !a || !a_err || !out) return fail(HTM_EINVAL, "NULL argument");
    if (n_sta < 3 || n_win < 1) return fail(HTM_EINVAL, "need n_sta >= 3 and n_win >= 1 (got %d, %d)", n_sta, n_win);
    // a wave per window, four per workgroup: the dispatch packet holds the grid in work-items as a uint32_t
    if (256L * ((n_win + 3L) / 4) > kMaxWorkItems)
        return fail(HTM_EINVAL, "n_win = %d windows need %ld work-items: more than one launch holds (2^32 - 1)", n_win,
                    256L * ((n_win + 3L) / 4));
    int rc = use_device(device);
    if (rc) return rc;
    DevPool pool;
    const size_t n = (size_t)n_sta * n_win;
    double *dx = nullptr, *dy = nullptr, *dz = nullptr, *dt = nullptr, *dte = nullptr, *da = nullptr, *dae = nullptr, *dout = nullptr;
    if ((rc = pool.upload(&dx, sta_x, n_sta)) || (rc = pool.upload(&dy, sta_y, n_sta)) || (rc = pool.upload(&dz, sta_z, n_sta)) ||
        (rc = pool.upload(&dt, t, n)) || (rc = pool.upload(&dte, t_err, n)) || (rc = pool.upload(&da, a, n)) ||
        (rc = pool.upload(&dae, a_err, n)) || (rc = pool.alloc(&dout, 6 * (size_t)n_win))) return rc;
    hipLaunchKernelGGL(k_regress, dim3((n_win + 3) / 4), dim3(256), 0, 0, n_sta, n_win, dx, dy, dz, z_guess, dt, dte, da, dae, dout);
    if (hipGetLastError() != hipSuccess) return fail(HTM_EHIP, "k_regress launch failed");
    return pool.download(out, dout, 6 * (size_t)n_win, "k_regress or its");
}

static int xcorr_check(long ld_env, long n_smp, int n_sta, int n, int n_step, int n_win, int pair0, int n_pairs, long ld_cc)
{
    if (n < 2 || n > kXcMaxN || n % 2) return fail(HTM_EINVAL, "window length n = %d: need an even n in 2..%d (the reference refuses odd n)", n, kXcMaxN);
    if (n_sta < 2 || n_step < 1 || n_win < 1 || n_pairs < 1 || pair0 < 0)
        return fail(HTM_EINVAL, "bad shape (n_sta %d, n_step %d, n_win %d, pair0 %d, n_pairs %d)", n_sta, n_step, n_win, pair0, n_pairs);
    if ((long)pair0 + n_pairs > (long)n_sta * (n_sta - 1) / 2)
        return fail(HTM_EINVAL, "pairs %d..%d outside the %d pairs of %d stations", pair0, pair0 + n_pairs - 1, n_sta * (n_sta - 1) / 2, n_sta);
    if ((long)(n_win - 1) * n_step + n > n_smp || n_smp > ld_env)
        return fail(HTM_EINVAL, "%d windows of %d samples every %d do not fit in %ld samples (row stride %ld)", n_win, n, n_step, n_smp, ld_env);
    if (ld_cc < n_pairs) return fail(HTM_EINVAL, "ld_cc %ld < n_pairs %d", ld_cc, n_pairs);
    if ((long)n_win * n_pairs > 0x7fffffffL) return fail(HTM_EINVAL, "n_win * n_pairs = %ld exceeds one launch", (long)n_win * n_pairs);
    // the dispatch packet holds the grid in work-items as a uint32_t (hsa_kernel_dispatch_packet_t::grid_size_x)
    if ((long)n_win * n_pairs * xc_threads(n) > kMaxWorkItems)
        return fail(HTM_EINVAL, "n_win * n_pairs * %d threads = %ld work-items exceed one launch (2^32 - 1)", xc_threads(n),
                    (long)n_win * n_pairs * xc_threads(n));
    return HTM_OK;
}

int htm_xcorr_dev(int device, const double *d_env, long ld_env, long n_smp, int n_sta, int n, int n_step, int n_win, int pair0,
                  int n_pairs, double *d_cc, long ld_cc, double *d_cc_max, void *hip_stream)
{
    if (!d_env || !d_cc || !d_cc_max) return fail(HTM_EINVAL, "NULL argument");
    int rc = xcorr_check(ld_env, n_smp, n_sta, n, n_step, n_win, pair0, n_pairs, ld_cc);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    const int threads = xc_threads(n);
    hipLaunchKernelGGL(k_xcorr, dim3((unsigned)((long)n_win * n_pairs)), dim3(threads), 2 * (size_t)n * sizeof(double),
                       static_cast<hipStream_t>(hip_stream), d_env, ld_env, n_sta, n, n_step, n_win, pair0, n_pairs, d_cc, ld_cc,
                       d_cc_max);
    HIPCHK(hipGetLastError());
    return HTM_OK;
}

int htm_xcorr(int device, const double *env, long n_smp, int n_sta, int n, int n_step, int n_win, int pair0, int n_pairs,
              double *cc, double *cc_max)
{
    if (!env || !cc || !cc_max) return fail(HTM_EINVAL, "NULL argument");
    int rc = xcorr_check(n_smp, n_smp, n_sta, n, n_step, n_win, pair0, n_pairs, n_pairs);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevPool pool;
    double *de = nullptr, *dc = nullptr, *dm = nullptr;
    const size_t n_cc = (size_t)n_win * n * n_pairs, n_m = (size_t)n_win * n_pairs;
    if ((rc = pool.upload(&de, env, (size_t)n_sta * n_smp)) || (rc = pool.alloc(&dc, n_cc)) || (rc = pool.alloc(&dm, n_m)))
        return rc;
    if ((rc = htm_xcorr_dev(device, de, n_smp, n_smp, n_sta, n, n_step, n_win, pair0, n_pairs, dc, n_pairs, dm, nullptr))) return rc;
    if ((rc = pool.download(cc, dc, n_cc, "k_xcorr or its")) || (rc = pool.download(cc_max, dm, n_m, "k_xcorr or its"))) return rc;
    return HTM_OK;
}

int htm_measure_windows(int device, int n_sta, int n, double dt, int n_det, const double *x, double *t, double *t_stdv,
                        double *amp, double *amp_stdv)
{
    if (!x || !t || !t_stdv || !amp || !amp_stdv) return fail(HTM_EINVAL, "NULL argument");
    if (n_sta < 3 || n < 2 || n > kXcMaxN || n_det < 0 || !(dt > 0.0))
        return fail(HTM_EINVAL, "need n_sta >= 3, n in 2..%d, n_det >= 0, dt > 0 (got %d, %d, %d, %g)", kXcMaxN, n_sta, n, n_det, dt);
    if (n_det == 0) return HTM_OK;
    int rc = use_device(device);
    if (rc) return rc;
    DevPool pool;
    // windows in launches of at most HTM_MEASURE_MB MiB of inputs and workspace (default 256: every window of a usual
    // run in one launch; at least one window per launch)
    const size_t per_win = ((size_t)n_sta * n + (size_t)n_sta * n_sta + 5 * (size_t)n_sta) * sizeof(double);
    const char *mb_env = getenv("HTM_MEASURE_MB");
    const double mb = mb_env ? atof(mb_env) : 256.0;
    const size_t budget = mb > 0.0 ? (size_t)std::min(mb * 1048576.0, 1e18) : 0;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_det, budget / per_win));
    double *dx = nullptr, *dws = nullptr, *dout = nullptr;
    if ((rc = pool.alloc(&dx, (size_t)chunk * n_sta * n)) || (rc = pool.alloc(&dws, (size_t)chunk * ((size_t)n_sta * n_sta + n_sta))) ||
        (rc = pool.alloc(&dout, 4 * (size_t)chunk * n_sta)))
        return rc;
    double *outs[4] = {t, t_stdv, amp, amp_stdv};
    for (int w0 = 0; w0 < n_det; w0 += chunk) {
        const int nw = std::min(chunk, n_det - w0);
        const size_t ns = (size_t)nw * n_sta;
        HIPCHK(hipMemcpy(dx, x + (size_t)w0 * n_sta * n, ns * n * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_measure, dim3(nw), dim3(xc_threads(n)), 2 * (size_t)n * sizeof(double), 0, dx, n_sta, n, dt, nw, dws,
                           dout, dout + (size_t)chunk * n_sta, dout + 2 * (size_t)chunk * n_sta, dout + 3 * (size_t)chunk * n_sta);
        if (hipGetLastError() != hipSuccess) return fail(HTM_EHIP, "k_measure launch failed");
        for (int k = 0; k < 4; ++k)
            if ((rc = pool.download(outs[k] + (size_t)w0 * n_sta, dout + k * (size_t)chunk * n_sta, ns, "k_measure or its"))) return rc;
    }
    return HTM_OK;
}

}  // extern "C"

// ---- step 1: FFT plans (htm_fft.hpp) and the convert pipeline (htm_convert.hpp) ---------------------------------------
namespace {

struct FftPlan {
    long n = 0;
    std::vector<int> radix;          // Stockham passes (empty for n = 1 and for Bluestein lengths)
    std::vector<long> tw_off;        // first twiddle of each pass in d_tw
    double2 *d_tw = nullptr;
    long m = 0;                      // Bluestein: inner power-of-two length (0: Stockham)
    const FftPlan *inner = nullptr;
    double2 *d_chirp = nullptr, *d_b = nullptr;
    FftPlan() = default;
    FftPlan(const FftPlan &) = delete; FftPlan &operator=(const FftPlan &) = delete;
    // only a plan whose build failed is destroyed: the plans in g_fft_plans are never deleted, on purpose (no hipFree at exit)
    ~FftPlan() { (void)hipFree(d_tw); (void)hipFree(d_chirp); (void)hipFree(d_b); }
};

std::mutex g_fft_mu;
std::map<std::pair<int, long>, FftPlan *> g_fft_plans;   // per (device, n); kept for the life of the process

bool fft_factor(long n, std::vector<int> &r)
{
    r.clear();
    while (n % 4 == 0) { r.push_back(4); n /= 4; }
    if (n % 2 == 0) { r.push_back(2); n /= 2; }
    for (int p : {3, 5, 7})
        while (n % p == 0) { r.push_back(p); n /= p; }
    return n == 1;
}

long fft_inner_len(long n)
{
    long m = 1;
    while (m < 2 * n - 1) m <<= 1;
    return m;
}

// complex elements of workspace fft_run needs for `rows` rows of n, and the most work-items one of its launches takes
size_t fft_ws_elems(long n, long rows)
{
    std::vector<int> r;
    return fft_factor(n, r) ? (size_t)rows * n : 2 * (size_t)rows * fft_inner_len(n);
}
long fft_max_items(long n, long rows)
{
    std::vector<int> r;
    return fft_factor(n, r) ? rows * n : rows * fft_inner_len(n);
}

dim3 fft_grid(long total) { return dim3((unsigned)((total + kFftThreads - 1) / kFftThreads)); }

int fft_run(const FftPlan &p, const double2 *in, long ld_in, double2 *out, long ld_out, long rows, int sign, double2 *ws,
            hipStream_t st)
{
    const long n = p.n;
    if (p.m == 0) {
        const int P = (int)p.radix.size();
        if (P == 0) {
            if (in != out) hipLaunchKernelGGL(k_fft_copy, fft_grid(rows * n), dim3(kFftThreads), 0, st, in, ld_in, out, ld_out, n, rows * n);
            HIPCHK(hipGetLastError());
            return HTM_OK;
        }
        // the last pass writes `out`; in place with an odd pass count the passes end in ws and a copy follows
        const bool extra = in == out && P % 2 == 1;
        const double2 *src = in;
        long lds = ld_in, ns = 1;
        for (int i = 0; i < P; ++i) {
            const bool to_out = extra ? (i % 2 == 1) : ((P - 1 - i) % 2 == 0);
            double2 *dst = to_out ? out : ws;
            const long ldd = to_out ? ld_out : n;
            const int R = p.radix[i];
            const long total = rows * (n / R);
            const double2 *tw = p.d_tw + p.tw_off[i];
            auto pass = [&](auto radix) {
                hipLaunchKernelGGL(k_fft_pass<decltype(radix)::value>, fft_grid(total), dim3(kFftThreads), 0, st, src, lds, dst, ldd, (int)n,
                                   (int)ns, tw, sign, total);
            };
            switch (R) {
            case 2: pass(Int<2>()); break;
            case 3: pass(Int<3>()); break;
            case 4: pass(Int<4>()); break;
            case 5: pass(Int<5>()); break;
            default: pass(Int<7>()); break;
            }
            src = dst; lds = ldd; ns *= R;
        }
        if (extra) hipLaunchKernelGGL(k_fft_copy, fft_grid(rows * n), dim3(kFftThreads), 0, st, ws, n, out, ld_out, n, rows * n);
        HIPCHK(hipGetLastError());
        return HTM_OK;
    }
    // Bluestein: backward(x) = conj(forward(conj(x))); ws holds a [rows][m] and the inner transforms' own rows * m
    const long m = p.m;
    double2 *a = ws, *ws2 = ws + (size_t)rows * m;
    hipLaunchKernelGGL(k_blue_pre, fft_grid(rows * m), dim3(kFftThreads), 0, st, in, ld_in, a, n, m, p.d_chirp, sign > 0 ? 1 : 0, rows * m);
    int rc = fft_run(*p.inner, a, m, a, m, rows, -1, ws2, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_blue_mul, fft_grid(rows * m), dim3(kFftThreads), 0, st, a, m, p.d_b, rows * m);
    if ((rc = fft_run(*p.inner, a, m, a, m, rows, +1, ws2, st))) return rc;
    hipLaunchKernelGGL(k_blue_post, fft_grid(rows * n), dim3(kFftThreads), 0, st, a, m, out, ld_out, n, p.d_chirp, sign > 0 ? 1 : 0, rows * n);
    HIPCHK(hipGetLastError());
    return HTM_OK;
}

const long double kPiL = 3.141592653589793238462643383279502884L;

// the plan of length n on the current device, built once (g_fft_mu held); tables in long double, rounded once
int fft_plan_locked(int device, long n, const FftPlan **out)
{
    auto it = g_fft_plans.find(std::make_pair(device, n));
    if (it != g_fft_plans.end()) { *out = it->second; return HTM_OK; }
    std::unique_ptr<FftPlan> p(new FftPlan);
    p->n = n;
    if (fft_factor(n, p->radix)) {
        // tw[off + k (R-1) + r - 1] = exp(-2 pi i r k / (ns R)), k < ns
        std::vector<double2> tw;
        long ns = 1;
        for (int R : p->radix) {
            p->tw_off.push_back((long)tw.size());
            for (long k = 0; k < ns; ++k)
                for (int r = 1; r < R; ++r) {
                    const long double a = -2.0L * kPiL * (long double)(r * k) / (long double)(ns * R);
                    tw.push_back(make_double2((double)cosl(a), (double)sinl(a)));
                }
            ns *= R;
        }
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&p->d_tw), std::max<size_t>(1, tw.size()) * sizeof(double2)));
        if (!tw.empty()) HIPCHK(hipMemcpy(p->d_tw, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice));
    } else {
        p->radix.clear();
        p->m = fft_inner_len(n);
        const long m = p->m;
        int rc = fft_plan_locked(device, m, &p->inner);
        if (rc) return rc;
        // chirp w[j] = exp(-pi i (j^2 mod 2n) / n); b = conj(w) at j and m - j, divided by m (a power of two: exact)
        std::vector<double2> w(n), b(m, make_double2(0.0, 0.0));
        for (long j = 0; j < n; ++j) {
            const long q = (long)(((unsigned long long)j * (unsigned long long)j) % (unsigned long long)(2 * n));
            const long double a = -kPiL * (long double)q / (long double)n;
            const long double c = cosl(a), s = sinl(a);
            w[j] = make_double2((double)c, (double)s);
            b[j] = make_double2((double)(c / m), (double)(-s / m));
            if (j) b[m - j] = b[j];
        }
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&p->d_chirp), n * sizeof(double2)));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&p->d_b), m * sizeof(double2)));
        HIPCHK(hipMemcpy(p->d_chirp, w.data(), n * sizeof(double2), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->d_b, b.data(), m * sizeof(double2), hipMemcpyHostToDevice));
        DevPool pool;
        double2 *tmp = nullptr;
        if ((rc = pool.alloc(&tmp, m))) return rc;
        rc = fft_run(*p->inner, p->d_b, m, p->d_b, m, 1, -1, tmp, nullptr);
        const hipError_t e = hipDeviceSynchronize();
        if (rc) return rc;
        if (e != hipSuccess) return fail(HTM_EHIP, "Bluestein table of n = %ld: %s", n, hipGetErrorString(e));
    }
    *out = p.get();
    g_fft_plans[std::make_pair(device, n)] = p.release();
    return HTM_OK;
}

int fft_plan(int device, long n, const FftPlan **out)
{
    std::lock_guard<std::mutex> lk(g_fft_mu);
    return fft_plan_locked(device, n, out);
}

int fft_check(const void *in, long ld_in, const void *out, long ld_out, long n, long batch, int direction)
{
    if (!in || !out) return fail(HTM_EINVAL, "NULL argument");
    if (n < 1 || n > kFftMaxN) return fail(HTM_EINVAL, "FFT length n = %ld outside 1..%ld", n, kFftMaxN);
    if (batch < 1 || ld_in < n || ld_out < n) return fail(HTM_EINVAL, "bad shape (batch %ld, ld_in %ld, ld_out %ld, n %ld)", batch, ld_in, ld_out, n);
    if (direction != -1 && direction != 1) return fail(HTM_EINVAL, "direction must be -1 (forward) or +1 (backward), got %d", direction);
    if (in == out && ld_in != ld_out) return fail(HTM_EINVAL, "in place needs ld_in == ld_out");
    if (fft_max_items(n, batch) > kMaxWorkItems)
        return fail(HTM_EINVAL, "%ld rows of n = %ld need %ld work-items in one launch (more than 2^32 - 1)", batch, n, fft_max_items(n, batch));
    return HTM_OK;
}

// step 1 geometry: index of the last segment, and the kept range [start, end) of stream samples of segment j
long cv_last(long n_total, int n) { return (n_total - n) / (n / 2) + 1; }
long cv_start(long j, int n) { return j == 0 ? 0 : j * (n / 2) + n / 4; }
long cv_end(long j, long n_total, int n) { return j == cv_last(n_total, n) ? n_total : j * (n / 2) + n - n / 4; }
long ceil_div(long a, long b) { return (a + b - 1) / b; }

int cv_check(long n_total, int n, int n_fac, int h, const int k_band[4], long j0, long j1)
{
    if (!k_band) return fail(HTM_EINVAL, "NULL argument");
    if (n < 4 || n % 4 || n > kFftMaxN) return fail(HTM_EINVAL, "n = %d: need a multiple of 4 in 4..%ld", n, kFftMaxN);
    if (n_total < n) return fail(HTM_EINVAL, "data length is not enough in queue (N = %ld < n = %d)", n_total, n);
    if (n_fac < 1 || n_fac > n / 2) return fail(HTM_EINVAL, "n_fac = %d: need 1 <= n_fac <= n/2 = %d", n_fac, n / 2);
    if (h < 0 || h > kCvMaxH || 2L * h > n) return fail(HTM_EINVAL, "half width h = %d: need 0 <= h <= %d and 2h <= n = %d", h, kCvMaxH, n);
    if (k_band[0] < 0 || k_band[0] > k_band[1] || k_band[1] > k_band[2] || k_band[2] > k_band[3])
        return fail(HTM_EINVAL, "band bins must satisfy 0 <= k1 <= k2 <= k3 <= k4 (got %d %d %d %d)", k_band[0], k_band[1], k_band[2], k_band[3]);
    const long last = cv_last(n_total, n);
    if (j0 < 0 || j0 > j1 || j1 > last) return fail(HTM_EINVAL, "segments %ld..%ld outside 0..%ld", j0, j1, last);
    const long S = j1 - j0 + 1;
    if (std::max(fft_max_items(n, 2 * S), 2 * S * (long)n) > kMaxWorkItems)
        return fail(HTM_EINVAL, "%ld segments of n = %d need more than 2^32 - 1 work-items in one launch", S, n);
    return HTM_OK;
}

}  // namespace

extern "C" {

int htm_fft_dev(int device, const double *d_in, long ld_in, double *d_out, long ld_out, long n, long batch, int direction,
                void *hip_stream)
{
    int rc = fft_check(d_in, ld_in, d_out, ld_out, n, batch, direction);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    const FftPlan *p = nullptr;
    if ((rc = fft_plan(device, n, &p))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StreamBuf ws;
    double2 *fw = nullptr;
    if ((rc = ws.alloc(st, [&](StreamBuf &b) { b.take(fw, fft_ws_elems(n, batch)); }))) return rc;
    if ((rc = fft_run(*p, reinterpret_cast<const double2 *>(d_in), ld_in, reinterpret_cast<double2 *>(d_out), ld_out, batch, direction, fw, st)))
        return rc;
    return ws.release();
}

int htm_fft(int device, const double *in, long ld_in, double *out, long ld_out, long n, long batch, int direction)
{
    int rc = fft_check(in, ld_in, out, ld_out, n, batch, direction);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevPool pool;
    const size_t ni = 2 * ((size_t)(batch - 1) * ld_in + n), no = 2 * ((size_t)(batch - 1) * ld_out + n);
    double *di = nullptr, *dout = nullptr;
    if ((rc = pool.upload(&dout, out, no))) return rc;      // keeps the padding between strided rows
    if (in == out) di = dout;
    else if ((rc = pool.upload(&di, in, ni))) return rc;
    if ((rc = htm_fft_dev(device, di, ld_in, dout, ld_out, n, batch, direction, nullptr))) return rc;
    return pool.download(out, dout, no, "FFT or its");
}

int htm_convert_dev(int device, const float *d_x1, const float *d_x2, long n_total, int n, int n_fac, int h,
                    const int k_band[4], double fac1, double fac2, long j0, long j1, double *d_out, void *hip_stream)
{
    if (!d_x1 || !d_x2 || !d_out) return fail(HTM_EINVAL, "NULL argument");
    int rc = cv_check(n_total, n, n_fac, h, k_band, j0, j1);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    const FftPlan *p = nullptr;
    if ((rc = fft_plan(device, n, &p))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const long S = j1 - j0 + 1, n2 = n / 2, last = cv_last(n_total, n);
    const long n_valid = std::min(n_total, j1 * n2 + n) - j0 * n2;
    // workspace: z [S][n] (later the first smoothing [2S][n] doubles), y [2S][n], the FFT's own, 4S coefficients
    const long sn = S * n;
    StreamBuf ws;
    double2 *z = nullptr, *y = nullptr, *fw = nullptr;
    double *coef = nullptr;
    if ((rc = ws.alloc(st, [&](StreamBuf &b) {
            b.take(z, (size_t)sn);
            b.take(y, 2 * (size_t)sn);
            b.take(fw, fft_ws_elems(n, 2 * S));
            b.take(coef, 4 * (size_t)S);
        }))) return rc;
    hipLaunchKernelGGL(k_cv_detrend, dim3((unsigned)S), dim3(kCvSumThreads), 0, st, d_x1, d_x2, n_valid, n, coef);
    hipLaunchKernelGGL(k_cv_pack, fft_grid(sn), dim3(kCvThreads), 0, st, d_x1, d_x2, n_valid, n, coef, z, sn);
    if ((rc = fft_run(*p, z, n, z, n, S, -1, fw, st))) return rc;
    const int4 kb = make_int4(k_band[0], k_band[1], k_band[2], k_band[3]);
    hipLaunchKernelGGL(k_cv_spectrum, fft_grid(sn), dim3(kCvThreads), 0, st, z, n, kb, y, sn);
    if ((rc = fft_run(*p, y, n, y, n, 2 * S, +1, fw, st))) return rc;
    const int tiles1 = (int)ceil_div(n, kCvTile), tiles2 = (int)ceil_div(n - n / 4, kCvTile);
    const size_t lds = 2 * (size_t)(kCvTile + 2 * h) * sizeof(double);
    double *e1 = reinterpret_cast<double *>(z);
    const long k_base = ceil_div(cv_start(j0, n), n_fac);
    hipLaunchKernelGGL(k_cv_smooth<false>, dim3((unsigned)(S * tiles1)), dim3(kCvThreads), lds, st, y, (const double *)nullptr, e1, n, h,
                       tiles1, j0, last, n_total, n_fac, k_base, fac1, fac2, (double *)nullptr);
    hipLaunchKernelGGL(k_cv_smooth<true>, dim3((unsigned)(S * tiles2)), dim3(kCvThreads), lds, st, (const double2 *)nullptr, e1,
                       (double *)nullptr, n, h, tiles2, j0, last, n_total, n_fac, k_base, fac1, fac2, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HTM_EHIP, "step-1 kernels failed to launch: %s", hipGetErrorString(e));
    return ws.release();
}

int htm_convert(int device, const float *x1, const float *x2, long n_total, int n, int n_fac, int h, const int k_band[4],
                double fac1, double fac2, long j0, long j1, double *out)
{
    if (!x1 || !x2 || !out) return fail(HTM_EINVAL, "NULL argument");
    int rc = cv_check(n_total, n, n_fac, h, k_band, j0, j1);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    DevPool pool;
    const long n2 = n / 2;
    const size_t n_valid = (size_t)(std::min(n_total, j1 * n2 + n) - j0 * n2);
    const size_t n_out = (size_t)(ceil_div(cv_end(j1, n_total, n), n_fac) - ceil_div(cv_start(j0, n), n_fac));
    float *d1 = nullptr, *d2 = nullptr;
    double *dout = nullptr;
    if ((rc = pool.upload(&d1, x1, n_valid)) || (rc = pool.upload(&d2, x2, n_valid)) || (rc = pool.alloc(&dout, n_out)))
        return rc;
    if ((rc = htm_convert_dev(device, d1, d2, n_total, n, n_fac, h, k_band, fac1, fac2, j0, j1, dout, nullptr))) return rc;
    return pool.download(out, dout, n_out, "step-1 kernels or their");
}

}  // extern "C"
