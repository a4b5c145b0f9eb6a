// htm_forward.hip -- the C ABI (include/htm_hip.h) of the forward model over the kernels in htm_kernels.hpp: htm_forward_*,
// htm_device_*, the library's one last-error string, htm_rng_jump and the self-tests.  What the units share: htm_host.hpp.
#include "htm_host.hpp"
#include "htm_forward_kernels.hpp"

#include <cmath>
#include <cstdarg>
#include <string>

using namespace htm;

namespace {
thread_local std::string g_err;      // behind htm_last_error(): every unit's failures go through fail()
}

namespace htm {

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int use_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(HTM_ENODEVICE, "no HIP device available (%s); libhtm_hip has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(HTM_EINVAL, "device %d out of range (0..%d)", device, n - 1);
    HIPCHK(hipSetDevice(device));
    return HTM_OK;
}

static Bits128 xs_step(Bits128 s)
{
    const uint32_t t = s.w[0] ^ (s.w[0] << 11);
    Bits128 r;
    r.w[0] = s.w[1]; r.w[1] = s.w[2]; r.w[2] = s.w[3];
    r.w[3] = (s.w[3] ^ (s.w[3] >> 19)) ^ (t ^ (t >> 8));
    return r;
}
Bits128 gf2_matvec(const Mat128 &M, const Bits128 &v)
{
    Bits128 a{{0, 0, 0, 0}};
    for (int j = 0; j < 128; ++j)
        if ((v.w[j >> 5] >> (j & 31)) & 1u)
            for (int k = 0; k < 4; ++k) a.w[k] ^= M[j].w[k];
    return a;
}
// P[k] = T^(2^k), k = 0..63
const std::vector<Mat128> &xs_powers()
{
    static const std::vector<Mat128> P = [] {
        std::vector<Mat128> p(64);
        for (int j = 0; j < 128; ++j) {
            Bits128 e{{0, 0, 0, 0}};
            e.w[j >> 5] = 1u << (j & 31);
            p[0][j] = xs_step(e);
        }
        for (int k = 1; k < 64; ++k)
            for (int j = 0; j < 128; ++j) p[k][j] = gf2_matvec(p[k - 1], p[k - 1][j]);
        return p;
    }();
    return P;
}

int launch_full(htm_forward *h, const FullJob &jb, int gy)
{
    dim3 grid(h->n_wg, gy), block(256);
    const size_t smem = 0;
    if (h->dev.fp32) {        // fp32 forward: htm_forward_set_precision allows it for one or two stations per lane only
        if (h->nch != 1 && h->nch != 2) return fail(HTM_ESTATE, "fp32 forward on a handle with %d stations", h->S);
        if (jb.desc) {
            if (h->nch == 1) hipLaunchKernelGGL((k_full<1, false, true>), grid, block, smem, h->stream, h->dev, jb);
            else hipLaunchKernelGGL((k_full<2, false, true>), grid, block, smem, h->stream, h->dev, jb);
        } else {
            if (h->nch == 1) hipLaunchKernelGGL((k_full<1, true, true>), grid, block, smem, h->stream, h->dev, jb);
            else hipLaunchKernelGGL((k_full<2, true, true>), grid, block, smem, h->stream, h->dev, jb);
        }
    } else if (jb.desc) {
        switch (h->nch) {
        case 1: hipLaunchKernelGGL((k_full<1, false>), grid, block, smem, h->stream, h->dev, jb); break;
        case 2: hipLaunchKernelGGL((k_full<2, false>), grid, block, smem, h->stream, h->dev, jb); break;
        case 4: hipLaunchKernelGGL((k_full<4, false>), grid, block, smem, h->stream, h->dev, jb); break;
        default: hipLaunchKernelGGL((k_full<0, false>), grid, block, smem, h->stream, h->dev, jb); break;
        }
    } else {
        switch (h->nch) {
        case 1: hipLaunchKernelGGL((k_full<1, true>), grid, block, smem, h->stream, h->dev, jb); break;
        case 2: hipLaunchKernelGGL((k_full<2, true>), grid, block, smem, h->stream, h->dev, jb); break;
        case 4: hipLaunchKernelGGL((k_full<4, true>), grid, block, smem, h->stream, h->dev, jb); break;
        default: hipLaunchKernelGGL((k_full<0, true>), grid, block, smem, h->stream, h->dev, jb); break;
        }
    }
    HIPCHK(hipGetLastError());
    return HTM_OK;
}

static int ensure_batch_scratch(htm_forward *h, int n_models)
{
    const size_t need = (size_t)n_models * h->n_wg;
    if (need > h->bpartial_cap) {
        if (h->d_bpartial) HIPCHK(hipFree(h->d_bpartial));
        h->d_bpartial = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&h->d_bpartial), need * sizeof(double)));
        h->bpartial_cap = need;
    }
    return HTM_OK;
}

int full_batch_dev(htm_forward *h, int n_models, const double *d_hypo, const double *d_tc, const double *d_vs,
                   const double *d_ac, const double *d_qs, double *d_L)
{
    int rc = ensure_batch_scratch(h, n_models);
    if (rc) return rc;
    FullJob jb{};
    jb.hypo = d_hypo; jb.hypo_stride = 3L * h->E;
    jb.tc = d_tc; jb.tc_stride = h->S;
    jb.ac = d_ac; jb.ac_stride = h->S;
    jb.vs = d_vs; jb.qs = d_qs;
    jb.n_models = n_models;
    jb.partial = h->d_bpartial; jb.n_wg = h->n_wg; jb.epw = h->epw;
    int gy = std::max(1, std::min(n_models, 2048 / std::max(1, h->n_wg)));
    if (const char *e = getenv("HTM_FULL_BLOCKS")) gy = std::max(1, std::min(n_models, atoi(e) / std::max(1, h->n_wg)));      // (tuning: blocks per launch)
    rc = launch_full(h, jb, gy);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sum_partials, dim3(n_models), dim3(64), 0, h->stream, h->d_bpartial, h->n_wg,
                       h->dev.const_sum, d_L);
    HIPCHK(hipGetLastError());
    return HTM_OK;
}

// The packed records (FwdDev::obs_pack, htm_device.hpp) for the precision in use, from the device's own rows -- the same bits
// the row loads return.  The observations never change after htm_forward_create, so neither do the records.  They repeat the
// four streams: 2 MB more at 1000 events x 64 stations in fp64, 41 MB at 10 000 x 128 -- only for a forward
// whose chain set can run the specialised master (htm_chains_create asks for them).
int ensure_obs_pack(htm_forward *h)
{
    if (!h->pack_wanted) { h->dev.obs_pack = nullptr; return HTM_OK; }
    const bool f32 = h->dev.fp32 != 0;
    void *&slot = f32 ? h->d_pack32 : h->d_pack64;
    if (!slot) {
        if ((h->nch != 1 && h->nch != 2) || h->S != 64 * h->nch) return fail(HTM_EINVAL, "packed records need full rows of 64 or 128 stations");
        const size_t S = (size_t)h->S, E = (size_t)h->E, n = S * E, es = f32 ? sizeof(float) : sizeof(double);
        const size_t stride = obs_pack_stride(h->nch, f32);
        const void *src[4] = {f32 ? (const void *)h->dev.t_obs32 : (const void *)h->dev.t_obs, f32 ? (const void *)h->dev.t_prec32 : (const void *)h->dev.t_prec,
                              f32 ? (const void *)h->dev.a_obs32 : (const void *)h->dev.a_obs, f32 ? (const void *)h->dev.a_prec32 : (const void *)h->dev.a_prec};
        std::vector<char> rows(n * es), buf(stride * E, 0);
        for (int k = 0; k < 4; ++k) {
            HIPCHK(hipMemcpy(rows.data(), src[k], n * es, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < E; ++i) std::memcpy(buf.data() + i * stride + (size_t)k * S * es, rows.data() + i * S * es, S * es);
        }
        std::vector<double> rt(E), ra(E);
        HIPCHK(hipMemcpy(rt.data(), h->dev.rpsum_t, E * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ra.data(), h->dev.rpsum_a, E * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < E; ++i) {
            std::memcpy(buf.data() + i * stride + 4 * S * es, &rt[i], sizeof(double));
            std::memcpy(buf.data() + i * stride + 4 * S * es + sizeof(double), &ra[i], sizeof(double));
        }
        char *p = nullptr;
        int rc = dev_upload(h->pool, &p, buf.data(), buf.size());
        if (rc) return rc;
        slot = p;
    }
    h->dev.obs_pack = slot;
    return HTM_OK;
}

}  // namespace htm

// ====================================================================================================
extern "C" {

const char *htm_last_error(void) { return g_err.c_str(); }
int htm_abi_version(void) { return 1; }

int htm_device_count(int *n)
{
    if (!n) return fail(HTM_EINVAL, "n is NULL");
    *n = 0;
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) { *n = 0; return fail(HTM_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    return HTM_OK;
}

int htm_device_physical_id(int device, int *id)
{
    if (!id) return fail(HTM_EINVAL, "id is NULL");
    *id = -1;
    int dom = 0, bus = 0, dv = 0;
    if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device) != hipSuccess ||
        hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device) != hipSuccess ||
        hipDeviceGetAttribute(&dv, hipDeviceAttributePciDeviceId, device) != hipSuccess)
        return fail(HTM_ENODEVICE, "no PCI address for HIP device %d", device);
    *id = ((dom & 0x7fff) << 16) | ((bus & 0xff) << 8) | (dv & 0xff);
    return HTM_OK;
}

// ---------------------------------------------------------------------------------------------------
int htm_forward_create(int n_sta, int n_events, const double *sta_x, const double *sta_y, const double *sta_z,
                       const double *t_obs, const double *t_stdv, const double *a_obs, const double *a_stdv,
                       int use_time, int use_amp, int device, htm_forward **out)
{
    if (!out) return fail(HTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_sta <= 0 || n_events <= 0) return fail(HTM_EINVAL, "n_sta and n_events must be positive");
    if (!sta_x || !sta_y || !sta_z || !t_obs || !t_stdv || !a_obs || !a_stdv)
        return fail(HTM_EINVAL, "NULL input array");
    int rc = use_device(device);
    if (rc) return rc;

    // (owns the handle until it is handed out: every early return destroys what was made so far)
    struct Guard {
        htm_forward *h;
        ~Guard() { if (h) htm_forward_destroy(h); }
    } guard{new htm_forward()};
    htm_forward *h = guard.h;
    h->device = device; h->S = n_sta; h->E = n_events; h->nch = nch_for(n_sta);
    const size_t n = (size_t)n_sta * n_events;

    // init_forward, cls_forward.f90:76-92: precision, log-stdv and the missing-data rule (keyed on t_stdv
    // only; log-stdv := 1.0 (sic), stdv := 1, precision := 1 for BOTH data types)
    std::vector<double> tpr(n), apr(n), pst(n_events), psa(n_events), lct(n_events), lca(n_events);
    const double log_2pi_half = 0.5 * std::log(2.0 * std::acos(-1.0));
    double const_t = 0.0, const_a = 0.0;
    for (int i = 0; i < n_events; ++i) {
        double st = 0.0, sa = 0.0, ct = 0.0, ca = 0.0;
        for (int j = 0; j < n_sta; ++j) {
            const size_t k = (size_t)i * n_sta + j;
            double lts, las;
            if (t_stdv[k] > 1.e-16) {
                lts = std::log(t_stdv[k]); tpr[k] = 1.0 / (t_stdv[k] * t_stdv[k]);
                las = std::log(a_stdv[k]); apr[k] = 1.0 / (a_stdv[k] * a_stdv[k]);
            } else {
                lts = 1.0; tpr[k] = 1.0; las = 1.0; apr[k] = 1.0;
            }
            st += tpr[k]; sa += apr[k];
            const_t += log_2pi_half + lts;
            const_a += log_2pi_half + las;
            ct += log_2pi_half + lts; ca += log_2pi_half + las;
        }
        pst[i] = st; psa[i] = sa; lct[i] = ct; lca[i] = ca;
    }

    double *p = nullptr;
#define UP(dst, src, cnt)                                          \
    if ((rc = dev_upload(h->pool, &p, (src), (cnt)))) return rc; \
    dst = p;
    UP(h->dev.sx, sta_x, n_sta) UP(h->dev.sy, sta_y, n_sta) UP(h->dev.sz, sta_z, n_sta)
    UP(h->dev.t_obs, t_obs, n) UP(h->dev.t_prec, tpr.data(), n)
    UP(h->dev.a_obs, a_obs, n) UP(h->dev.a_prec, apr.data(), n)
    UP(h->dev.psum_t, pst.data(), n_events) UP(h->dev.psum_a, psa.data(), n_events)
    {
        std::vector<double> rt(n_events), ra(n_events);
        for (int i = 0; i < n_events; ++i) { rt[i] = 1.0 / pst[i]; ra[i] = 1.0 / psa[i]; }
        UP(h->dev.rpsum_t, rt.data(), n_events) UP(h->dev.rpsum_a, ra.data(), n_events)
    }
    UP(h->d_lconst_t, lct.data(), n_events) UP(h->d_lconst_a, lca.data(), n_events)
#undef UP
    h->dev.S = n_sta; h->dev.E = n_events; h->dev.use_time = use_time ? 1 : 0; h->dev.use_amp = use_amp ? 1 : 0;
    h->dev.const_sum = (use_time ? const_t : 0.0) + (use_amp ? const_a : 0.0);

    h->epw = std::max(1, (n_events + 4 * 1024 - 1) / (4 * 1024));
    h->n_wg = (n_events + 4 * h->epw - 1) / (4 * h->epw);

    if ((rc = dev_alloc(h->pool, &h->d_hypo, 3 * (size_t)n_events))) return rc;
    if ((rc = dev_alloc(h->pool, &h->d_tc, n_sta))) return rc;
    if ((rc = dev_alloc(h->pool, &h->d_ac, n_sta))) return rc;
    if ((rc = dev_alloc(h->pool, &h->d_scal, 16))) return rc;
    if ((rc = dev_alloc(h->pool, &h->d_partial, h->n_wg))) return rc;
    if ((rc = dev_alloc(h->pool, &h->d_syn, n))) return rc;
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(HTM_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    h->stream = h->own_stream;
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess)
        return fail(HTM_EHIP, "hipEventCreate failed");
    *out = h;
    guard.h = nullptr;
    return HTM_OK;
}

int htm_forward_destroy(htm_forward *h)
{
    if (!h) return HTM_OK;
    (void)hipSetDevice(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    for (void *p : h->pool) (void)hipFree(p);
    if (h->d_bpartial) (void)hipFree(h->d_bpartial);
    if (h->d_bmodels) (void)hipFree(h->d_bmodels);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return HTM_OK;
}

int htm_forward_obs_pack_bytes(htm_forward *h, int64_t *bytes)
{
    if (!h || !bytes) return fail(HTM_EINVAL, "NULL argument");
    *bytes = (h->d_pack64 ? (int64_t)(obs_pack_stride(h->nch, false) * (size_t)h->E) : 0) +
             (h->d_pack32 ? (int64_t)(obs_pack_stride(h->nch, true) * (size_t)h->E) : 0);
    return HTM_OK;
}

int htm_forward_set_precision(htm_forward *h, int forward_fp32)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!forward_fp32) { h->dev.fp32 = 0; return ensure_obs_pack(h); }
    if (h->nch != 1 && h->nch != 2) return fail(HTM_EINVAL, "the fp32 forward covers n_sta <= 128 (this handle has %d stations)", h->S);
    if (!h->dev.t_obs32) {
        // the four observation streams once more as float: the bytes a full evaluation reads are halved
        const size_t n = (size_t)h->S * h->E;
        std::vector<double> tmp(n);
        std::vector<float> f32(n);
        const double *src[4] = {h->dev.t_obs, h->dev.t_prec, h->dev.a_obs, h->dev.a_prec};
        const float **dst[4] = {&h->dev.t_obs32, &h->dev.t_prec32, &h->dev.a_obs32, &h->dev.a_prec32};
        for (int k = 0; k < 4; ++k) {
            HIPCHK(hipMemcpy(tmp.data(), src[k], n * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i) f32[i] = (float)tmp[i];
            float *p = nullptr;
            int rc = dev_upload(h->pool, &p, f32.data(), n);
            if (rc) return rc;
            *dst[k] = p;
        }
    }
    h->dev.fp32 = 1;
    return ensure_obs_pack(h);
}

int htm_forward_set_stream(htm_forward *h, void *hip_stream)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->stream = static_cast<hipStream_t>(hip_stream);
    return HTM_OK;
}

int htm_forward_reset_stream(htm_forward *h)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->stream = h->own_stream;
    return HTM_OK;
}

int htm_forward_sync(htm_forward *h)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HTM_OK;
}

int htm_forward_loglik_full(htm_forward *h, const double *hypo, const double *t_corr, double vs,
                            const double *a_corr, double qs, double *log_likelihood)
{
    if (!h || !hypo || !t_corr || !a_corr || !log_likelihood) return fail(HTM_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(h->device));
    const double sc[2] = {vs, qs};
    HIPCHK(hipMemcpyAsync(h->d_hypo, hypo, 3 * (size_t)h->E * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_tc, t_corr, h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ac, a_corr, h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_scal, sc, sizeof(sc), hipMemcpyHostToDevice, h->stream));
    int rc = full_batch_dev(h, 1, h->d_hypo, h->d_tc, h->d_scal, h->d_ac, h->d_scal + 1, h->d_scal + 2);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(log_likelihood, h->d_scal + 2, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HTM_OK;
}

int htm_forward_loglik_partial(htm_forward *h, int evt_id, const double hypo_old_xyz[3],
                               double log_likelihood_old, const double hypo_xyz[3], const double *t_corr,
                               double vs, const double *a_corr, double qs, double *log_likelihood)
{
    if (!h || !hypo_old_xyz || !hypo_xyz || !t_corr || !a_corr || !log_likelihood)
        return fail(HTM_EINVAL, "NULL argument");
    if (evt_id < 1 || evt_id > h->E) return fail(HTM_EINVAL, "evt_id %d out of range 1..%d", evt_id, h->E);
    HIPCHK(hipSetDevice(h->device));
    const double sc[6] = {hypo_old_xyz[0], hypo_old_xyz[1], hypo_old_xyz[2], hypo_xyz[0], hypo_xyz[1], hypo_xyz[2]};
    HIPCHK(hipMemcpyAsync(h->d_tc, t_corr, h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_ac, a_corr, h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_scal + 4, sc, sizeof(sc), hipMemcpyHostToDevice, h->stream));
    if (h->dev.fp32 && h->nch <= 2 && h->nch >= 1) {
        if (h->nch == 1) hipLaunchKernelGGL((k_partial_one<1, true>), dim3(1), dim3(64), 0, h->stream, h->dev, evt_id - 1, h->d_scal + 4, h->d_scal + 7, h->d_tc, h->d_ac, vs, qs, log_likelihood_old, h->d_scal + 2);
        else hipLaunchKernelGGL((k_partial_one<2, true>), dim3(1), dim3(64), 0, h->stream, h->dev, evt_id - 1, h->d_scal + 4, h->d_scal + 7, h->d_tc, h->d_ac, vs, qs, log_likelihood_old, h->d_scal + 2);
    } else
    switch (h->nch) {
    case 1: hipLaunchKernelGGL(k_partial_one<1>, dim3(1), dim3(64), 0, h->stream, h->dev, evt_id - 1, h->d_scal + 4, h->d_scal + 7, h->d_tc, h->d_ac, vs, qs, log_likelihood_old, h->d_scal + 2); break;
    case 2: hipLaunchKernelGGL(k_partial_one<2>, dim3(1), dim3(64), 0, h->stream, h->dev, evt_id - 1, h->d_scal + 4, h->d_scal + 7, h->d_tc, h->d_ac, vs, qs, log_likelihood_old, h->d_scal + 2); break;
    case 4: hipLaunchKernelGGL(k_partial_one<4>, dim3(1), dim3(64), 0, h->stream, h->dev, evt_id - 1, h->d_scal + 4, h->d_scal + 7, h->d_tc, h->d_ac, vs, qs, log_likelihood_old, h->d_scal + 2); break;
    default: hipLaunchKernelGGL(k_partial_one<0>, dim3(1), dim3(64), 0, h->stream, h->dev, evt_id - 1, h->d_scal + 4, h->d_scal + 7, h->d_tc, h->d_ac, vs, qs, log_likelihood_old, h->d_scal + 2); break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(log_likelihood, h->d_scal + 2, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HTM_OK;
}

static int syn_common(htm_forward *h, const double *hypo, const double *corr, double beta, double q, int which,
                      int evt_id, double *out)
{
    if (!h || !hypo || !corr || !out) return fail(HTM_EINVAL, "NULL argument");
    if (evt_id != 0 && (evt_id < 1 || evt_id > h->E))
        return fail(HTM_EINVAL, "evt_id %d out of range 1..%d", evt_id, h->E);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h->d_hypo, hypo, 3 * (size_t)h->E * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_tc, corr, h->S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int nblk = evt_id ? 1 : (h->E + 3) / 4;
    hipLaunchKernelGGL(k_syn, dim3(nblk), dim3(256), 0, h->stream, h->dev, h->d_hypo, h->d_tc, beta, q, which,
                       evt_id ? evt_id - 1 : -1, h->d_syn);
    HIPCHK(hipGetLastError());
    const size_t cnt = evt_id ? (size_t)h->S : (size_t)h->S * h->E;
    HIPCHK(hipMemcpyAsync(out, h->d_syn, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HTM_OK;
}

int htm_forward_travel_time(htm_forward *h, const double *hypo, const double *t_corr, double vs, double *t_syn)
{ return syn_common(h, hypo, t_corr, vs, 1.0, 0, 0, t_syn); }
int htm_forward_amp(htm_forward *h, const double *hypo, const double *a_corr, double qs, double vs, double *a_syn)
{ return syn_common(h, hypo, a_corr, vs, qs, 1, 0, a_syn); }
int htm_forward_travel_time_single(htm_forward *h, int evt_id, const double *hypo, const double *t_corr,
                                   double vs, double *t_syn)
{
    if (h && (evt_id < 1 || evt_id > h->E)) return fail(HTM_EINVAL, "evt_id %d out of range", evt_id);
    return syn_common(h, hypo, t_corr, vs, 1.0, 0, evt_id, t_syn);
}
int htm_forward_amp_single(htm_forward *h, int evt_id, const double *hypo, const double *a_corr, double qs,
                           double vs, double *a_syn)
{
    if (h && (evt_id < 1 || evt_id > h->E)) return fail(HTM_EINVAL, "evt_id %d out of range", evt_id);
    return syn_common(h, hypo, a_corr, vs, qs, 1, evt_id, a_syn);
}

int htm_forward_loglik_full_batch_dev(htm_forward *h, int n_models, const double *d_hypo, const double *d_t_corr,
                                      const double *d_vs, const double *d_a_corr, const double *d_qs,
                                      double *d_log_likelihood)
{
    if (!h || !d_hypo || !d_t_corr || !d_vs || !d_a_corr || !d_qs || !d_log_likelihood)
        return fail(HTM_EINVAL, "NULL argument");
    if (n_models <= 0) return fail(HTM_EINVAL, "n_models must be positive");
    HIPCHK(hipSetDevice(h->device));
    return full_batch_dev(h, n_models, d_hypo, d_t_corr, d_vs, d_a_corr, d_qs, d_log_likelihood);
}

int htm_forward_loglik_full_batch(htm_forward *h, int n_models, const double *hypo, const double *t_corr,
                                  const double *vs, const double *a_corr, const double *qs, double *log_likelihood)
{
    if (!h || !hypo || !t_corr || !vs || !a_corr || !qs || !log_likelihood) return fail(HTM_EINVAL, "NULL argument");
    if (n_models <= 0) return fail(HTM_EINVAL, "n_models must be positive");
    HIPCHK(hipSetDevice(h->device));
    const size_t nh = 3 * (size_t)h->E, ns = h->S;
    const size_t per = nh + 2 * ns + 3, need = per * n_models;
    if (need > h->bmodels_cap) {
        if (h->d_bmodels) HIPCHK(hipFree(h->d_bmodels));
        h->d_bmodels = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&h->d_bmodels), need * sizeof(double)));
        h->bmodels_cap = need;
    }
    double *dh = h->d_bmodels, *dt = dh + nh * n_models, *da = dt + ns * n_models, *dv = da + ns * n_models,
           *dq = dv + n_models, *dL = dq + n_models;
    HIPCHK(hipMemcpyAsync(dh, hypo, nh * n_models * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dt, t_corr, ns * n_models * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(da, a_corr, ns * n_models * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dv, vs, n_models * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dq, qs, n_models * sizeof(double), hipMemcpyHostToDevice, h->stream));
    int rc = full_batch_dev(h, n_models, dh, dt, dv, da, dq, dL);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(log_likelihood, dL, n_models * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HTM_OK;
}

int htm_forward_time_full_batch_dev(htm_forward *h, int n_models, const double *d_hypo, const double *d_t_corr,
                                    const double *d_vs, const double *d_a_corr, const double *d_qs,
                                    double *d_log_likelihood, int reps, double *avg_us)
{
    if (!h || !avg_us || reps <= 0) return fail(HTM_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    int rc = htm_forward_loglik_full_batch_dev(h, n_models, d_hypo, d_t_corr, d_vs, d_a_corr, d_qs, d_log_likelihood);
    if (rc) return rc;   // warm-up, also sizes the scratch
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int r = 0; r < reps; ++r) {
        rc = full_batch_dev(h, n_models, d_hypo, d_t_corr, d_vs, d_a_corr, d_qs, d_log_likelihood);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *avg_us = 1000.0 * ms / reps;
    return HTM_OK;
}

// ---------------------------------------------------------------------------------------------------
int htm_rng_jump(const uint32_t state_in[4], unsigned long long n_draws, uint32_t state_out[4])
{
    if (!state_in || !state_out) return fail(HTM_EINVAL, "NULL argument");
    const std::vector<Mat128> &P = xs_powers();
    Bits128 s{{state_in[0], state_in[1], state_in[2], state_in[3]}};
    for (int k = 0; k < 64; ++k)
        if ((n_draws >> k) & 1ull) s = gf2_matvec(P[k], s);
    for (int k = 0; k < 4; ++k) state_out[k] = s.w[k];
    return HTM_OK;
}

// the parallel generator against a serial loop on the device: n draws from `seed`, ring of `cap` positions starting at `start`
static int selftest_rawgen(const uint32_t seed[4], int n, long long start, long long cap)
{
    std::vector<void *> pool;
    auto done = [&](int code) { for (void *p : pool) (void)hipFree(p); return code; };
    StreamDev sd{};
    sd.mask = cap - 1;
    uint32_t *d_ser = nullptr, *d_gen = nullptr;
    u32x4 *d_jump = nullptr;
    int rc;
    if ((rc = dev_alloc(pool, &sd.raw, (size_t)cap)) || (rc = dev_alloc(pool, &d_ser, (size_t)n))) return done(rc);
    uint32_t g16[16] = {seed[0], seed[1], seed[2], seed[3]};
    if ((rc = dev_upload(pool, &d_gen, g16, 16))) return done(rc);
    const std::vector<Mat128> &P = xs_powers();
    std::vector<u32x4> jt((size_t)kJumpLevels * 128);
    for (int b = 0; b < kJumpLevels; ++b)
        for (int j = 0; j < 128; ++j) jt[(size_t)b * 128 + j] = u32x4{P[6 + b][j].w[0], P[6 + b][j].w[1], P[6 + b][j].w[2], P[6 + b][j].w[3]};
    if ((rc = dev_upload(pool, &d_jump, jt.data(), jt.size()))) return done(rc);
    hipLaunchKernelGGL(k_rawgen, dim3((unsigned)((n + 4095) / 4096)), dim3(64), 0, 0, sd, start, n, d_jump, d_gen, d_gen + 4);
    hipLaunchKernelGGL(k_rawgen_serial, dim3(1), dim3(1), 0, 0, d_ser, n, d_gen, d_gen + 8);
    if (hipDeviceSynchronize() != hipSuccess) return done(fail(HTM_EHIP, "rawgen selftest kernels failed"));
    std::vector<uint32_t> ring((size_t)cap), ser((size_t)n);
    uint32_t g[16];
    if (hipMemcpy(ring.data(), sd.raw, cap * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ser.data(), d_ser, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(g, d_gen, sizeof(g), hipMemcpyDeviceToHost) != hipSuccess) return done(fail(HTM_EHIP, "download failed"));
    for (int k = 0; k < n; ++k)
        if (ring[(size_t)((start + k) & (cap - 1))] != ser[k])
            return done(fail(HTM_ESTATE, "parallel xorshift128 differs from the serial stream at draw %d of %d", k, n));
    uint32_t hj[4];
    htm_rng_jump(seed, (unsigned long long)n, hj);
    for (int k = 0; k < 4; ++k)
        if (g[4 + k] != g[8 + k] || g[4 + k] != hj[k])
            return done(fail(HTM_ESTATE, "generator state after %d draws: parallel %08x serial %08x host jump %08x", n, g[4 + k], g[8 + k], hj[k]));
    return done(HTM_OK);
}

int htm_selftest_math(int device, int which, const double *x, double *y, int n)
{
    int rc = use_device(device);
    if (rc) return rc;
    if (!x || !y || n < 0 || which < 0 || which > 9 || (which == 4 && n % 64 != 0) || ((which == 5 || which == 6 || which >= 8) && n % 256 != 0))
        return fail(HTM_EINVAL, "htm_selftest_math: null pointer, negative count or unknown function");
    if (n == 0) return HTM_OK;
    double *d = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d), 2 * (size_t)n * sizeof(double)));
    auto done = [&](int code) { (void)hipFree(d); return code; };
    if (hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return done(fail(HTM_EHIP, "htm_selftest_math: copy in"));
    hipLaunchKernelGGL(k_mathtest, dim3((n + 255) / 256), dim3(256), 0, 0, which, d, d + n, n);
    if (hipGetLastError() != hipSuccess || hipMemcpy(y, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(HTM_EHIP, "htm_selftest_math: kernel or copy out failed"));
    return done(HTM_OK);
}

int htm_selftest(int device)
{
    int rc = use_device(device);
    if (rc) return rc;
    std::vector<double> in(128);
    uint32_t s = 12345u;
    for (auto &v : in) { s = s * 1664525u + 1013904223u; v = (double)(int32_t)s / 65536.0 / 7.0; }
    double *d_in = nullptr, *d_o = nullptr;
    uint32_t *d_r = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_in), 128 * sizeof(double)));
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_o), 16 * sizeof(double)));
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_r), 8 * sizeof(uint32_t)));
    HIPCHK(hipMemcpy(d_in, in.data(), 128 * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, 0, d_in, d_o, d_o + 2, d_r, d_o + 4);
    HIPCHK(hipGetLastError());
    double o[16];
    uint32_t r[8];
    HIPCHK(hipMemcpy(o, d_o, sizeof(o), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(r, d_r, sizeof(r), hipMemcpyDeviceToHost));
    (void)hipFree(d_in); (void)hipFree(d_o); (void)hipFree(d_r);
    if (memcmp(&o[0], &o[2], 2 * sizeof(double)) != 0)
        return fail(HTM_ESTATE, "DPP wave_sum mismatch: %.17g vs %.17g / %.17g vs %.17g", o[0], o[2], o[1], o[3]);
    // SURVEY.md §8a golden vector: first five rand_u() of rank 0
    const double want[5] = {0.55850877496413887, 0.12064291047863662, 0.58295862120576203, 0.68001799611374736,
                            0.45020412676967681};
    for (int i = 0; i < 5; ++i)
        if (o[4 + i] != want[i]) return fail(HTM_ESTATE, "device rand_u[%d] = %.17g, want %.17g", i, o[4 + i], want[i]);
    if (o[13] != 0.0) return fail(HTM_ESTATE, "DPP wave_incl_scan disagrees with the serial prefix sum");
    if (std::fabs(o[12] - 0.78381228502204603) > 1e-15)
        return fail(HTM_ESTATE, "device rand_g = %.17g, want 0.78381228502204603", o[12]);
    // jump-ahead generator == serial generator: one wave, several waves with a ragged tail, a ring wrap-around
    const uint32_t seed0[4] = {0x4b88a366u, 0x1b11733cu, 0x097044b6u, 0x00676ea2u};   // rank-0 state
    const uint32_t seed1[4] = {0x311ce1d7u, 0x6c840a86u, 0x28236c5fu, 0x019ea85du};   // rank 1
    if ((rc = selftest_rawgen(seed0, 64, 0, 1 << 12))) return rc;
    if ((rc = selftest_rawgen(seed0, 4096 * 3 + 64 * 5, 0, 1 << 14))) return rc;
    if ((rc = selftest_rawgen(seed1, 1 << 16, (1 << 16) - 4096 - 192, 1 << 16))) return rc;
    if ((rc = selftest_rawgen(seed1, 1 << 18, 12345 * 64, 1 << 18))) return rc;
    return HTM_OK;
}

}  // extern "C"
