// htm_locate.hip -- the locate part of the C ABI (include/htm_hip.h): the location posterior of every event of a forward handle
// on a grid, under a fixed structure or marginalised over draws of it, the draws' evidences, the stacked density and the stations'
// residuals, and the same posterior on a box of its own per event, over the
// kernels of htm_locate.hpp -- the one unit that includes them.  What a call allocates and how it is batched is the plan of
// htm_locate_plan.hpp, which htm_forward_locate_plan gives out without a device; this unit runs it.  The handle itself
// (htm_forward, with d_lconst_t, d_lconst_a and loc_fp32 for these entry points) is htm_forward.hip's.
#include "htm_steps_host.hpp"
#include "htm_locate.hpp"

#include <cmath>

using namespace htm;

namespace {

// One call: what it wants (the request), what it is given and where its results go.  Host pointers; an output that is NULL is
// not downloaded.  The entry points fill it in; nothing below them reads a job out of which pointers are NULL.
struct LocCall {
    LocRequest rq;
    const double *t_corr, *vs, *a_corr, *qs;      // one structure (t_corr, a_corr [S]; *vs, *qs) or rq.n_draws of them ([n_draws][S]; [n_draws])
    const double *grid9, *prior5;
    const double *origin3;                        // [E][3] where rq.boxes: every event's box origin
    const int *layer;                             // [E] where rq.layer
    double *loc, *marg, *vol;                     // kLocFixed, kLocMarginal
    double *log_z, *summary;                      // kLocEvidence
    double *xy, *xz, *yz, *stack, *tally;         // rq.n_layer > 0; stack may be NULL
    double *res, *fit;                            // rq.residuals
};

// the device arrays of a call, each as long as the plan says (LocLengths; per event ones times the batch); nullptr: none
struct LocWork {
    DevPool pool;
    LocSta *sta = nullptr;
    LocEv *ev = nullptr;
    double *prior = nullptr, *part = nullptr, *vol = nullptr, *loc = nullptr, *marg = nullptr, *logz = nullptr, *sum = nullptr, *w = nullptr;
    double *stack = nullptr, *xy = nullptr, *xz = nullptr, *yz = nullptr, *tally = nullptr;
    int *layer = nullptr;
    double *rbase = nullptr, *rpart = nullptr, *res = nullptr, *fit = nullptr;
    double *org = nullptr;

    template <class T>
    int take(T **p, size_t n) { return n ? pool.alloc(p, n) : HTM_OK; }
};

// f(std::integral_constant<int, MODE>()) for the run-time mode 0 .. 3 (1: travel times, 2: amplitudes): a kernel family's instantiation
template <class F>
void with_mode(int mode, F f)
{
    switch (mode) {
    case 0: f(std::integral_constant<int, 0>()); break;
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    default: f(std::integral_constant<int, 3>()); break;
    }
}

// The prior of one event, p = {mu_x, mu_y, w_xy, z0, w_z}, on the grid: q [nx + ny + nz], the log densities per ix, iy (normalised
// Gaussians) and iz (the depth prior of cls_model.f90:178-185, normalised; -inf at and below z0).  The prior is separable.
void locate_prior_tables(const double *p, const MapGrid &g, double *q)
{
    const double log_2pi_half = 0.5 * std::log(2.0 * std::acos(-1.0));
    const double lw = std::log(p[2]), lwz = std::log(p[4]);
    for (int i = 0; i < g.nx; ++i) { const double d = map_centre(g.x0, g.dx, i) - p[0]; q[i] = (-log_2pi_half - lw) - d * d / (2.0 * p[2] * p[2]); }
    for (int i = 0; i < g.ny; ++i) { const double d = map_centre(g.y0, g.dy, i) - p[1]; q[g.nx + i] = (-log_2pi_half - lw) - d * d / (2.0 * p[2] * p[2]); }
    for (int i = 0; i < g.nz; ++i) {
        const double d = map_centre(g.z0, g.dz, i) - p[3];
        q[g.nx + g.ny + i] = d > 0.0 ? (std::log(d) - 2.0 * lwz) - d * d / (2.0 * p[4] * p[4]) : -INFINITY;
    }
}

// The run of one call in the precision of the handle: run() takes the steps in their order.  F32: the single-precision forward of
// htm_forward_locate_set_precision -- the kernels' F32 instantiations, and the draws' table in floats.
template <bool F32>
struct LocRun {
    typedef LocPairT<loc_real<F32>> Pair;
    htm_forward *h;
    const LocCall &c;
    LocPlan pl{};
    LocWork w;
    LocJob jb{};
    LocDraws<loc_real<F32>> dr{};
    std::vector<double> tab;      // a batch's prior tables
    std::vector<double> org;      // a batch's box origins, [m][4]

    LocRun(htm_forward *h_, const LocCall &c_) : h(h_), c(c_) {}

    // the plan; between the grid and the budget, the one check that reads the caller's data
    int plan()
    {
        if (int rc = locate_tiles(c.grid9, &pl)) return rc;
        if (c.rq.prior)
            for (int i = 0; i < c.rq.n_events; ++i)
                if (!(c.prior5[5 * i + 2] > 0.0) || !(c.prior5[5 * i + 4] > 0.0))
                    return fail(HTM_EINVAL, "event %d: prior widths w_xy = %g, w_z = %g: need values > 0", i, c.prior5[5 * i + 2], c.prior5[5 * i + 4]);
        double mb;
        if (int rc = env_mib("HTM_LOCATE_MB", 1024.0, &mb)) return rc;
        return locate_budget(c.rq, mb, &pl);
    }

    // every array of a batch and of the stack, from the plan's lengths; the stack starts from 0
    int workspace()
    {
        const LocLengths &n = pl.len;
        const size_t nb = (size_t)pl.nb;
        int rc;
        if ((rc = w.take(&w.sta, nb * n.sta)) || (rc = w.take(&w.ev, nb * n.ev)) || (rc = w.take(&w.part, nb * n.part)) || (rc = w.take(&w.logz, nb * n.logz)) ||
            (rc = w.take(&w.sum, nb * n.sum)) || (rc = w.take(&w.loc, nb * n.loc)) || (rc = w.take(&w.marg, nb * n.marg)) || (rc = w.take(&w.prior, nb * n.prior)) ||
            (rc = w.take(&w.vol, nb * n.vol)) || (rc = w.take(&w.w, nb * n.w)) || (rc = w.take(&w.stack, n.stack)) || (rc = w.take(&w.xy, n.xy)) ||
            (rc = w.take(&w.xz, n.xz)) || (rc = w.take(&w.yz, n.yz)) || (rc = w.take(&w.tally, n.tally)) || (rc = w.take(&w.rbase, nb * n.rbase)) ||
            (rc = w.take(&w.rpart, nb * n.rpart)) || (rc = w.take(&w.res, nb * n.res)) || (rc = w.take(&w.fit, nb * n.fit)) || (rc = w.take(&w.org, nb * n.org)))
            return rc;
        if (n.layer && (rc = w.pool.upload(&w.layer, c.layer, n.layer))) return rc;
        if (n.stack) {
            HIPCHK(hipMemsetAsync(w.stack, 0, n.stack * sizeof(double), h->stream));
            HIPCHK(hipMemsetAsync(w.tally, 0, n.tally * sizeof(double), h->stream));
        }
        jb.sta = w.sta; jb.ev = w.ev; jb.prior = w.prior; jb.part = w.part; jb.vol = w.vol; jb.org = w.org; jb.S = c.rq.n_sta;
        return HTM_OK;
    }

    // the structure: one, into the handle's arrays and the job; or the draws' table (k_locate_pack_draws)
    int structure()
    {
        const int S = c.rq.n_sta, K = pl.K, Kpad = pl.Kpad;
        if (c.rq.job == kLocFixed) {
            HIPCHK(hipMemcpy(h->d_tc, c.t_corr, (size_t)S * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(h->d_ac, c.a_corr, (size_t)S * sizeof(double), hipMemcpyHostToDevice));
            jb.rbeta = 1.0 / *c.vs; jb.katt = (kPi * kFreq) / (*c.qs * *c.vs);          // as event_misfit forms them
            jb.rbeta32 = (float)jb.rbeta; jb.katt32 = (float)jb.katt;
            return HTM_OK;
        }
        // (the station records' tc and ac are not read on this path: k_locate_pack fills them from whatever the handle holds)
        const LocLengths &n = pl.len;
        std::vector<double> rk(n.rk);
        for (int k = 0; k < K; ++k) { rk[k] = 1.0 / c.vs[k]; rk[(size_t)K + k] = (kPi * kFreq) / (c.qs[k] * c.vs[k]); }
        double *d_dtc = nullptr, *d_dac = nullptr, *d_rk = nullptr;
        Pair *d_corr = nullptr, *d_vq = nullptr;
        int rc;
        if ((rc = w.pool.upload(&d_dtc, c.t_corr, n.dtc)) || (rc = w.pool.upload(&d_dac, c.a_corr, n.dac)) || (rc = w.pool.upload(&d_rk, rk.data(), n.rk)) ||
            (rc = w.pool.alloc(&d_corr, n.corr)) || (rc = w.pool.alloc(&d_vq, n.vq)))
            return rc;
        hipLaunchKernelGGL(k_locate_pack_draws<loc_real<F32>>, dim3((unsigned)((((long)S + 1) * Kpad + 255) / 256)), dim3(256), 0, h->stream, S, K, Kpad, d_dtc, d_dac, d_rk,
                           d_rk + K, d_corr, d_vq);
        dr.vq = d_vq; dr.corr = d_corr; dr.K = K; dr.Kpad = Kpad;
        return HTM_OK;
    }

    // the grid of event e: the call's, with the event's own origin where the call has boxes (what loc_grid_of does on the device)
    MapGrid grid_of(long e) const
    {
        MapGrid ge = pl.g;
        if (c.rq.boxes) { ge.x0 = c.origin3[3 * e]; ge.y0 = c.origin3[3 * e + 1]; ge.z0 = c.origin3[3 * e + 2]; }
        return ge;
    }

    // events e0 .. e0 + m - 1: the boxes' origins, the prior's tables, pack, evaluate, combine, stack, download
    int batch(long e0, long m)
    {
        const LocGrid &g = pl.g;
        const int S = c.rq.n_sta, K = pl.K, Kpad = pl.Kpad, job = c.rq.job;
        const long n_tiles = pl.n_tiles, cells = pl.cells, nm = pl.nm;
        const double log_cell = std::log(g.dx * g.dy * g.dz);
        const int mode = (h->dev.use_time ? 1 : 0) | (h->dev.use_amp ? 2 : 0);
        int rc;
        if (c.rq.boxes) {       // (the origins travel with the batch: event e0 + b is row b)
            org.assign((size_t)m * 4, 0.0);
            for (long b = 0; b < m; ++b)
                for (int a = 0; a < 3; ++a) org[(size_t)b * 4 + a] = c.origin3[3 * (e0 + b) + a];
            HIPCHK(hipMemcpy(w.org, org.data(), org.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if (c.rq.prior) {
            tab.resize((size_t)m * nm);
            for (long b = 0; b < m; ++b) locate_prior_tables(c.prior5 + 5 * (e0 + b), grid_of(e0 + b), tab.data() + (size_t)b * nm);
            HIPCHK(hipMemcpy(w.prior, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        hipLaunchKernelGGL(k_locate_pack, dim3((unsigned)((m * S + 255) / 256)), dim3(256), 0, h->stream, h->dev, (int)e0, (int)m, h->d_tc, h->d_ac,
                           h->d_lconst_t, h->d_lconst_a, w.sta, w.ev);
        const dim3 grid((unsigned)n_tiles, (unsigned)m), block(kLocThreads);
        with_mode(mode, [&](auto M) {
            constexpr int MODE = decltype(M)::value;
            if (job == kLocFixed) hipLaunchKernelGGL((k_locate<MODE, F32>), grid, block, 0, h->stream, g, jb);
            else if (job == kLocEvidence) hipLaunchKernelGGL((k_locate_draw_evidence<MODE, F32>), grid, block, 0, h->stream, g, jb, dr);
            else hipLaunchKernelGGL((k_locate_marginal<MODE, F32>), grid, block, 0, h->stream, g, jb, dr);
        });
        if (job == kLocEvidence)
            hipLaunchKernelGGL(k_locate_draw_combine, dim3((unsigned)m), dim3(256), 0, h->stream, (int)n_tiles, K, Kpad, w.part, log_cell, w.logz, w.sum);
        else
            hipLaunchKernelGGL(k_locate_combine, dim3((unsigned)m), dim3(256), 0, h->stream, g, w.part, log_cell, w.loc, w.marg, w.w, w.org);
        if (c.rq.n_layer)
            hipLaunchKernelGGL(k_locate_stack, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->stream, cells, (int)m, (int)e0, w.vol, w.loc, w.w, w.layer,
                               c.rq.n_layer, w.stack, w.tally);
        if (c.rq.residuals) {
            // the residual pass reads the batch's volume, loc records and weight sums where k_locate and k_locate_combine left them
            const LocRes rs{w.loc, w.w, w.rbase, w.rpart, w.res, w.fit, cells, (int)pl.n_rblk};
            with_mode(mode, [&](auto M) {
                constexpr int MODE = decltype(M)::value;
                hipLaunchKernelGGL((k_locate_res_best<MODE, F32>), dim3((unsigned)m), dim3(64), 0, h->stream, g, jb, rs);
                hipLaunchKernelGGL((k_locate_residuals<MODE, F32>), dim3((unsigned)pl.n_rblk, (unsigned)m), block, 0, h->stream, g, jb, rs);
            });
            hipLaunchKernelGGL(k_locate_res_combine, dim3((unsigned)m), dim3(256), 0, h->stream, rs, S, mode & 1, (mode >> 1) & 1);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        if (job == kLocEvidence) {
            if ((rc = w.pool.download(c.log_z + (size_t)e0 * K, w.logz, (size_t)m * K, "the draws' evidences'"))) return rc;
            if (c.summary && (rc = w.pool.download(c.summary + (size_t)e0 * 4, w.sum, (size_t)m * 4, "the draws' summary's"))) return rc;
            return HTM_OK;
        }
        if (c.loc && (rc = w.pool.download(c.loc + (size_t)e0 * 16, w.loc, (size_t)m * 16, "the locations'"))) return rc;
        if (c.marg && (rc = w.pool.download(c.marg + (size_t)e0 * nm, w.marg, (size_t)m * nm, "the marginals'"))) return rc;
        if (c.vol && (rc = w.pool.download(c.vol + (size_t)e0 * cells, w.vol, (size_t)m * cells, "the volume's"))) return rc;
        if (c.rq.residuals) {
            if ((rc = w.pool.download(c.res + (size_t)e0 * 4 * S, w.res, (size_t)m * 4 * S, "the residuals'"))) return rc;
            if ((rc = w.pool.download(c.fit + (size_t)e0 * 10, w.fit, (size_t)m * 10, "the fit's"))) return rc;
        }
        return HTM_OK;
    }

    // the stack's three maps (k_locate_stack_project) and its downloads
    int project()
    {
        const LocGrid &g = pl.g;
        const LocLengths &n = pl.len;
        const long nl = c.rq.n_layer;
        const long most = std::max(nl * std::max((long)g.nx * g.ny, (long)g.nx * g.nz), 64L * nl * g.ny * g.nz);
        const unsigned blocks = (unsigned)std::min((most + 255) / 256, 1L << 20);
        hipLaunchKernelGGL(k_locate_stack_project, dim3(blocks), dim3(256), 0, h->stream, g, c.rq.n_layer, w.stack, w.xy, w.xz, w.yz);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        int rc;
        if ((rc = w.pool.download(c.xy, w.xy, n.xy, "the xy map's")) || (rc = w.pool.download(c.xz, w.xz, n.xz, "the xz map's")) ||
            (rc = w.pool.download(c.yz, w.yz, n.yz, "the yz map's")) || (rc = w.pool.download(c.tally, w.tally, n.tally, "the tally's")))
            return rc;
        if (c.stack && (rc = w.pool.download(c.stack, w.stack, n.stack, "the stack's"))) return rc;
        return HTM_OK;
    }

    int run()
    {
        int rc = plan();
        if (rc) return rc;
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        if ((rc = workspace()) || (rc = structure())) return rc;
        const long E = c.rq.n_events;
        for (long e0 = 0; e0 < E; e0 += pl.nb)
            if ((rc = batch(e0, std::min(pl.nb, E - e0)))) return rc;
        return c.rq.n_layer ? project() : HTM_OK;
    }
};

// a call of that job on this handle; the entry points add their arguments by name
LocCall locate_call(const htm_forward *h, int job, int n_draws)
{
    LocCall c{};
    c.rq.n_sta = h->S; c.rq.n_events = h->E; c.rq.job = job; c.rq.n_draws = n_draws; c.rq.fp32 = h->loc_fp32;
    return c;
}

int locate_run(htm_forward *h, const LocCall &c)
{
    return c.rq.fp32 ? LocRun<true>(h, c).run() : LocRun<false>(h, c).run();
}

int locate_structure_ok(double vs, double qs)
{
    if (!std::isfinite(vs) || !std::isfinite(qs) || !(vs > 0.0) || !(qs > 0.0))
        return fail(HTM_EINVAL, "vs = %g, qs = %g: need finite values > 0", vs, qs);
    return HTM_OK;
}

// what the entry points over draws ask of them
int locate_draws_ok(int n_draws, const double *vs, const double *qs)
{
    if (n_draws < 1 || n_draws > kLocMaxDraws) return fail(HTM_EINVAL, "n_draws = %d: need 1..%d", n_draws, kLocMaxDraws);
    for (int k = 0; k < n_draws; ++k)
        if (!std::isfinite(vs[k]) || !std::isfinite(qs[k]) || !(vs[k] > 0.0) || !(qs[k] > 0.0))
            return fail(HTM_EINVAL, "draw %d: vs = %g, qs = %g: need finite values > 0", k, vs[k], qs[k]);
    return HTM_OK;
}

}  // namespace

// ====================================================================================================
extern "C" {

// The arithmetic of the locate entry points on this handle (include/htm_hip.h); step 5's switch is htm_forward_set_precision
int htm_forward_locate_set_precision(htm_forward *h, int forward_fp32)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    if (forward_fp32 != 0 && forward_fp32 != 1) return fail(HTM_EINVAL, "forward_fp32 = %d: need 0 (fp64) or 1 (fp32)", forward_fp32);
    h->loc_fp32 = forward_fp32 != 0;
    return HTM_OK;
}

// The plan of a call, without a handle or a device: htm_forward_locate_plan's request against what the entry points accept,
// then the very steps of LocRun::plan (all but the prior's widths, which are data)
int htm_forward_locate_plan(const htm_locate_request *request, const double *grid9, htm_locate_plan *plan)
{
    if (!request || !grid9 || !plan) return fail(HTM_EINVAL, "NULL argument");
    const htm_locate_request &r = *request;
    if (r.n_sta <= 0 || r.n_events <= 0) return fail(HTM_EINVAL, "n_sta and n_events must be positive");
    if (r.job != kLocFixed && r.job != kLocMarginal && r.job != kLocEvidence)
        return fail(HTM_EINVAL, "job = %d: need 0 (fixed structure), 1 (marginal over draws) or 2 (draw evidence)", r.job);
    if (r.job == kLocFixed ? r.n_draws != 0 : (r.n_draws < 1 || r.n_draws > kLocMaxDraws))
        return r.job == kLocFixed ? fail(HTM_EINVAL, "n_draws = %d under a fixed structure: need 0", r.n_draws)
                                  : fail(HTM_EINVAL, "n_draws = %d: need 1..%d", r.n_draws, kLocMaxDraws);
    if (r.n_layer < 0) return fail(HTM_EINVAL, "n_layer = %d: need at least 1, or 0 for no stack", r.n_layer);
    if (!r.layer && r.n_layer > 1) return fail(HTM_EINVAL, "n_layer = %d without a layer per window", r.n_layer);
    if (r.layer && r.n_layer == 0) return fail(HTM_EINVAL, "a layer per window without a stack (n_layer = 0)");
    if (r.job == kLocEvidence && (r.volume || r.n_layer)) return fail(HTM_EINVAL, "the draws' evidences come without a volume and without a stack");
    if (r.residuals && (r.job != kLocFixed || r.volume || r.n_layer))
        return fail(HTM_EINVAL, "the residuals come under a fixed structure, without a volume and without a stack");
    if (r.boxes && (r.job == kLocEvidence || r.n_layer || r.residuals))
        return fail(HTM_EINVAL, "a box per event comes under a fixed structure or its mixture over draws, without a stack and without residuals");
    const LocRequest rq{r.n_sta, r.n_events, r.job, r.n_draws, r.volume != 0, r.prior != 0, r.n_layer, r.layer != 0, r.forward_fp32 != 0, r.residuals != 0,
                        r.boxes != 0};
    LocPlan p;
    if (int rc = locate_tiles(grid9, &p)) return rc;
    double mb;
    if (int rc = env_mib("HTM_LOCATE_MB", 1024.0, &mb)) return rc;
    if (int rc = locate_budget(rq, mb, &p)) return rc;
    const LocLengths &n = p.len;
    *plan = htm_locate_plan{};
    plan->rows = p.g.rows; plan->tpl = p.g.tpl; plan->stride = p.g.stride;
    plan->cells = p.cells; plan->n_tiles = p.n_tiles; plan->n_marg = p.nm; plan->map_cells = p.map_cells;
    plan->n_draws = p.K; plan->n_draws_padded = p.Kpad;
#define LEN(a) plan->len_##a = (int64_t)n.a;
    LEN(sta) LEN(ev) LEN(part) LEN(logz) LEN(sum) LEN(loc) LEN(marg) LEN(prior) LEN(vol) LEN(w)
    LEN(dtc) LEN(dac) LEN(rk) LEN(corr) LEN(vq) LEN(stack) LEN(xy) LEN(xz) LEN(yz) LEN(tally) LEN(layer)
    plan->per_event_bytes = p.per_event; plan->table_bytes = p.table; plan->fixed_bytes = p.fixed;
    for (int i = 0; i < kLocLimits; ++i) plan->nb_limit[i] = p.limit[i];
    plan->nb = p.nb;
    LEN(rbase) LEN(rpart) LEN(res) LEN(fit) LEN(org)
#undef LEN
    return HTM_OK;
}

int htm_forward_locate(htm_forward *h, const double *t_corr, double vs, const double *a_corr, double qs, const double *grid9,
                       const double *prior5, double *loc, double *marg, double *vol)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    if (!t_corr || !a_corr || !grid9 || !loc) return fail(HTM_EINVAL, "NULL argument");
    if (int rc = locate_structure_ok(vs, qs)) return rc;
    LocCall c = locate_call(h, kLocFixed, 0);
    c.t_corr = t_corr; c.vs = &vs; c.a_corr = a_corr; c.qs = &qs;
    c.grid9 = grid9; c.prior5 = prior5; c.rq.prior = prior5 != nullptr;
    c.loc = loc; c.marg = marg; c.vol = vol; c.rq.volume = vol != nullptr;
    return locate_run(h, c);
}

// The stations' residuals, the source terms and the fit of every window (include/htm_hip.h): htm_forward_locate's
// call with the residual pass behind every batch's combine.  The batch volume is kept on the device and is not downloaded; loc and
// marg may be NULL
int htm_forward_locate_residuals(htm_forward *h, const double *t_corr, double vs, const double *a_corr, double qs, const double *grid9,
                                 const double *prior5, double *loc, double *marg, double *res, double *fit)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    if (!t_corr || !a_corr || !grid9) return fail(HTM_EINVAL, "NULL argument");
    if (int rc = locate_structure_ok(vs, qs)) return rc;
    if (!res || !fit) return fail(HTM_EINVAL, "NULL output: res and fit are required");
    LocCall c = locate_call(h, kLocFixed, 0);
    c.t_corr = t_corr; c.vs = &vs; c.a_corr = a_corr; c.qs = &qs;
    c.grid9 = grid9; c.prior5 = prior5; c.rq.prior = prior5 != nullptr;
    c.loc = loc; c.marg = marg;
    c.res = res; c.fit = fit; c.rq.residuals = true;
    return locate_run(h, c);
}

int htm_forward_locate_marginal(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr, const double *qs,
                                const double *grid9, const double *prior5, double *loc, double *marg, double *vol)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    if (!t_corr || !vs || !a_corr || !qs || !grid9 || !loc) return fail(HTM_EINVAL, "NULL argument");
    if (int rc = locate_draws_ok(n_draws, vs, qs)) return rc;
    LocCall c = locate_call(h, kLocMarginal, n_draws);
    c.t_corr = t_corr; c.vs = vs; c.a_corr = a_corr; c.qs = qs;
    c.grid9 = grid9; c.prior5 = prior5; c.rq.prior = prior5 != nullptr;
    c.loc = loc; c.marg = marg; c.vol = vol; c.rq.volume = vol != nullptr;
    return locate_run(h, c);
}

int htm_forward_locate_draw_evidence(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr, const double *qs,
                                     const double *grid9, const double *prior5, double *log_z, double *summary)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    if (!t_corr || !vs || !a_corr || !qs || !grid9 || !log_z) return fail(HTM_EINVAL, "NULL argument");
    if (int rc = locate_draws_ok(n_draws, vs, qs)) return rc;
    LocCall c = locate_call(h, kLocEvidence, n_draws);
    c.t_corr = t_corr; c.vs = vs; c.a_corr = a_corr; c.qs = qs;
    c.grid9 = grid9; c.prior5 = prior5; c.rq.prior = prior5 != nullptr;
    c.log_z = log_z; c.summary = summary;
    return locate_run(h, c);
}

// A box of its own per event (include/htm_hip.h): n_draws = 0 htm_forward_locate's structure (*vs, *qs), n_draws >= 1
// htm_forward_locate_marginal's, event e on grid9's cells from origin3[e]
int htm_forward_locate_boxes(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr, const double *qs,
                             const double *grid9, const double *origin3, const double *prior5, double *loc, double *marg, double *vol)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    if (!t_corr || !vs || !a_corr || !qs || !grid9 || !loc) return fail(HTM_EINVAL, "NULL argument");
    if (int rc = n_draws == 0 ? locate_structure_ok(*vs, *qs) : locate_draws_ok(n_draws, vs, qs)) return rc;
    if (!origin3) return fail(HTM_EINVAL, "NULL origin3: a box per event needs every event's origin");
    for (int e = 0; e < h->E; ++e)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(origin3[3 * (size_t)e + a]))
                return fail(HTM_EINVAL, "event %d: box origin %c = %g: need a finite value", e, "xyz"[a], origin3[3 * (size_t)e + a]);
    LocCall c = locate_call(h, n_draws == 0 ? kLocFixed : kLocMarginal, n_draws);
    c.t_corr = t_corr; c.vs = vs; c.a_corr = a_corr; c.qs = qs;
    c.grid9 = grid9; c.prior5 = prior5; c.rq.prior = prior5 != nullptr;
    c.origin3 = origin3; c.rq.boxes = true;
    c.loc = loc; c.marg = marg; c.vol = vol; c.rq.volume = vol != nullptr;
    return locate_run(h, c);
}

// The stacked density of the windows' posteriors (include/htm_hip.h): n_draws = 0 htm_forward_locate's
// structure (*vs, *qs), n_draws >= 1 htm_forward_locate_marginal's.  The batch volume is always on the device and is not
// downloaded; loc may be NULL
int htm_forward_locate_stack(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr, const double *qs,
                             const double *grid9, const double *prior5, const int *layer, int n_layer, double *loc, double *marg, double *xy,
                             double *xz, double *yz, double *stack, double *tally)
{
    if (!h) return fail(HTM_EINVAL, "NULL handle");
    if (!t_corr || !vs || !a_corr || !qs || !grid9) return fail(HTM_EINVAL, "NULL argument");
    if (int rc = n_draws == 0 ? locate_structure_ok(*vs, *qs) : locate_draws_ok(n_draws, vs, qs)) return rc;
    if (n_layer < 1) return fail(HTM_EINVAL, "n_layer = %d: need at least 1", n_layer);
    if (!layer && n_layer != 1) return fail(HTM_EINVAL, "n_layer = %d without a layer per window", n_layer);
    if (!xy || !xz || !yz || !tally) return fail(HTM_EINVAL, "NULL output: xy, xz, yz and tally are required");
    LocCall c = locate_call(h, n_draws == 0 ? kLocFixed : kLocMarginal, n_draws);
    c.t_corr = t_corr; c.vs = vs; c.a_corr = a_corr; c.qs = qs;
    c.grid9 = grid9; c.prior5 = prior5; c.rq.prior = prior5 != nullptr;
    c.layer = layer; c.rq.n_layer = n_layer; c.rq.layer = layer != nullptr;
    c.loc = loc; c.marg = marg;
    c.xy = xy; c.xz = xz; c.yz = yz; c.stack = stack; c.tally = tally;
    return locate_run(h, c);
}

}  // extern "C"
