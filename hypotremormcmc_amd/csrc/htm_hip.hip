// htm_hip.hip -- the chain sets' part of the C ABI (include/htm_hip.h): htm_chains_* and htm_comm_*.  (The forward model's part
// is htm_forward.hip, the other steps' htm_steps.hip; this file keeps its name because most of it stayed where it was.)  Sets a chain set up from
// its launch plan (htm_plan.hpp: which chain-master loop a launch takes, and its shape) and looks the loop's kernel up in the table of htm_host.hpp; the instantiations themselves are
// compiled by the loop units (htm_loop_*.hip), none here.  This unit owns the small kernels of htm_chains_kernels.hpp.  From the loops it takes
// sizes only: FlowShared, MbShared and kXSlots (htm_flow.hpp, through htm_chains_kernels.hpp), PipeShared and pipe_ring_bytes (htm_pipe.hpp),
// mcmc_threads (htm_mcmc.hpp); the barrier loop's StepSharedT is htm_handoff.hpp's, so htm_step.hpp is not needed.
#include "htm_host.hpp"
#include "htm_chains_kernels.hpp"
#include "htm_pipe.hpp"
#include "htm_mcmc.hpp"

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

using namespace htm;

namespace htm {

// ---- the kernel table's two lookups (htm_host.hpp): the rows of every loop unit -------------------------------------------
// Three or more stations per lane run the instantiation for any station count (<0, ..>), as they always have; the fp32
// forward and the masters of htm_flow.hpp / htm_pipe.hpp other than MK 3 and 4 exist for one or two stations per lane only.
static const LoopKernel *find_row(bool step, bool wide, int nch, bool fp32, int mk)
{
    const int n = (nch == 1 || nch == 2) ? nch : 0;
    const LoopRows units[] = {loop_rows_free(), loop_rows_lock(), loop_rows_barrier(), loop_rows_wide(), loop_rows_pipe()};
    for (const LoopRows &u : units)
        for (size_t k = 0; k < u.n; ++k) {
            const LoopRow &r = u.rows[k];
            if (r.step == step && r.wide == wide && r.nch == n && r.fp32 == fp32 && r.mk == mk) return &r.k;
        }
    return nullptr;
}
const LoopKernel *mcmc_kernel(int nch, bool fp32, int mk, bool wide) { return find_row(false, wide, nch, fp32, mk); }
const LoopKernel *step_kernel(int nch, bool fp32, bool wide) { return find_row(true, wide, nch, fp32, 0); }

static int no_kernel(const htm_chains *hc, const char *what, int mk)
{
    return fail(HTM_EINVAL, "no %s kernel is built for %d stations with the %s forward%s (loop %d)", what, hc->fwd->S,
                hc->fwd->dev.fp32 ? "fp32" : "fp64", hc->plan.wide ? ", more than 32 chains" : "", mk);
}

int launch_mcmc(htm_chains *hc, int mode, int target, const double *gathered)
{
    htm_forward *h = hc->fwd;
    const LoopPlan &lp = hc->plan;
    hc->ctrl_fresh = false;
    // one instantiation per main loop (MK, htm_mcmc.hpp k_mcmc); the step log can be switched on after htm_chains_create
    const int mk = loop_for(lp, mode, hc->h_ctrl.slog_cap != 0);
    LoopLaunch l{};
    l.grid = dim3((mk == 7 ? lp.mb_blocks : 1) + hc->dev.n_workers);
    l.smem = lp.step_smem; l.stream = h->stream; l.f = &h->dev; l.cs = &hc->dev;
    l.mode = mode; l.target = target; l.gathered = gathered; l.ring_size = lp.ring_size; l.wmax = lp.wmax;
    l.seq = ++hc->launch_seq;      // this chain set's k_mcmc launches, counted from 1
    if (mk == 8 && !h->dev.obs_pack) return fail(HTM_EINVAL, "the specialised chain master needs the forward's packed records");
    const LoopKernel *k = mcmc_kernel(h->nch, h->dev.fp32 != 0, mk, lp.wide);
    if (!k) return no_kernel(hc, "k_mcmc", mk);
    // (the specialised master's chain wave keeps its chain's correction pair in registers, htm_flow.hpp FlowOwn: a wave per chain)
    if (mk == 8 && hc->dev.n_chains > std::min(k->threads / 64, 8))
        return fail(HTM_EINVAL, "the specialised chain master runs one chain per wave: %d chains, %d threads", hc->dev.n_chains, k->threads);
    if (mode == MODE_RUN) hc->last_fixed = mk == 8;
    if (mk == 5 || mk == 6) { l.smem = lp.pipe_smem; l.ring_size = lp.pipe_ring; }      // (its own LDS layout and stream window)
    // several master workgroups: what their chains share lives in memory (MbShared), set up by a one-wave kernel first
    if (mk == 7) hipLaunchKernelGGL(k_mb_init, dim3(1), dim3(64), 0, h->stream, hc->dev, target);
    l.block = dim3(k->threads);
    k->launch(l);
    HIPCHK(hipGetLastError());
    return HTM_OK;
}

int launch_step(htm_chains *hc, int mode, int target, const double *gathered)
{
    htm_forward *h = hc->fwd;
    hc->ctrl_fresh = false;
    const LoopKernel *k = step_kernel(h->nch, h->dev.fp32 != 0, hc->plan.wide);
    if (!k) return no_kernel(hc, "k_step", 0);
    LoopLaunch l{};
    l.grid = dim3(1); l.block = dim3(64 * hc->plan.nw);
    l.smem = hc->plan.step_smem; l.stream = h->stream; l.f = &h->dev; l.cs = &hc->dev_np;
    l.mode = mode; l.target = target; l.gathered = gathered; l.ring_size = hc->plan.ring_size; l.wmax = hc->plan.wmax;
    k->launch(l);
    HIPCHK(hipGetLastError());
    return HTM_OK;
}
}  // namespace htm

namespace {

// Append n (multiple of 64) positions to the rank's random stream on the side stream.  Asynchronous; the
// new coverage is published to the device (StreamDev::hop_end) by the last kernel of the sequence.
int stream_produce(htm_chains *hc, long long n)
{
    if (n <= 0) return HTM_OK;
    n = (n + 63) / 64 * 64;
    const StreamDev &sd = hc->dev.stream;
    // never overwrite positions that may still be needed: everything from (consumed - 4) on
    const long long room = hc->cap - (hc->n_raw - (hc->spos_lo - 4));
    if (n > room) n = room / 64 * 64;
    if (n <= 0) return HTM_OK;
    hipStream_t st = hc->side;
    hipLaunchKernelGGL(k_rawgen, dim3((unsigned)((n + 4095) / 4096)), dim3(64), 0, st, sd, hc->n_raw, (int)n, hc->d_jump,
                       sd.gen + 4 * hc->gen_par, sd.gen + 4 * (hc->gen_par ^ 1));
    hc->gen_par ^= 1;
    hc->n_raw += n;
    auto blocks = [](long long cnt) { return dim3((unsigned)((cnt + 255) / 256)); };
    long long e = hc->n_raw - 1;
    if (e > hc->n_tr) { hipLaunchKernelGGL(k_stream_tr, blocks(e - hc->n_tr), dim3(256), 0, st, sd, hc->n_tr, e); hc->n_tr = e; }
    e = hc->n_tr - kRecLag;
    if (e > hc->n_rec) {
        hipLaunchKernelGGL(k_stream_rec, blocks(e - hc->n_rec), dim3(256), 0, st, sd, hc->n_rec, e, hc->th[0], hc->th[1],
                           hc->th[2], hc->th[3], hc->dev.S, hc->dev.E, hc->dev.n_procs, hc->dev.n_chains);
        hc->n_rec = e;
    }
    e = hc->n_rec - kHopLag;
    if (e > hc->n_hop) { hipLaunchKernelGGL(k_stream_hop, blocks(e - hc->n_hop), dim3(256), 0, st, sd, hc->n_hop, e); hc->n_hop = e; }
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, st, sd.hop_end, hc->n_hop);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(hc->ev_side, st));
    return HTM_OK;
}

FullJob chain_full_job(htm_chains *hc)
{
    FullJob jb{};
    const ChainsDev &d = hc->dev_np;
    jb.hypo = d.hypo.x; jb.hypo_stride = d.hypo.nx;
    jb.tc = d.tc.x; jb.tc_stride = d.S;
    jb.ac = d.ac.x; jb.ac_stride = d.S;
    jb.vs = d.vs.x; jb.qs = d.qs.x;
    jb.desc = d.desc;
    jb.n_models = d.n_chains;
    jb.partial = d.partial; jb.n_wg = hc->fwd->n_wg; jb.epw = hc->fwd->epw;
    return jb;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// chains
// ---------------------------------------------------------------------------------------------------
namespace {

static_assert(MODE_RUN == kPlanModeRun && MODE_ADVANCE == kPlanModeAdvance && MODE_LOCKRUN == kPlanModeLockrun,
              "htm_plan.hpp and htm_device.hpp disagree on the modes");

// Owns a handle under construction: every early return of htm_chains_create and of the functions it calls destroys what was
// made so far (htm_chains_destroy tolerates a half-built handle); released on success.
struct ChainsGuard {
    htm_chains *hc;
    ~ChainsGuard() { if (hc) htm_chains_destroy(hc); }
    htm_chains *release() { htm_chains *p = hc; hc = nullptr; return p; }
};

PlanSizes plan_sizes(int nc)
{
    PlanSizes s;
    s.flow_shared = sizeof(FlowShared); s.wide_shared = sizeof(StepSharedT<kMaxWideChains>); s.pipe_shared = sizeof(PipeShared);
    s.pipe_ring_bytes = pipe_ring_bytes(nc);
    s.gath_stage = kGathStage; s.hops = kHops; s.pipe_threads_nch1 = mcmc_threads<1, 5>();
    s.max_chains = kMaxChains; s.gran_per_slot = kGranPerSlot; s.max_slot_replicas = kMaxSlotReplicas;
    return s;
}

void export_plan(const LoopPlan &lp, int n_workers, int mirror_n, int mirror_steps, int nch, bool fp32, htm_launch_plan *o)
{
    *o = htm_launch_plan{};
    o->persist = lp.persist; o->flow = lp.flow; o->flow_fixed = lp.flow_fixed; o->wide = lp.wide; o->flow_lock = lp.flow_lock;
    o->mb_blocks = lp.mb_blocks; o->pipe = lp.pipe; o->pipe_lock = lp.pipe_lock; o->pipe_smem = (int64_t)lp.pipe_smem;
    o->pipe_ring = lp.pipe_ring; o->ring_size = lp.ring_size; o->wmax = lp.wmax; o->step_smem = (int64_t)lp.step_smem;
    o->worker_cap = lp.worker_cap; o->blocks_fit = lp.blocks_fit; o->nw = lp.nw;
    o->n_workers = n_workers; o->mirror_n = mirror_n; o->mirror_steps = mirror_steps;
    const int modes[3] = {MODE_RUN, MODE_ADVANCE, MODE_LOCKRUN};
    for (int m = 0; m < 3; ++m)
        for (int s = 0; s < 2; ++s) {
            o->loop[m][s] = loop_for(lp, modes[m], s != 0);
            o->loop_built[m][s] = mcmc_kernel(nch, fp32, (int)o->loop[m][s], lp.wide) ? 1 : 0;
        }
}

// one group of the rank's parameter vector: a window [off, off + nx*nc) of the five per-field allocations
int upload_model(htm_chains *hc, ModelDev &m, const htm_model_init &in, int nx, int nc, size_t off, const char *name)
{
    if (!in.x) return fail(HTM_EINVAL, "%s.x is NULL", name);
    const size_t n = (size_t)nx * nc;
    std::vector<double> zeros(n, 0.0);
    std::vector<double> ones(n, 1.0);
    std::vector<int32_t> izeros(n, 0);
    const ChainsDev &d = hc->dev;
    m.nx = nx;
    m.x = d.xall + off; m.mu = d.muall + off; m.sigma = d.sgall + off; m.step = d.stall + off; m.ptype = d.ptall + off;
    HIPCHK(hipMemcpy(m.x, in.x, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.mu, in.mu ? in.mu : zeros.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.sigma, in.sigma ? in.sigma : ones.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.step, in.step_size ? in.step_size : zeros.data(), n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.ptype, in.prior_type ? in.prior_type : izeros.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    return HTM_OK;
}

// ---- what htm_chains_create allocates and uploads, group by group.  Each returns at its first failure; the caller's guard
// ---- frees what was made.
int alloc_params(htm_chains *hc, const htm_chains_init *init, const Knobs &kn)
{
    htm_forward *h = hc->fwd;
    ChainsDev &d = hc->dev;
    const int nc = d.n_chains;
    int rc;
    // [vs | t_corr | qs | a_corr | hypo], the order of the proposal types (chain_pass computes these offsets too)
    const size_t S = (size_t)h->S, E = (size_t)h->E, n = (size_t)nc;
    const size_t total = 2 * n + 2 * n * S + 3 * E * n;
    if ((rc = dev_alloc(hc->pool, &d.xall, total)) || (rc = dev_alloc(hc->pool, &d.muall, total)) ||
        (rc = dev_alloc(hc->pool, &d.sgall, total)) || (rc = dev_alloc(hc->pool, &d.stall, total)) ||
        (rc = dev_alloc(hc->pool, &d.ptall, total))) return rc;
    if ((rc = upload_model(hc, d.vs, init->vs, 1, nc, 0, "vs"))) return rc;
    if ((rc = upload_model(hc, d.tc, init->t_corr, h->S, nc, n, "t_corr"))) return rc;
    if ((rc = upload_model(hc, d.qs, init->qs, 1, nc, n + n * S, "qs"))) return rc;
    if ((rc = upload_model(hc, d.ac, init->a_corr, h->S, nc, 2 * n + n * S, "a_corr"))) return rc;
    if ((rc = upload_model(hc, d.hypo, init->hypo, 3 * h->E, nc, 2 * n + 2 * n * S, "hypo"))) return rc;
    {
        std::vector<double> sg(total), r2(total);
        HIPCHK(hipMemcpy(sg.data(), d.sgall, total * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < total; ++k) r2[k] = 1.0 / (2.0 * sg[k] * sg[k]);
        if ((rc = dev_upload(hc->pool, &d.rs2all, r2.data(), total))) return rc;
        // the packed records the chain steps read (PriorRec), and whether every chain has chain 0's
        std::vector<double> mu(total), stp(total);
        std::vector<int32_t> pt(total);
        HIPCHK(hipMemcpy(mu.data(), d.muall, total * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(stp.data(), d.stall, total * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pt.data(), d.ptall, total * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<PriorRec> pr(total);
        for (size_t k = 0; k < total; ++k) { pr[k].mu = mu[k]; pr[k].rs2 = r2[k]; pr[k].step = stp[k]; pr[k].ptype = pt[k]; pr[k].pad = 0; }
        bool same = true;
        const size_t goffs[5] = {0, n, n + n * S, 2 * n + n * S, 2 * n + 2 * n * S}, gnx[5] = {1, S, 1, S, 3 * E};
        for (int gi = 0; gi < 5 && same; ++gi)
            for (size_t c = 1; c < n && same; ++c)
                same = memcmp(&pr[goffs[gi] + c * gnx[gi]], &pr[goffs[gi]], gnx[gi] * sizeof(PriorRec)) == 0;
        if (!kn.prior_same) same = false;      // (diagnostics: every chain reads its own records)
        PriorRec *dp = nullptr;
        if ((rc = dev_upload(hc->pool, &dp, pr.data(), total))) return rc;
        d.prior = dp; d.prior_same = same ? 1 : 0;
    }
    d.rayleigh14 = 0;
    auto any_rayleigh = [](const htm_model_init &m, size_t cnt) {
        if (!m.prior_type) return false;
        for (size_t k = 0; k < cnt; ++k) if (m.prior_type[k] == 1) return true;
        return false;
    };
    if (any_rayleigh(init->vs, n) || any_rayleigh(init->qs, n) || any_rayleigh(init->t_corr, n * S) ||
        any_rayleigh(init->a_corr, n * S)) d.rayleigh14 = 1;
    return HTM_OK;
}

int alloc_chain_state(htm_chains *hc, const htm_chains_init *init)
{
    htm_forward *h = hc->fwd;
    ChainsDev &d = hc->dev;
    const int nc = d.n_chains;
    int rc;
    if ((rc = dev_upload(hc->pool, &d.temp, init->temp, nc))) return rc;
    std::vector<double> L0(nc, -9.e+300);   // cls_mcmc.f90:88
    if ((rc = dev_upload(hc->pool, &d.L, L0.data(), nc))) return rc;
    std::vector<int32_t> z7(7 * (size_t)nc, 0);
    if ((rc = dev_upload(hc->pool, &d.n_propose, z7.data(), z7.size()))) return rc;
    if ((rc = dev_upload(hc->pool, &d.n_accept, z7.data(), z7.size()))) return rc;
    // proposal probabilities, cls_mcmc.f90:91-106, and the cumulative sums of :139-153 in the same order
    const double p_vs = init->solve_vs ? 0.025 : 0.0, p_tc = init->solve_t_corr ? 0.025 : 0.0;
    const double p_qs = init->solve_qs ? 0.025 : 0.0, p_ac = init->solve_a_corr ? 0.025 : 0.0;
    d.th1 = p_vs; d.th2 = p_vs + p_tc; d.th3 = p_vs + p_tc + p_qs; d.th4 = p_vs + p_tc + p_qs + p_ac;
    d.n_burn = init->n_burn; d.n_interval = init->n_interval;
    if ((rc = dev_alloc(hc->pool, &d.prop, nc))) return rc;
    HIPCHK(hipMemset(d.prop, 0, nc * sizeof(Proposal)));
    if ((rc = dev_alloc(hc->pool, &d.desc, 1))) return rc;
    HIPCHK(hipMemset(d.desc, 0, sizeof(FullDesc)));
    if ((rc = dev_alloc(hc->pool, &d.partial, (size_t)nc * std::max(h->n_wg, 256)))) return rc;      // (<= 256 workers whatever the launch shape)
    if ((rc = dev_alloc(hc->pool, &d.ps, 1))) return rc;
    HIPCHK(hipMemset(d.ps, 0, sizeof(PSync)));
    return HTM_OK;
}

// the control block: last, as it always was (the groups allocate in the order htm_chains_create has always allocated in, so
// that a chain set's buffers lie where they lay)
int upload_ctrl(htm_chains *hc)
{
    Ctrl c{};
    c.spos = 0;
    c.stage = ST_IDLE;
    hc->h_ctrl = c;
    return dev_upload(hc->pool, &hc->dev.ctrl, &c, 1);
}

// the hand-off area between the master's chain waves and the worker blocks (its geometry: the plan), and the
// swap record that the rank hands to the other ranks
int alloc_handoff(htm_chains *hc)
{
    ChainsDev &d = hc->dev;
    const int nc = d.n_chains;
    int rc;
    if ((rc = dev_alloc(hc->pool, &d.slots, (size_t)d.slot_rep * d.slot_stride))) return rc;
    HIPCHK(hipMemset(d.slots, 0, (size_t)d.slot_rep * d.slot_stride * sizeof(unsigned long long)));
    unsigned long long *mbw = nullptr;
    if ((rc = dev_alloc(hc->pool, &mbw, sizeof(MbShared) / sizeof(unsigned long long)))) return rc;
    d.mb = reinterpret_cast<MbShared *>(mbw);
    if ((rc = dev_alloc(hc->pool, &d.prev_mid, (size_t)nc))) return rc;
    HIPCHK(hipMemset(d.prev_mid, 0, (size_t)nc * sizeof(int)));
    if ((rc = dev_alloc(hc->pool, &d.lo_gran, (size_t)nc * 16))) return rc;
    HIPCHK(hipMemset(d.lo_gran, 0, (size_t)nc * 16 * sizeof(unsigned long long)));
    if ((rc = dev_alloc(hc->pool, &d.pgran, (size_t)nc * 256 * d.pgran_stride))) return rc;
    HIPCHK(hipMemset(d.pgran, 0, (size_t)nc * 256 * d.pgran_stride * sizeof(unsigned long long)));
    if ((rc = dev_alloc(hc->pool, &d.swap_rec, 4 + 2 * (size_t)nc))) return rc;
    HIPCHK(hipMemset(d.swap_rec, 0, (4 + 2 * (size_t)nc) * sizeof(double)));
    return HTM_OK;
}

int alloc_records(htm_chains *hc, const htm_chains_init *init)
{
    htm_forward *h = hc->fwd;
    ChainsDev &d = hc->dev;
    const int nc = d.n_chains;
    int rc;
    hc->rec_len = 3 * h->E + 2 * h->S + 2;
    d.cap_lik = init->lik_capacity > 0 ? init->lik_capacity : 1 << 16;
    if (init->sample_capacity > 0) d.cap_smp = init->sample_capacity;
    else d.cap_smp = (int)std::max<size_t>(4 * (size_t)nc, std::min<size_t>(4096, (size_t(128) << 20) / (hc->rec_len * sizeof(double))));
    if (d.cap_lik < 2 * nc || d.cap_smp < 2 * nc) return fail(HTM_EINVAL, "record capacities must be >= 2*n_chains");
    if ((rc = dev_alloc(hc->pool, &d.lik_iter, d.cap_lik))) return rc;
    if ((rc = dev_alloc(hc->pool, &d.lik_chain, d.cap_lik))) return rc;
    if ((rc = dev_alloc(hc->pool, &d.lik_val, d.cap_lik))) return rc;
    if ((rc = dev_alloc(hc->pool, &d.smp_iter, d.cap_smp))) return rc;
    if ((rc = dev_alloc(hc->pool, &d.smp_chain, d.cap_smp))) return rc;
    if ((rc = dev_alloc(hc->pool, &d.smp_data, (size_t)d.cap_smp * hc->rec_len))) return rc;
    d.slog_i = nullptr; d.slog_d = nullptr;
    // (and the diagnostic words: ChainsDev::diag, the phase stamps of a diagnostic build)
    if ((rc = dev_alloc(hc->pool, &d.diag, 32))) return rc;
    HIPCHK(hipMemset(d.diag, 0, 32 * sizeof(unsigned long long)));
    d.stamps = nullptr;
#ifdef HTM_STAMPS
    if ((rc = dev_alloc(hc->pool, &d.stamps, 128 + 2 * 8192))) return rc;      // (+ the event trace of htm_pipe.hpp)
    HIPCHK(hipMemset(d.stamps, 0, (128 + 2 * 8192) * sizeof(unsigned long long)));
#endif
    return HTM_OK;
}

// random-stream service: hc->cap positions of every table (htm_stream.hpp), the generator state and its jump table
int alloc_stream(htm_chains *hc, const htm_chains_init *init)
{
    ChainsDev &d = hc->dev;
    int rc;
    hc->th[0] = d.th1; hc->th[1] = d.th2; hc->th[2] = d.th3; hc->th[3] = d.th4;
    for (int k = 0; k < 4; ++k) hc->init_state[k] = init->rng_state[k];
    StreamDev &sd = d.stream;
    const size_t n = (size_t)hc->cap;
    sd.mask = hc->cap - 1;
    if ((rc = dev_alloc(hc->pool, &sd.raw, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.U, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.LOGU, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.G, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.pg, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.pr, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.plogr, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.dec, n))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.hop, n * kHops))) return rc;
    if ((rc = dev_alloc(hc->pool, &sd.sw, n))) return rc;
    uint32_t g8[8] = {hc->init_state[0], hc->init_state[1], hc->init_state[2], hc->init_state[3], 0, 0, 0, 0};
    if ((rc = dev_upload(hc->pool, &sd.gen, g8, 8))) return rc;
    hc->gen_par = 0;
    const std::vector<Mat128> &P = xs_powers();
    std::vector<u32x4> jt((size_t)kJumpLevels * 128);
    for (int b = 0; b < kJumpLevels; ++b)
        for (int j = 0; j < 128; ++j) {
            const Bits128 &c = P[6 + b][j];
            jt[(size_t)b * 128 + j] = u32x4{c.w[0], c.w[1], c.w[2], c.w[3]};
        }
    if ((rc = dev_upload(hc->pool, &hc->d_jump, jt.data(), jt.size()))) return rc;
    const long long zero = 0;
    return dev_upload(hc->pool, &sd.hop_end, &zero, 1);
}

int create_events(htm_chains *hc)
{
    hipError_t e1 = hipStreamCreateWithFlags(&hc->side, hipStreamNonBlocking);
    hipError_t e2 = hipEventCreateWithFlags(&hc->ev_side, hipEventDisableTiming);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(HTM_EHIP, "side stream/event creation failed");
    if (hipEventCreateWithFlags(&hc->ev_wd, hipEventDisableTiming) != hipSuccess) return fail(HTM_EHIP, "hipEventCreate failed");
    if (hipEventCreate(&hc->ev0) != hipSuccess || hipEventCreate(&hc->ev1) != hipSuccess) return fail(HTM_EHIP, "hipEventCreate failed");
    return HTM_OK;
}

// What phase B of the plan needs from the device (PlanDevice).  A kernel that is to be launched with more than 48 KiB of
// dynamic LDS has its limit raised here, before its occupancy is asked.
int device_facts(htm_chains *hc, const Plan &a, const PlanJob &job, const Knobs &kn, PlanDevice *f)
{
    htm_forward *h = hc->fwd;
    const bool fp32 = h->dev.fp32 != 0, wide = a.loop.wide;
    const size_t smem = a.loop.step_smem;
    if (smem > 48 * 1024) {
        const LoopKernel *ks = step_kernel(h->nch, fp32, wide);
        if (!ks) return no_kernel(hc, "k_step", 0);
        HIPCHK(hipFuncSetAttribute(ks->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    }
    if (!a.loop.persist) return HTM_OK;
    // every loop a launch of this chain set can take (loop_for); several master workgroups (MK 7) and the free-running
    // master specialised on the job's shape (MK 8) exist for one or two stations per lane
    std::vector<int> mks = {0, 1, 2};
    if (!wide) { mks.push_back(3); mks.push_back(4); }
    if (!wide && (h->nch == 1 || h->nch == 2)) { mks.push_back(7); mks.push_back(8); }
    // the residency bound holds for whichever main loop gets launched: the smallest of the instantiations' occupancies
    std::vector<const void *> fns;
    for (int mk : mks) {
        const LoopKernel *k = mcmc_kernel(h->nch, fp32, mk, wide);
        if (!k) return no_kernel(hc, "k_mcmc", mk);
        fns.push_back(k->fn);
    }
    if (smem > 48 * 1024)
        for (const void *g : fns) HIPCHK(hipFuncSetAttribute(g, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    int per_cu = 1 << 20;
    for (const void *g : fns) {
        int pc = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, g, 512, smem));
        per_cu = std::min(per_cu, pc);
    }
    HIPCHK(hipDeviceGetAttribute(&f->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    f->blocks_per_cu = per_cu;
    // the pipelined master's two loops, when one is asked for and the persistent launch stands (which these facts decide)
    Plan r = a;
    plan_residency(r, job, kn, *f);
    if (!a.pipe_asked || !r.loop.persist) return HTM_OK;
    for (int lk = 5; lk <= 6; ++lk) {
        const LoopKernel *pk = mcmc_kernel(h->nch, fp32, lk, false);
        if (!pk) return no_kernel(hc, "k_mcmc", lk);
        if (a.pipe_smem_want > 48 * 1024) HIPCHK(hipFuncSetAttribute(pk->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.pipe_smem_want));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&f->pipe_blocks_per_cu[lk - 5], pk->fn, a.pipe_threads, a.pipe_smem_want));
    }
    return HTM_OK;
}

}  // namespace

// ====================================================================================================
extern "C" {

int htm_chains_plan(const htm_plan_job *job, const htm_plan_device *device, htm_launch_plan *plan)
{
    if (!job || !device || !plan) return fail(HTM_EINVAL, "NULL argument");
    if (job->n_chains < 1 || job->n_chains > HTM_MAX_CHAINS)
        return fail(HTM_EINVAL, "n_chains must be in 1..%d (HTM_MAX_CHAINS), got %d", HTM_MAX_CHAINS, job->n_chains);
    if (job->n_procs < 1) return fail(HTM_EINVAL, "bad rank/n_procs");
    if (job->n_sta <= 0 || job->n_events <= 0) return fail(HTM_EINVAL, "n_sta and n_events must be positive");
    PlanJob j;
    j.nc = job->n_chains; j.n_procs = job->n_procs; j.S = job->n_sta; j.E = job->n_events; j.nch = nch_for(job->n_sta);
    j.fp32 = job->forward_fp32 != 0; j.use_time = job->use_time != 0; j.use_amp = job->use_amp != 0;
    if (j.fp32 && j.nch != 1 && j.nch != 2) return fail(HTM_EINVAL, "the fp32 forward covers n_sta <= 128 (this handle has %d stations)", j.S);
    const Knobs kn = read_knobs();
    const Plan a = plan_phase_a(j, kn, plan_sizes(j.nc));
    if (a.refused[0]) return fail(HTM_EINVAL, "%s", a.refused);
    PlanDevice f;
    f.n_cu = device->n_cu; f.blocks_per_cu = device->blocks_per_cu;
    f.pipe_blocks_per_cu[0] = device->pipe_blocks_per_cu[0]; f.pipe_blocks_per_cu[1] = device->pipe_blocks_per_cu[1];
    const Plan p = plan_phase_b(a, j, kn, f);
    export_plan(p.loop, p.n_workers, p.mirror_n, p.mirror_steps, j.nch, j.fp32, plan);
    return HTM_OK;
}

int htm_chains_get_plan(htm_chains *hc, htm_launch_plan *plan, htm_plan_device *seen)
{
    if (!hc || !plan) return fail(HTM_EINVAL, "NULL argument");
    export_plan(hc->plan, hc->dev.n_workers, hc->dev.mirror_n, hc->dev.mirror_steps, hc->fwd->nch, hc->fwd->dev.fp32 != 0, plan);
    if (seen) {
        seen->n_cu = hc->seen.n_cu; seen->blocks_per_cu = hc->seen.blocks_per_cu;
        seen->pipe_blocks_per_cu[0] = hc->seen.pipe_blocks_per_cu[0]; seen->pipe_blocks_per_cu[1] = hc->seen.pipe_blocks_per_cu[1];
    }
    return HTM_OK;
}

int htm_chains_create(htm_forward *h, const htm_chains_init *init, htm_chains **out)
{
    if (!out) return fail(HTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (!h || !init) return fail(HTM_EINVAL, "NULL argument");
    const int nc = init->n_chains;
    static_assert(HTM_MAX_CHAINS == kMaxWideChains, "include/htm_hip.h and htm_device.hpp disagree on the chain limit");
    if (nc < 1 || nc > HTM_MAX_CHAINS) return fail(HTM_EINVAL, "n_chains must be in 1..%d (HTM_MAX_CHAINS), got %d", HTM_MAX_CHAINS, nc);
    if (init->n_procs < 1 || init->rank < 0 || init->rank >= init->n_procs) return fail(HTM_EINVAL, "bad rank/n_procs");
    if (init->n_interval < 1) return fail(HTM_EINVAL, "n_interval must be >= 1");
    if (!init->temp) return fail(HTM_EINVAL, "temp is NULL");
    HIPCHK(hipSetDevice(h->device));

    const Knobs kn = read_knobs();
    PlanJob job;
    job.nc = nc; job.n_procs = init->n_procs; job.S = h->S; job.E = h->E; job.nch = h->nch;
    job.fp32 = h->dev.fp32 != 0; job.use_time = h->dev.use_time != 0; job.use_amp = h->dev.use_amp != 0;
    const Plan a = plan_phase_a(job, kn, plan_sizes(nc));

    ChainsGuard guard{new htm_chains()};
    htm_chains *hc = guard.hc;
    hc->fwd = h;
    hc->plan = a.loop;
    hc->cap = a.stream_cap;
    ChainsDev &d = hc->dev;
    d.n_chains = nc; d.n_procs = init->n_procs; d.rank = init->rank; d.S = h->S; d.E = h->E;
    d.n_wg = h->n_wg;
    d.n_workers = a.n_workers; d.mirror_n = a.mirror_n; d.mirror_steps = a.mirror_steps;
    d.slot_rep = a.slot_rep; d.slot_stride = a.slot_stride; d.pgran_stride = a.pgran_stride; d.npoll = a.npoll;
    d.dbg = kn.dbg; d.xwait_ticks = kn.xwait_ticks; d.dbg_xfail_iter = kn.xfail_iter; d.xown = kn.xown;

    int rc;
    if ((rc = alloc_params(hc, init, kn))) return rc;
    if ((rc = alloc_chain_state(hc, init))) return rc;
    if ((rc = alloc_handoff(hc))) return rc;
    if ((rc = alloc_records(hc, init))) return rc;
    if ((rc = alloc_stream(hc, init))) return rc;
    if ((rc = create_events(hc))) return rc;
    if ((rc = upload_ctrl(hc))) return rc;
    // (where the LDS budget has always been checked: after the arguments that the allocations above look at)
    if (a.refused[0]) return fail(HTM_EINVAL, "%s", a.refused);

    hc->dev_np = hc->dev;                       // same state; partial sums laid out per k_full tile, the worker count before its residency cap
    if ((rc = device_facts(hc, a, job, kn, &hc->seen))) return rc;
    const Plan p = plan_phase_b(a, job, kn, hc->seen);
    hc->plan = p.loop;
    d.n_workers = p.n_workers;
    d.n_wg = d.n_workers;                       // persistent kernel: one partial per worker block
    // (the specialised master's steps read an event's observations from one packed record: built here, once per forward and precision)
    if (p.loop.flow_fixed) {
        h->pack_wanted = true;
        if ((rc = ensure_obs_pack(h))) return rc;
    }
    // first stretch of the random stream (synchronous)
    if ((rc = stream_produce(hc, 1 << 16))) return rc;
    HIPCHK(hipStreamSynchronize(hc->side));
    *out = guard.release();
    return HTM_OK;
}

int htm_chains_destroy(htm_chains *hc)
{
    if (!hc) return HTM_OK;
    (void)hipSetDevice(hc->fwd->device);
    if (hc->side) (void)hipStreamSynchronize(hc->side);
    (void)hipStreamSynchronize(hc->fwd->stream);
    if (hc->ev_side) (void)hipEventDestroy(hc->ev_side);
    if (hc->side) (void)hipStreamDestroy(hc->side);
    if (hc->gexec) (void)hipGraphExecDestroy(hc->gexec);
    if (hc->graph) (void)hipGraphDestroy(hc->graph);
    for (void *p : hc->peer_maps) (void)hipIpcCloseMemHandle(p);
    if (hc->d_inbox) (void)hipFree(hc->d_inbox);
    for (void *p : hc->pool) (void)hipFree(p);
    if (hc->h_gath_pinned) (void)hipHostFree(hc->h_gath_pinned);
    if (hc->ev_wd) (void)hipEventDestroy(hc->ev_wd);
    if (hc->ev0) (void)hipEventDestroy(hc->ev0);
    if (hc->ev1) (void)hipEventDestroy(hc->ev1);
    delete hc;
    return HTM_OK;
}

static int flush_pending(htm_chains *hc)
{
    if (!hc->pending_gathered) return HTM_OK;
    const double *g = hc->pending_gathered;
    hc->pending_gathered = nullptr;
    return launch_step(hc, MODE_APPLY, hc->h_target, g);
}

// Wait for the chain kernels' stream, but never forever: every device-side wait is bounded (workers 30 s, master
// 5 s per hand-over), so a stream that has not drained after kWatchdogSeconds means the device is wedged -- report
// it instead of hanging the caller (HTM_WATCHDOG_S overrides the limit; 0 = wait without limit).
static int bounded_stream_sync(htm_chains *hc, const char *what)
{
    static const double limit = [] { const char *e = getenv("HTM_WATCHDOG_S"); return e ? atof(e) : 300.0; }();
    hipStream_t st = hc->fwd->stream;
    if (limit <= 0.0) { HIPCHK(hipStreamSynchronize(st)); return HTM_OK; }
    HIPCHK(hipEventRecord(hc->ev_wd, st));
    const auto t0 = std::chrono::steady_clock::now();
    for (long spin = 0;; ++spin) {
        const hipError_t e = hipEventQuery(hc->ev_wd);
        if (e == hipSuccess) return HTM_OK;
        if (e != hipErrorNotReady) return fail(HTM_EHIP, "%s: %s", what, hipGetErrorString(e));
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (dt > limit)
            return fail(HTM_ESTATE, "%s: the device made no progress for %.0f s (iteration %d + in-flight work, launch %llu)",
                        what, dt, hc->h_ctrl.iter_done, hc->launch_seq);
        if (spin > 2000) std::this_thread::sleep_for(std::chrono::microseconds(dt > 0.01 ? 200 : 5));
    }
}

static int read_ctrl(htm_chains *hc)
{
    // (nothing launched since the last read: the copy is current -- a driver that runs in short slices and asks for the state
    // in between would pay the copy and the stream synchronisation three times per slice)
    if (hc->ctrl_fresh && !hc->pending_gathered) return HTM_OK;
    int rc_ = flush_pending(hc);
    if (rc_) return rc_;
    HIPCHK(hipMemcpyAsync(&hc->h_ctrl, hc->dev.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, hc->fwd->stream));
    if ((rc_ = bounded_stream_sync(hc, "waiting for the chain kernels"))) return rc_;
    hc->spos_lo = hc->spos_hi = hc->h_ctrl.spos;
    hc->ctrl_fresh = true;
    return HTM_OK;
}

static int ctrl_error(const htm_chains *hc)
{
    switch (hc->h_ctrl.err) {
    case 0: return HTM_OK;
    case -4: return fail(HTM_ESTATE, "device RNG window exhausted (iteration %d)", hc->h_ctrl.iter_done + 1);
    case -5: return fail(HTM_EOVERFLOW, "record buffer overflow in lock-step mode: call htm_chains_drain more often");
    case -6: return fail(HTM_EDESYNC, "swap records of the ranks carry different iteration numbers");
    case -8: {
        // what the chain wave that gave up was waiting for (ChainsDev::diag), the chain's order slot and how many workers answered
        const ChainsDev &d = hc->dev;
        unsigned long long dg[32] = {0}, slot[kGranPerSlot] = {0};
        char extra[900] = "";
        if (hipMemcpy(dg, d.diag, sizeof(dg), hipMemcpyDeviceToHost) == hipSuccess && dg[0] == 1 && (int)dg[1] < d.n_chains) {
            const int c = (int)dg[1];
            int answered = 0;
            std::vector<unsigned long long> pg((size_t)d.n_workers * d.pgran_stride);
            if (hipMemcpy(slot, d.slots + (size_t)c * kGranPerSlot, sizeof(slot), hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(pg.data(), d.pgran + (size_t)c * d.n_workers * d.pgran_stride, pg.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
                for (int k = 0; k < d.n_workers; ++k)
                    if ((unsigned)(pg[(size_t)k * d.pgran_stride] >> 32) == (unsigned)dg[2]) ++answered;
                snprintf(extra, sizeof(extra),
                         "; chain %d waited for the sums of order %08llx (%s, step type %llu index %llu at stream position %llu, %s pass); "
                         "%d of %d workers answered; the chain's order slot holds tags %08llx %08llx %08llx %08llx %08llx %08llx %08llx %08llx, launch word %llu",
                         c, dg[2], dg[3] ? (dg[4] == 2 ? "sent two iterations ahead" : "sent one iteration ahead") : "sent by the chain's own wave",
                         dg[7], dg[8], dg[6], dg[11] ? "first" : "repeated", answered, d.n_workers,
                         slot[0] >> 32, slot[1] >> 32, slot[2] >> 32, slot[3] >> 32, slot[4] >> 32, slot[5] >> 32, slot[6] >> 32, slot[7] >> 32,
                         slot[0] & 0xffffffffull);
            }
            if (dg[24]) {
                const size_t n = strlen(extra);
                snprintf(extra + n, sizeof(extra) - n, "; worker 0 put %llu orders aside (named commit not visible within 20 us)", dg[24]);
            }
            if (dg[16] == 1) {
                const size_t n = strlen(extra);
                snprintf(extra + n, sizeof(extra) - n,
                         "; worker 0 has been waiting for more than a second for the commit named by order %08llx of chain %llu: element %llu "
                         "should read %016llx, reads %016llx (order word %llx, element left out %llu)",
                         dg[18], dg[17], dg[19], dg[20], dg[21], dg[22], dg[23]);
            }
        }
        return fail(HTM_ESTATE, "persistent workers did not answer within 5 s (iteration %d)%s", hc->h_ctrl.iter_done + 1, extra);
    }
    case -7: return fail(HTM_ESTATE, "random stream underrun in lock-step mode (iteration %d)", hc->h_ctrl.iter_done + 1);
    case -10: return fail(HTM_ESTATE, "swap records of another rank did not arrive within %.1f s (after iteration %d; HTM_XCHG_TIMEOUT_MS)",
                          (double)hc->dev.xwait_ticks * 1.0e-8, hc->h_ctrl.iter_done);
    case -11: return fail(HTM_ESTATE, "another rank reported a failure (iteration %d)", hc->h_ctrl.iter_done + 1);
    case -15: return fail(HTM_EDESYNC, "a swap record in the inbox was overwritten before it was read (after iteration %d): the ranks are more than the ring's depth apart", hc->h_ctrl.iter_done);
    case -12: return fail(HTM_ESTATE, "a chain wave of the master waited 5 s for another chain's step (its check, its commit before a swap, or the "
                          "rank's own header) after iteration %d: a wave has stopped making progress", hc->h_ctrl.iter_done);
    case -13: return fail(HTM_ESTATE, "the master's window of the random stream did not reach a step's position within 5 s (after iteration %d)",
                          hc->h_ctrl.iter_done);
    case -14: return fail(HTM_ESTATE, "an evaluator of the pipelined master waited 5 s for a proposal record (after iteration %d)", hc->h_ctrl.iter_done);
    case -16: {
        unsigned long long dg[8] = {0};
        (void)hipMemcpy(dg, hc->dev.diag, sizeof(dg), hipMemcpyDeviceToHost);
        return fail(HTM_ESTATE, "several master workgroups: chain %llu waited 5 s in its turn of iteration %llu for the chains %#llx (its epoch %llu, "
                    "the epoch in memory %llu, first awaited word %#llx)", dg[1], dg[2], dg[3], dg[4], dg[5], dg[6]);
    }
    case -17: case -18: case -19: case -20: case -21:
        return fail(HTM_ESTATE, "several master workgroups: a wait for %s gave up after 5 s (after iteration %d)",
                    hc->h_ctrl.err == -17 ? "the swap record of the iteration before" : hc->h_ctrl.err == -18 ? "the swap partner's record"
                    : hc->h_ctrl.err == -19 ? "the anchor the wave had just written" : "the last iteration's records at the end of the launch", hc->h_ctrl.iter_done);
    default: return fail(HTM_ESTATE, "device error flag %d", hc->h_ctrl.err);
    }
}

// move device record buffers to the host vectors; requires h_ctrl to be current and the stream idle
static int drain_records(htm_chains *hc)
{
    const ChainsDev &d = hc->dev;
    const int nl = hc->h_ctrl.n_lik, ns = hc->h_ctrl.n_smp;
    if (nl > 0) {
        const size_t o = hc->lik_iter.size();
        hc->lik_iter.resize(o + nl); hc->lik_chain.resize(o + nl); hc->lik_val.resize(o + nl);
        HIPCHK(hipMemcpy(hc->lik_iter.data() + o, d.lik_iter, nl * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hc->lik_chain.data() + o, d.lik_chain, nl * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hc->lik_val.data() + o, d.lik_val, nl * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (ns > 0) {
        const size_t o = hc->smp_iter.size();
        hc->smp_iter.resize(o + ns); hc->smp_chain.resize(o + ns); hc->smp_data.resize((o + ns) * hc->rec_len);
        HIPCHK(hipMemcpy(hc->smp_iter.data() + o, d.smp_iter, ns * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hc->smp_chain.data() + o, d.smp_chain, ns * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(hc->smp_data.data() + o * hc->rec_len, d.smp_data, (size_t)ns * hc->rec_len * sizeof(double),
                         hipMemcpyDeviceToHost));
    }
    if (hc->plan.flow || hc->plan.flow_lock) {
        // the free-running master hands out record slots as its waves get to them: put the drained records into the
        // reference's order, iteration by iteration and chain by chain (hypo_tremor_mcmc.f90:270-280)
        auto order = [](size_t n, const int32_t *it, const int32_t *ch) {
            std::vector<size_t> idx(n);
            for (size_t k = 0; k < n; ++k) idx[k] = k;
            std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return it[a] != it[b] ? it[a] < it[b] : ch[a] < ch[b]; });
            return idx;
        };
        if (nl > 1) {
            const size_t o = hc->lik_iter.size() - nl;
            const std::vector<size_t> idx = order(nl, hc->lik_iter.data() + o, hc->lik_chain.data() + o);
            std::vector<int32_t> it(nl), ch(nl); std::vector<double> v(nl);
            for (int k = 0; k < nl; ++k) { it[k] = hc->lik_iter[o + idx[k]]; ch[k] = hc->lik_chain[o + idx[k]]; v[k] = hc->lik_val[o + idx[k]]; }
            std::copy(it.begin(), it.end(), hc->lik_iter.begin() + o); std::copy(ch.begin(), ch.end(), hc->lik_chain.begin() + o);
            std::copy(v.begin(), v.end(), hc->lik_val.begin() + o);
        }
        if (ns > 1) {
            const size_t o = hc->smp_iter.size() - ns, rl = hc->rec_len;
            const std::vector<size_t> idx = order(ns, hc->smp_iter.data() + o, hc->smp_chain.data() + o);
            std::vector<int32_t> it(ns), ch(ns); std::vector<double> v((size_t)ns * rl);
            for (int k = 0; k < ns; ++k) {
                it[k] = hc->smp_iter[o + idx[k]]; ch[k] = hc->smp_chain[o + idx[k]];
                std::copy(hc->smp_data.begin() + (o + idx[k]) * rl, hc->smp_data.begin() + (o + idx[k] + 1) * rl, v.begin() + (size_t)k * rl);
            }
            std::copy(it.begin(), it.end(), hc->smp_iter.begin() + o); std::copy(ch.begin(), ch.end(), hc->smp_chain.begin() + o);
            std::copy(v.begin(), v.end(), hc->smp_data.begin() + o * rl);
        }
    }
    if (nl > 0 || ns > 0 || hc->h_ctrl.stop) {   // stop: 1 = record buffers full, 2 = stream underrun
        hc->h_ctrl.n_lik = 0; hc->h_ctrl.n_smp = 0; hc->h_ctrl.stop = 0;
        // stop, n_lik, n_smp are consecutive ints in Ctrl
        HIPCHK(hipMemcpy(&hc->dev.ctrl->stop, &hc->h_ctrl.stop, 3 * sizeof(int), hipMemcpyHostToDevice));
    }
    return HTM_OK;
}

static int build_graph(htm_chains *hc)
{
    if (hc->gexec) return HTM_OK;
    htm_forward *h = hc->fwd;
    hipStream_t cap = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    hipStream_t saved = h->stream;
    h->stream = cap;
    hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeRelaxed);
    int rc = HTM_OK;
    if (e != hipSuccess) rc = fail(HTM_EHIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
    const FullJob jb = chain_full_job(hc);
    for (int k = 0; k < hc->pairs && rc == HTM_OK; ++k) {
        rc = launch_step(hc, MODE_RUN, -1, nullptr);
        if (rc == HTM_OK) rc = launch_full(h, jb, hc->dev.n_chains);
    }
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(cap, &g);
    h->stream = saved;
    if (rc == HTM_OK && e != hipSuccess) rc = fail(HTM_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    if (rc == HTM_OK) {
        hc->graph = g;
        e = hipGraphInstantiate(&hc->gexec, g, nullptr, nullptr, 0);
        if (e != hipSuccess) rc = fail(HTM_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    }
    (void)hipStreamDestroy(cap);
    return rc;
}

// Single-rank main loop on the persistent kernel: one k_mcmc launch runs until the target, a full record
// buffer or the end of the produced random stream; no graph, no per-hand-over launches.
static int run_persistent(htm_chains *hc, int n_iter)
{
    htm_forward *h = hc->fwd;
    int rc;
    hc->h_target = hc->h_ctrl.iter_done + n_iter;
    hc->run_full0 = hc->h_ctrl.n_full_evals; hc->run_part0 = hc->h_ctrl.n_partial_evals;
    hc->last_graph_launches = 0;
    HIPCHK(hipEventRecord(hc->ev0, h->stream));
    while (hc->h_ctrl.iter_done < hc->h_target) {
        // a launch may run as far as the produced stream reaches
        const long long fed = (hc->n_hop - hc->h_ctrl.spos) / (6 * hc->dev.n_chains + 4) - 2;
        const int target = (int)std::min<long long>(hc->h_target, hc->h_ctrl.iter_done + std::max<long long>(1, fed));
        if ((rc = launch_mcmc(hc, MODE_RUN, target, nullptr))) return rc;
        hc->last_graph_launches += 1;
        // keep the random stream about half a ring ahead (asynchronous, side stream), while the launch runs
        {
            const long long ahead = hc->n_hop - hc->h_ctrl.spos;
            if (ahead < hc->cap / 2 && (rc = stream_produce(hc, std::min<long long>(hc->cap / 2 - ahead + 4096, 1 << 18)))) return rc;
        }
        if ((rc = read_ctrl(hc))) return rc;
        if ((rc = ctrl_error(hc))) return rc;
        if (hc->h_ctrl.stop == 2) HIPCHK(hipStreamSynchronize(hc->side));
        if (hc->h_ctrl.stop) { if ((rc = drain_records(hc))) return rc; }
    }
    HIPCHK(hipEventRecord(hc->ev1, h->stream));
    HIPCHK(hipEventSynchronize(hc->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, hc->ev0, hc->ev1));
    hc->last_device_us = 1000.0 * ms;
    hc->last_full = hc->h_ctrl.n_full_evals - hc->run_full0;
    hc->last_part = hc->h_ctrl.n_partial_evals - hc->run_part0;
    return drain_records(hc);
}

int htm_chains_run(htm_chains *hc, int n_iter)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    if (n_iter < 0) return fail(HTM_EINVAL, "n_iter must be >= 0");
    if (hc->dev.n_procs != 1)
        return fail(HTM_ESTATE, "htm_chains_run is the single-rank driver; use step_begin/step_end for n_procs > 1");
    htm_forward *h = hc->fwd;
    HIPCHK(hipSetDevice(h->device));
    int rc = read_ctrl(hc);
    if (rc) return rc;
    if (hc->h_ctrl.stage == ST_WAIT_SWAP) return fail(HTM_ESTATE, "a lock-step iteration is in flight");
    if (hc->plan.persist && hc->h_ctrl.stage == ST_IDLE) return run_persistent(hc, n_iter);
    if ((rc = build_graph(hc))) return rc;
    hc->h_target = hc->h_ctrl.iter_done + n_iter;
    HIPCHK(hipMemcpyAsync(&hc->dev.ctrl->iter_target, &hc->h_target, sizeof(int), hipMemcpyHostToDevice, h->stream));
    hc->run_full0 = hc->h_ctrl.n_full_evals; hc->run_part0 = hc->h_ctrl.n_partial_evals;
    hc->last_graph_launches = 0;
    HIPCHK(hipEventRecord(hc->ev0, h->stream));
    double it_per_launch = 1.5 * hc->pairs;     // refined from what the device actually achieved
    while (true) {
        const int remaining = hc->h_target - hc->h_ctrl.iter_done;
        if (remaining <= 0 && hc->h_ctrl.stage == ST_IDLE) break;
        int g = (int)(0.8 * remaining / it_per_launch);
        // no more launches than the produced random stream can feed (an iteration draws < 6*n_chains + 4)
        const long long fed = (hc->n_hop - hc->h_ctrl.spos) / (6 * hc->dev.n_chains + 4);
        g = std::min<long long>(g, (long long)(0.9 * fed / it_per_launch));
        g = std::max(1, std::min(g, 512));
        const int before = hc->h_ctrl.iter_done;
        hc->ctrl_fresh = false;
        for (int k = 0; k < g; ++k) HIPCHK(hipGraphLaunch(hc->gexec, h->stream));
        hc->last_graph_launches += g;
        if ((rc = read_ctrl(hc))) return rc;
        if ((rc = ctrl_error(hc))) return rc;
        if (hc->h_ctrl.iter_done > before && !hc->h_ctrl.stop)
            it_per_launch = std::max(1.0, double(hc->h_ctrl.iter_done - before) / g);
        // keep the random stream about two batches ahead (asynchronous, on the side stream)
        {
            const long long want = hc->cap / 2;
            const long long ahead = hc->n_hop - hc->h_ctrl.spos;
            if (ahead < want && (rc = stream_produce(hc, std::min<long long>(want - ahead + 4096, 1 << 18)))) return rc;
        }
        if (hc->h_ctrl.stop == 2) HIPCHK(hipStreamSynchronize(hc->side));   // underrun: wait for the producer
        if (hc->h_ctrl.stop) { if ((rc = drain_records(hc))) return rc; }
    }
    HIPCHK(hipEventRecord(hc->ev1, h->stream));
    HIPCHK(hipEventSynchronize(hc->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, hc->ev0, hc->ev1));
    hc->last_device_us = 1000.0 * ms;
    hc->last_full = hc->h_ctrl.n_full_evals - hc->run_full0;
    hc->last_part = hc->h_ctrl.n_partial_evals - hc->run_part0;
    return drain_records(hc);
}

int htm_chains_profile(htm_chains *hc, int n_iter, double *step_us, int *step_launches, double *full_us,
                       int *full_launches, int64_t *full_evals, int64_t *partial_evals)
{
    if (!hc || n_iter < 0) return fail(HTM_EINVAL, "bad argument");
    if (hc->dev.n_procs != 1) return fail(HTM_ESTATE, "htm_chains_profile is single-rank");
    htm_forward *h = hc->fwd;
    HIPCHK(hipSetDevice(h->device));
    int rc = read_ctrl(hc);
    if (rc) return rc;
    hc->h_target = hc->h_ctrl.iter_done + n_iter;
    HIPCHK(hipMemcpyAsync(&hc->dev.ctrl->iter_target, &hc->h_target, sizeof(int), hipMemcpyHostToDevice, h->stream));
    const long long f0 = hc->h_ctrl.n_full_evals, p0 = hc->h_ctrl.n_partial_evals;
    constexpr int B = 64;                       // launch pairs between host checks
    struct Events {             // destroyed on every return path
        std::vector<hipEvent_t> v;
        ~Events() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); }
    } evs;
    evs.v.assign(3 * B, nullptr);
    std::vector<hipEvent_t> &ev = evs.v;
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    const FullJob jb = chain_full_job(hc);
    double s_us = 0.0, f_us = 0.0;
    int s_n = 0, f_n = 0;
    while (true) {
        if (hc->h_target - hc->h_ctrl.iter_done <= 0 && hc->h_ctrl.stage == ST_IDLE) break;
        for (int k = 0; k < B; ++k) {
            HIPCHK(hipEventRecord(ev[3 * k], h->stream));
            if ((rc = launch_step(hc, MODE_RUN, -1, nullptr))) return rc;
            HIPCHK(hipEventRecord(ev[3 * k + 1], h->stream));
            if ((rc = launch_full(h, jb, hc->dev.n_chains))) return rc;
            HIPCHK(hipEventRecord(ev[3 * k + 2], h->stream));
        }
        if ((rc = read_ctrl(hc))) return rc;
        if ((rc = ctrl_error(hc))) return rc;
        if (hc->n_hop - hc->h_ctrl.spos < 16384 && (rc = stream_produce(hc, 16384))) return rc;
        if (hc->h_ctrl.stop == 2) HIPCHK(hipStreamSynchronize(hc->side));
        for (int k = 0; k < B; ++k) {
            float a = 0.f, b = 0.f;
            HIPCHK(hipEventElapsedTime(&a, ev[3 * k], ev[3 * k + 1]));
            HIPCHK(hipEventElapsedTime(&b, ev[3 * k + 1], ev[3 * k + 2]));
            s_us += 1000.0 * a; f_us += 1000.0 * b; s_n++; f_n++;
        }
        if (hc->h_ctrl.stop && (rc = drain_records(hc))) return rc;
    }
    if (step_us) *step_us = s_us;
    if (step_launches) *step_launches = s_n;
    if (full_us) *full_us = f_us;
    if (full_launches) *full_launches = f_n;
    if (full_evals) *full_evals = hc->h_ctrl.n_full_evals - f0;
    if (partial_evals) *partial_evals = hc->h_ctrl.n_partial_evals - p0;
    return drain_records(hc);
}

int htm_chains_step_begin(htm_chains *hc)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    htm_forward *h = hc->fwd;
    HIPCHK(hipSetDevice(h->device));
    hc->h_target += 1;
    int rc;
    // an iteration consumes at most wmax draws; keep the produced stream safely ahead of that bound
    hc->spos_hi += hc->plan.wmax;
    if (hc->n_hop - hc->spos_hi < 4 * (long long)hc->plan.wmax) {
        if ((rc = read_ctrl(hc))) return rc;              // exact position (also frees ring capacity)
        if ((rc = ctrl_error(hc))) return rc;
        hc->spos_hi += hc->plan.wmax;
        if ((rc = stream_produce(hc, 1 << 16))) return rc;
        HIPCHK(hipStreamWaitEvent(h->stream, hc->ev_side, 0));
    }
    if (hc->plan.persist) {       // whole iteration (full evaluations included) in one launch
        rc = launch_mcmc(hc, MODE_ADVANCE, hc->h_target, hc->pending_gathered);
        hc->pending_gathered = nullptr;
        return rc;
    }
    rc = launch_step(hc, MODE_ADVANCE, hc->h_target, hc->pending_gathered);   // applies the previous swap first
    hc->pending_gathered = nullptr;
    if (rc) return rc;
    if ((rc = launch_full(h, chain_full_job(hc), hc->dev.n_chains))) return rc;
    return launch_step(hc, MODE_FINISH, hc->h_target, nullptr);
}

int htm_chains_run_lockstep(htm_chains *hc, int n_iter, htm_allgather_fn allgather, void *comm, void *d_gathered)
{
    if (!hc || !allgather || !d_gathered || n_iter < 0) return fail(HTM_EINVAL, "bad argument");
    htm_forward *h = hc->fwd;
    HIPCHK(hipSetDevice(h->device));
    const size_t words = 4 + 2 * (size_t)hc->dev.n_chains;
    // records a rank may hold on the device between drains: n_chains per iteration at most
    const int drain_every = std::max(1, std::min(hc->dev.cap_lik, hc->dev.cap_smp) / (2 * hc->dev.n_chains) - 2);
    int k = 0, since_drain = 0, rc;
    // stats of this call (htm_chains_last_run_stats): evaluations counted on the device, HIP events on the kernels' stream
    if ((rc = read_ctrl(hc))) return rc;
    hc->run_full0 = hc->h_ctrl.n_full_evals; hc->run_part0 = hc->h_ctrl.n_partial_evals;
    hc->last_graph_launches = 0;
    HIPCHK(hipEventRecord(hc->ev0, h->stream));
    for (; k < n_iter; ++k) {
        rc = htm_chains_step_begin(hc);
        if (rc) return rc;
        const int st = allgather(hc->dev.swap_rec, d_gathered, words, 8 /* ncclFloat64 */, comm, h->stream);
        if (st != 0) return fail(HTM_EHIP, "all-gather of the swap records failed with status %d", st);
        if ((rc = htm_chains_step_end(hc, d_gathered))) return rc;
        if (++since_drain >= drain_every) { if ((rc = htm_chains_drain(hc))) return rc; since_drain = 0; }
        else if ((k & 511) == 511 && (rc = bounded_stream_sync(hc, "lock-step loop"))) return rc;
    }
    hc->last_graph_launches = n_iter;
    HIPCHK(hipEventRecord(hc->ev1, h->stream));
    if ((rc = read_ctrl(hc))) return rc;          // flushes the last swap, waits for the stream
    if ((rc = ctrl_error(hc))) return rc;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, hc->ev0, hc->ev1));
    hc->last_device_us = 1000.0 * ms;
    hc->last_full = hc->h_ctrl.n_full_evals - hc->run_full0;
    hc->last_part = hc->h_ctrl.n_partial_evals - hc->run_part0;
    return HTM_OK;
}

// ---- persistent lock-step: swap records exchanged inside the launch (exchange_post / exchange_finish in htm_handoff.hpp) --------
static int xchg_alloc(htm_chains *hc)
{
    if (hc->d_inbox) return HTM_OK;
    ChainsDev &d = hc->dev;
    d.xg = 2 * (4 + 2 * d.n_chains) + 2;
    // (region A [2][n_procs][xg]: the barrier loop's records; region B [kXSlots][n_procs][xg]: the free-running lock-step loop's, htm_flow.hpp)
    hc->inbox_bytes = (size_t)(2 + kXSlots) * d.n_procs * d.xg * sizeof(unsigned long long);
    void *p = nullptr;
    // fine-grained: peers write it over xGMI while this rank's kernel polls it (system-scope accesses, no L2 copy)
    hipError_t e = hipExtMallocWithFlags(&p, hc->inbox_bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        e = hipExtMallocWithFlags(&p, hc->inbox_bytes, hipDeviceMallocUncached);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); HIPCHK(hipMalloc(&p, hc->inbox_bytes)); }
    HIPCHK(hipMemset(p, 0, hc->inbox_bytes));
    hc->d_inbox = static_cast<unsigned long long *>(p);
    d.inbox = hc->d_inbox;
    return HTM_OK;
}

int htm_chains_xchg_handle(htm_chains *hc, void *handle, size_t handle_bytes)
{
    if (!hc || !handle) return fail(HTM_EINVAL, "NULL argument");
    if (handle_bytes < sizeof(hipIpcMemHandle_t)) return fail(HTM_EINVAL, "handle buffer too small (%zu < %zu)", handle_bytes, sizeof(hipIpcMemHandle_t));
    HIPCHK(hipSetDevice(hc->fwd->device));
    int rc = xchg_alloc(hc);
    if (rc) return rc;
    hipIpcMemHandle_t h;
    HIPCHK(hipIpcGetMemHandle(&h, hc->d_inbox));
    std::memset(handle, 0, handle_bytes);
    std::memcpy(handle, &h, sizeof(h));
    return HTM_OK;
}

int htm_chains_xchg_connect(htm_chains *hc, const void *handles, size_t handle_bytes)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    const ChainsDev &d0 = hc->dev;
    if (d0.n_procs > 1 && (!handles || handle_bytes < sizeof(hipIpcMemHandle_t)))
        return fail(HTM_EINVAL, "handles of all %d ranks are needed", d0.n_procs);
    if (!hc->plan.persist) return fail(HTM_ESTATE, "the in-kernel exchange needs the persistent kernel (HTM_PERSIST=0 is set)");
    if ((size_t)d0.n_procs * (4 + 2 * d0.n_chains) > (size_t)kGathStage)
        return fail(HTM_EINVAL, "%d ranks x %d chains: the gathered records do not fit the kernel's staging area", d0.n_procs, d0.n_chains);
    HIPCHK(hipSetDevice(hc->fwd->device));
    int rc = xchg_alloc(hc);
    if (rc) return rc;
    if (hc->xchg_ready) return HTM_OK;
    std::vector<unsigned long long *> ptr(d0.n_procs, nullptr);
    for (int q = 0; q < d0.n_procs; ++q) {
        if (q == d0.rank) { ptr[q] = hc->d_inbox; continue; }
        hipIpcMemHandle_t h;
        std::memcpy(&h, static_cast<const char *>(handles) + (size_t)q * handle_bytes, sizeof(h));
        void *p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            for (void *m : hc->peer_maps) (void)hipIpcCloseMemHandle(m);
            hc->peer_maps.clear();
            return fail(HTM_EHIP, "hipIpcOpenMemHandle of rank %d's inbox failed: %s", q, hipGetErrorString(e));
        }
        hc->peer_maps.push_back(p);
        ptr[q] = static_cast<unsigned long long *>(p);
    }
    if ((rc = dev_upload(hc->pool, &hc->d_outbox, ptr.data(), ptr.size()))) return rc;
    hc->dev.outbox = hc->d_outbox;
    hc->xchg_ready = true;
    return HTM_OK;
}

int htm_chains_xchg_probe(htm_chains *hc, unsigned token, double seconds)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    if (!hc->xchg_ready) return fail(HTM_ESTATE, "htm_chains_xchg_connect has not been called");
    HIPCHK(hipSetDevice(hc->fwd->device));
    int *d_res = nullptr;
    int rc = dev_alloc(hc->pool, &d_res, 1);
    if (rc) return rc;
    HIPCHK(hipMemset(d_res, 0, sizeof(int)));
    const unsigned long long ticks = (unsigned long long)(std::max(0.01, std::min(seconds, 60.0)) * 1e8);
    // (the probe is collective: every rank has made the same number of calls, so the count makes a repeated probe's tokens
    // new ones whatever token the callers pass -- a second probe must not pass on what the first one left in the inboxes)
    const unsigned eff = (token + 0x10000u * ++hc->probe_calls) & 0x7fffffffu;
    hipLaunchKernelGGL(k_xchg_probe, dim3(1), dim3(64), 0, hc->fwd->stream, hc->dev, eff, ticks, d_res);
    HIPCHK(hipGetLastError());
    int res = 0;
    HIPCHK(hipMemcpyAsync(&res, d_res, sizeof(int), hipMemcpyDeviceToHost, hc->fwd->stream));
    if ((rc = bounded_stream_sync(hc, "inbox probe"))) return rc;
    if (!res) return fail(HTM_ESTATE, "inbox probe: the tokens of the other ranks did not arrive within %.1f s", seconds);
    return HTM_OK;
}

// n_iter lock-step iterations with the exchange inside the kernel: one k_mcmc launch runs until the target, or until
// some rank asks everybody to stop (its record buffers or its produced random stream are nearly used up); then every
// rank drains / refills and launches again.  All ranks leave a launch after the same iteration.
int htm_chains_run_lockstep_direct(htm_chains *hc, int n_iter)
{
    if (!hc || n_iter < 0) return fail(HTM_EINVAL, "bad argument");
    if (!hc->xchg_ready) return fail(HTM_ESTATE, "htm_chains_xchg_connect has not been called");
    htm_forward *h = hc->fwd;
    HIPCHK(hipSetDevice(h->device));
    int rc = read_ctrl(hc);
    if (rc) return rc;
    if ((rc = ctrl_error(hc))) return rc;
    if (hc->h_ctrl.stage != ST_IDLE) return fail(HTM_ESTATE, "an iteration is in flight");
    hc->h_target = hc->h_ctrl.iter_done + n_iter;
    hc->run_full0 = hc->h_ctrl.n_full_evals; hc->run_part0 = hc->h_ctrl.n_partial_evals;
    hc->last_graph_launches = 0;
    HIPCHK(hipEventRecord(hc->ev0, h->stream));
    while (hc->h_ctrl.iter_done < hc->h_target) {
        // the launch reads the produced stream's extent once, at its start: have a good stretch ready
        long long ahead = hc->n_hop - hc->h_ctrl.spos;
        if (ahead < hc->cap / 2 && (rc = stream_produce(hc, std::min<long long>(hc->cap / 2 - ahead + 4096, 1 << 18)))) return rc;
        HIPCHK(hipStreamWaitEvent(h->stream, hc->ev_side, 0));      // (the producer takes ~0.1 ms per 2^18 positions)
        const int before = hc->h_ctrl.iter_done;
        if ((rc = launch_mcmc(hc, MODE_LOCKRUN, hc->h_target, nullptr))) return rc;
        hc->last_graph_launches += 1;
        ahead = hc->n_hop - hc->h_ctrl.spos;        // top up while the launch runs (for the next one)
        if (ahead < hc->cap / 2 && (rc = stream_produce(hc, std::min<long long>(hc->cap / 2 - ahead + 4096, 1 << 18)))) return rc;
        if ((rc = read_ctrl(hc))) return rc;
        if ((rc = ctrl_error(hc))) return rc;
        if (hc->h_ctrl.stop) { if ((rc = drain_records(hc))) return rc; }
        else if (hc->h_ctrl.iter_done == before && hc->h_ctrl.iter_done < hc->h_target)
            return fail(HTM_ESTATE, "lock-step launch made no progress at iteration %d", before);
    }
    HIPCHK(hipEventRecord(hc->ev1, h->stream));
    HIPCHK(hipEventSynchronize(hc->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, hc->ev0, hc->ev1));
    hc->last_device_us = 1000.0 * ms;
    hc->last_full = hc->h_ctrl.n_full_evals - hc->run_full0;
    hc->last_part = hc->h_ctrl.n_partial_evals - hc->run_part0;
    return drain_records(hc);
}

// ---- RCCL reached from the C ABI (so that a Fortran / C host needs no Python to use RCCL for the swap) ----------
// librccl is bound at run time (dlopen): the library itself does not link against it, and inside a PyTorch process the
// copy torch has already loaded is reused.  Only the four entry points the swap needs.
struct htm_comm {
    void *lib = nullptr, *comm = nullptr;
    int rank = 0, n_ranks = 1, device = 0;
    int (*all_gather)(const void *, void *, size_t, int, void *, void *) = nullptr;
    int (*comm_destroy)(void *) = nullptr;
    double *d_gathered = nullptr;
    size_t gathered_cap = 0;
};
namespace {
struct NcclId { char b[HTM_COMM_ID_BYTES]; };
void *rccl_open()
{
    static void *lib = [] {
        const char *names[] = {getenv("HTM_RCCL_LIB"), "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        void *h = nullptr;
        for (const char *n : names) {
            if (!n || !*n) continue;
            if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD))) break;      // already in the process (PyTorch's copy)
        }
        for (const char *n : names) {
            if (h) break;
            if (!n || !*n) continue;
            h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        }
        return h;
    }();
    return lib;
}
}  // namespace

int htm_comm_unique_id(void *id, size_t id_bytes)
{
    if (!id || id_bytes < HTM_COMM_ID_BYTES) return fail(HTM_EINVAL, "id buffer must hold %d bytes", HTM_COMM_ID_BYTES);
    void *lib = rccl_open();
    if (!lib) return fail(HTM_ENODEVICE, "librccl.so not found (%s)", dlerror());
    auto get_id = reinterpret_cast<int (*)(NcclId *)>(dlsym(lib, "ncclGetUniqueId"));
    if (!get_id) return fail(HTM_ENODEVICE, "ncclGetUniqueId not found in librccl");
    NcclId u;
    std::memset(&u, 0, sizeof(u));
    const int st = get_id(&u);
    if (st != 0) return fail(HTM_EHIP, "ncclGetUniqueId failed with status %d", st);
    std::memset(id, 0, id_bytes);
    std::memcpy(id, &u, sizeof(u));
    return HTM_OK;
}

int htm_comm_create(const void *id, size_t id_bytes, int rank, int n_ranks, int device, htm_comm **out)
{
    if (!out) return fail(HTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (!id || id_bytes < HTM_COMM_ID_BYTES || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(HTM_EINVAL, "bad argument");
    int rc = use_device(device);
    if (rc) return rc;
    void *lib = rccl_open();
    if (!lib) return fail(HTM_ENODEVICE, "librccl.so not found (%s)", dlerror());
    auto init_rank = reinterpret_cast<int (*)(void **, int, NcclId, int)>(dlsym(lib, "ncclCommInitRank"));
    auto all_gather = reinterpret_cast<int (*)(const void *, void *, size_t, int, void *, void *)>(dlsym(lib, "ncclAllGather"));
    auto destroy = reinterpret_cast<int (*)(void *)>(dlsym(lib, "ncclCommDestroy"));
    if (!init_rank || !all_gather || !destroy) return fail(HTM_ENODEVICE, "librccl lacks ncclCommInitRank / ncclAllGather / ncclCommDestroy");
    NcclId u;
    std::memcpy(&u, id, sizeof(u));
    void *comm = nullptr;
    const int st = init_rank(&comm, n_ranks, u, rank);
    if (st != 0 || !comm) return fail(HTM_EHIP, "ncclCommInitRank failed with status %d (RCCL refuses two ranks on one device)", st);
    htm_comm *c = new htm_comm();
    c->lib = lib; c->comm = comm; c->rank = rank; c->n_ranks = n_ranks; c->device = device;
    c->all_gather = all_gather; c->comm_destroy = destroy;
    *out = c;
    return HTM_OK;
}

int htm_comm_destroy(htm_comm *c)
{
    if (!c) return HTM_OK;
    (void)hipSetDevice(c->device);
    if (c->d_gathered) (void)hipFree(c->d_gathered);
    if (c->comm && c->comm_destroy) (void)c->comm_destroy(c->comm);
    delete c;
    return HTM_OK;
}

int htm_comm_allgather(htm_comm *c, const void *d_send, void *d_recv, size_t bytes_per_rank, void *hip_stream)
{
    if (!c || !d_send || !d_recv) return fail(HTM_EINVAL, "NULL argument");
    const int st = c->all_gather(d_send, d_recv, bytes_per_rank, 0 /* ncclInt8 */, c->comm, hip_stream);
    if (st != 0) return fail(HTM_EHIP, "ncclAllGather failed with status %d", st);
    return HTM_OK;
}

int htm_chains_run_lockstep_comm(htm_chains *hc, int n_iter, htm_comm *c)
{
    if (!hc || !c) return fail(HTM_EINVAL, "NULL argument");
    if (c->n_ranks != hc->dev.n_procs || c->rank != hc->dev.rank) return fail(HTM_EINVAL, "communicator rank/size do not match the chain set");
    HIPCHK(hipSetDevice(hc->fwd->device));
    const size_t words = (4 + 2 * (size_t)hc->dev.n_chains) * (size_t)c->n_ranks;
    if (words > c->gathered_cap) {
        if (c->d_gathered) HIPCHK(hipFree(c->d_gathered));
        c->d_gathered = nullptr;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&c->d_gathered), words * sizeof(double)));
        c->gathered_cap = words;
    }
    return htm_chains_run_lockstep(hc, n_iter, c->all_gather, c->comm, c->d_gathered);
}

int htm_chains_swap_record(htm_chains *hc, void **d_record, size_t *record_bytes)
{
    if (!hc || !d_record || !record_bytes) return fail(HTM_EINVAL, "NULL argument");
    *d_record = hc->dev.swap_rec;
    *record_bytes = (4 + 2 * (size_t)hc->dev.n_chains) * sizeof(double);
    return HTM_OK;
}

int htm_chains_step_end(htm_chains *hc, const void *d_gathered_records)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    if (!d_gathered_records) return fail(HTM_EINVAL, "gathered records pointer is NULL");
    HIPCHK(hipSetDevice(hc->fwd->device));
    // deferred: the next step_begin's kernel applies the swap before it advances (one launch less per
    // iteration); anything that looks at the state flushes it first (flush_pending)
    hc->pending_gathered = static_cast<const double *>(d_gathered_records);
    return HTM_OK;
}

int htm_chains_swap_record_host(htm_chains *hc, double *record)
{
    if (!hc || !record) return fail(HTM_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(hc->fwd->device));
    const size_t words = 4 + 2 * (size_t)hc->dev.n_chains;
    HIPCHK(hipMemcpyAsync(record, hc->dev.swap_rec, words * sizeof(double), hipMemcpyDeviceToHost, hc->fwd->stream));
    return bounded_stream_sync(hc, "waiting for the iteration's swap record");
}

int htm_chains_step_end_host(htm_chains *hc, const double *gathered_records)
{
    if (!hc || !gathered_records) return fail(HTM_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(hc->fwd->device));
    const size_t words = (4 + 2 * (size_t)hc->dev.n_chains) * (size_t)hc->dev.n_procs;
    if (!hc->d_gath_host) {
        int rc = dev_alloc(hc->pool, &hc->d_gath_host, words);
        if (rc) return rc;
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&hc->h_gath_pinned), words * sizeof(double), hipHostMallocDefault));
    }
    // the caller may reuse its array at once: stage through pinned memory (the previous copy has completed --
    // swap_record_host of this iteration waited for the stream)
    std::memcpy(hc->h_gath_pinned, gathered_records, words * sizeof(double));
    HIPCHK(hipMemcpyAsync(hc->d_gath_host, hc->h_gath_pinned, words * sizeof(double), hipMemcpyHostToDevice, hc->fwd->stream));
    return htm_chains_step_end(hc, hc->d_gath_host);
}

int htm_chains_sync(htm_chains *hc)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(hc->fwd->device));
    int rc = read_ctrl(hc);
    if (rc) return rc;
    return ctrl_error(hc);
}

int htm_chains_drain(htm_chains *hc)
{
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    return drain_records(hc);
}

int htm_chains_iterations_done(htm_chains *hc, int *n)
{
    if (!hc || !n) return fail(HTM_EINVAL, "NULL argument");
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    *n = hc->h_ctrl.iter_done;
    return HTM_OK;
}

// ---- checkpoint / resume ------------------------------------------------------------------------------
namespace {
struct CkptHeader {
    uint32_t magic, version;
    int32_t n_chains, n_sta, n_events, n_procs, rank, iter_done;
    uint32_t rng_state[4];
    int64_t n_full_evals, n_partial_evals;
    uint64_t jobs_total;
    uint64_t total;           // doubles in the parameter vector
};
constexpr uint32_t kCkptMagic = 0x48544d43u;   // "HTMC"
size_t ckpt_total(const htm_chains *hc)
{
    const size_t n = hc->dev.n_chains, S = hc->dev.S, E = hc->dev.E;
    return 2 * n + 2 * n * S + 3 * E * n;
}
size_t ckpt_bytes(const htm_chains *hc)
{
    const size_t n = hc->dev.n_chains;
    return sizeof(CkptHeader) + (ckpt_total(hc) + 2 * n) * sizeof(double) + (2 * 7 + 1) * n * sizeof(int32_t);      // (+ prev_mid)
}
}  // namespace

int htm_chains_checkpoint_size(htm_chains *hc, size_t *bytes)
{
    if (!hc || !bytes) return fail(HTM_EINVAL, "NULL argument");
    *bytes = ckpt_bytes(hc);
    return HTM_OK;
}

int htm_chains_checkpoint_save(htm_chains *hc, void *blob, size_t bytes)
{
    if (!hc || !blob) return fail(HTM_EINVAL, "NULL argument");
    if (bytes < ckpt_bytes(hc)) return fail(HTM_EINVAL, "checkpoint buffer too small (%zu < %zu)", bytes, ckpt_bytes(hc));
    int rc = htm_chains_sync(hc);            // flushes a pending swap, raises device error flags
    if (rc) return rc;
    if (hc->h_ctrl.stage != ST_IDLE) return fail(HTM_ESTATE, "a lock-step iteration is in flight");
    CkptHeader h{};
    h.magic = kCkptMagic; h.version = 2;
    h.n_chains = hc->dev.n_chains; h.n_sta = hc->dev.S; h.n_events = hc->dev.E; h.n_procs = hc->dev.n_procs; h.rank = hc->dev.rank;
    h.iter_done = hc->h_ctrl.iter_done;
    if ((rc = htm_chains_get_rng(hc, h.rng_state))) return rc;
    h.n_full_evals = hc->h_ctrl.n_full_evals; h.n_partial_evals = hc->h_ctrl.n_partial_evals;
    h.jobs_total = hc->h_ctrl.jobs_total;
    h.total = ckpt_total(hc);
    char *p = static_cast<char *>(blob);
    std::memcpy(p, &h, sizeof(h)); p += sizeof(h);
    const size_t n = hc->dev.n_chains;
    HIPCHK(hipMemcpy(p, hc->dev.xall, h.total * sizeof(double), hipMemcpyDeviceToHost)); p += h.total * sizeof(double);
    HIPCHK(hipMemcpy(p, hc->dev.temp, n * sizeof(double), hipMemcpyDeviceToHost)); p += n * sizeof(double);
    HIPCHK(hipMemcpy(p, hc->dev.L, n * sizeof(double), hipMemcpyDeviceToHost)); p += n * sizeof(double);
    HIPCHK(hipMemcpy(p, hc->dev.n_propose, 7 * n * sizeof(int32_t), hipMemcpyDeviceToHost)); p += 7 * n * sizeof(int32_t);
    HIPCHK(hipMemcpy(p, hc->dev.n_accept, 7 * n * sizeof(int32_t), hipMemcpyDeviceToHost)); p += 7 * n * sizeof(int32_t);
    // (what each chain's last step was: decides which event its next full evaluation leaves to the chain's own wave, so that
    // a continued run sums in the order of the uninterrupted one)
    HIPCHK(hipMemcpy(p, hc->dev.prev_mid, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HTM_OK;
}

int htm_chains_checkpoint_load(htm_chains *hc, const void *blob, size_t bytes)
{
    if (!hc || !blob) return fail(HTM_EINVAL, "NULL argument");
    if (bytes < sizeof(CkptHeader)) return fail(HTM_EINVAL, "checkpoint blob truncated");
    CkptHeader h{};
    std::memcpy(&h, blob, sizeof(h));
    if (h.magic != kCkptMagic || h.version != 2) return fail(HTM_EINVAL, "not a checkpoint of this library (magic/version)");
    if (h.n_chains != hc->dev.n_chains || h.n_sta != hc->dev.S || h.n_events != hc->dev.E || h.n_procs != hc->dev.n_procs ||
        h.rank != hc->dev.rank || h.total != ckpt_total(hc))
        return fail(HTM_EINVAL, "checkpoint shape (%d chains, %d x %d, rank %d/%d) does not match this chain set", h.n_chains,
                    h.n_events, h.n_sta, h.rank, h.n_procs);
    if (bytes < ckpt_bytes(hc)) return fail(HTM_EINVAL, "checkpoint blob truncated");
    // A load REPLACES the control block -- iteration counter, stage, error word -- so it must work on a chain set whose last
    // run failed (the roll-back of a failed lock-step run, parallel.py): wait for the stream, do not report what is about to
    // be overwritten.  (An iteration of the per-launch lock-step in flight -- records out, swap not applied -- is dropped too.)
    HIPCHK(hipSetDevice(hc->fwd->device));
    hc->pending_gathered = nullptr;
    int rc = bounded_stream_sync(hc, "waiting for the chain kernels before a checkpoint load");
    if (rc) return rc;
    hc->ctrl_fresh = false;
    HIPCHK(hipStreamSynchronize(hc->side));
    const char *p = static_cast<const char *>(blob) + sizeof(h);
    const size_t n = hc->dev.n_chains;
    HIPCHK(hipMemcpy(hc->dev.xall, p, h.total * sizeof(double), hipMemcpyHostToDevice)); p += h.total * sizeof(double);
    HIPCHK(hipMemcpy(hc->dev.temp, p, n * sizeof(double), hipMemcpyHostToDevice)); p += n * sizeof(double);
    HIPCHK(hipMemcpy(hc->dev.L, p, n * sizeof(double), hipMemcpyHostToDevice)); p += n * sizeof(double);
    HIPCHK(hipMemcpy(hc->dev.n_propose, p, 7 * n * sizeof(int32_t), hipMemcpyHostToDevice)); p += 7 * n * sizeof(int32_t);
    HIPCHK(hipMemcpy(hc->dev.n_accept, p, 7 * n * sizeof(int32_t), hipMemcpyHostToDevice)); p += 7 * n * sizeof(int32_t);
    HIPCHK(hipMemcpy(hc->dev.prev_mid, p, n * sizeof(int32_t), hipMemcpyHostToDevice));
    // the random stream restarts at the saved generator state: position 0 of a fresh stream
    for (int k = 0; k < 4; ++k) hc->init_state[k] = h.rng_state[k];
    HIPCHK(hipMemcpy(hc->dev.stream.gen, hc->init_state, 4 * sizeof(uint32_t), hipMemcpyHostToDevice));
    hc->gen_par = 0;
    const long long zero = 0;
    HIPCHK(hipMemcpy(hc->dev.stream.hop_end, &zero, sizeof(zero), hipMemcpyHostToDevice));
    hc->n_raw = hc->n_tr = hc->n_rec = hc->n_hop = 0;
    hc->spos_lo = hc->spos_hi = 0;
    Ctrl c{};
    c.stage = ST_IDLE; c.spos = 0; c.iter_done = h.iter_done; c.iter_target = h.iter_done;
    c.n_full_evals = h.n_full_evals; c.n_partial_evals = h.n_partial_evals; c.jobs_total = h.jobs_total;
    c.slog_n = 0; c.slog_cap = hc->h_ctrl.slog_cap;
    hc->h_ctrl = c;
    hc->h_target = h.iter_done;
    hc->pending_gathered = nullptr;
    HIPCHK(hipMemcpy(hc->dev.ctrl, &c, sizeof(Ctrl), hipMemcpyHostToDevice));
    // hand-off buffers of the persistent kernel: tags are functions of the job counter and of iteration | chain, which
    // a roll-back repeats -- nothing an earlier run left there may match
    {
        const ChainsDev &d = hc->dev;
        HIPCHK(hipMemset(d.slots, 0, (size_t)d.slot_rep * d.slot_stride * sizeof(unsigned long long)));
        HIPCHK(hipMemset(d.pgran, 0, (size_t)d.n_chains * d.n_workers * d.pgran_stride * sizeof(unsigned long long)));
        HIPCHK(hipMemset(d.lo_gran, 0, (size_t)d.n_chains * 16 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(d.diag, 0, 24 * sizeof(unsigned long long)));      // (what a failed wait left for the error message; [24], [25] are counters)
        // The swap-record inbox too: its tags are bare iteration numbers, and the iterations after the saved one are about
        // to be run again (records and stop / error words of the first time must not be taken for the second).  For a
        // multi-rank job a load is therefore COLLECTIVE: every rank loads, then the ranks meet at a barrier before the next
        // htm_chains_run_lockstep_direct (no peer posts outside a run, so nothing lands in a cleared inbox before that).
        if (hc->d_inbox && hc->inbox_bytes) HIPCHK(hipMemset(hc->d_inbox, 0, hc->inbox_bytes));
    }
    hc->lik_iter.clear(); hc->lik_chain.clear(); hc->lik_val.clear();
    hc->smp_iter.clear(); hc->smp_chain.clear(); hc->smp_data.clear();
    if ((rc = stream_produce(hc, 1 << 16))) return rc;
    HIPCHK(hipStreamSynchronize(hc->side));
    return HTM_OK;
}

int htm_chains_get_state(htm_chains *hc, int chain, double *hypo, double *t_corr, double *vs, double *a_corr,
                         double *qs, double *temp, double *log_likelihood, int32_t n_propose[7], int32_t n_accept[7])
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    const ChainsDev &d = hc->dev;
    if (chain < 0 || chain >= d.n_chains) return fail(HTM_EINVAL, "chain %d out of range", chain);
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    const size_t c = chain;
    if (hypo) HIPCHK(hipMemcpy(hypo, d.hypo.x + c * d.hypo.nx, d.hypo.nx * sizeof(double), hipMemcpyDeviceToHost));
    if (t_corr) HIPCHK(hipMemcpy(t_corr, d.tc.x + c * d.S, d.S * sizeof(double), hipMemcpyDeviceToHost));
    if (a_corr) HIPCHK(hipMemcpy(a_corr, d.ac.x + c * d.S, d.S * sizeof(double), hipMemcpyDeviceToHost));
    if (vs) HIPCHK(hipMemcpy(vs, d.vs.x + c, sizeof(double), hipMemcpyDeviceToHost));
    if (qs) HIPCHK(hipMemcpy(qs, d.qs.x + c, sizeof(double), hipMemcpyDeviceToHost));
    if (temp) HIPCHK(hipMemcpy(temp, d.temp + c, sizeof(double), hipMemcpyDeviceToHost));
    if (log_likelihood) HIPCHK(hipMemcpy(log_likelihood, d.L + c, sizeof(double), hipMemcpyDeviceToHost));
    if (n_propose) HIPCHK(hipMemcpy(n_propose, d.n_propose + 7 * c, 7 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n_accept) HIPCHK(hipMemcpy(n_accept, d.n_accept + 7 * c, 7 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HTM_OK;
}

int htm_chains_share_gpu(htm_chains *hc, int ranks_on_this_gpu)
{
    if (!hc || ranks_on_this_gpu < 1) return fail(HTM_EINVAL, "bad argument");
    if (ranks_per_gpu_knob(nullptr) || !hc->plan.persist || ranks_on_this_gpu == 1) return HTM_OK;      // (an explicit setting, HTM_RANKS_PER_GPU, stands)
    // (a chain set that has already run keeps the launch shape it ran with: ADVICE r3 -- a world built around it must not fail)
    if (hc->launch_seq > 0) return HTM_OK;
    const long room = room_for_workers(hc->plan.blocks_fit, ranks_on_this_gpu);
    if (room < 1) return fail(HTM_ESTATE, "%d ranks on one GPU: not even one worker block per rank fits next to the masters", ranks_on_this_gpu);
    if (hc->dev.n_workers > room) hc->dev.n_workers = worker_blocks(hc->fwd->E, 8, room);
    hc->dev.n_wg = hc->dev.n_workers;
    return HTM_OK;
}

int htm_chains_get_loglik(htm_chains *hc, int chain, double *log_likelihood)
{
    if (!hc || !log_likelihood) return fail(HTM_EINVAL, "NULL argument");
    if (chain < 0 || chain >= hc->dev.n_chains) return fail(HTM_EINVAL, "chain %d out of range", chain);
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    HIPCHK(hipMemcpy(log_likelihood, hc->dev.L + chain, sizeof(double), hipMemcpyDeviceToHost));
    return HTM_OK;
}

int htm_chains_get_rng(htm_chains *hc, uint32_t state[4])
{
    if (!hc || !state) return fail(HTM_EINVAL, "NULL argument");
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    // mod_random state after spos draws = words spos..spos+3 of [x0, y0, z0, w0, out_0, out_1, ...]
    const long long sp = hc->h_ctrl.spos;
    for (int k = 0; k < 4; ++k) {
        const long long word = sp + k;
        if (word < 4) state[k] = hc->init_state[word];
        else HIPCHK(hipMemcpy(&state[k], hc->dev.stream.raw + ((word - 4) & hc->dev.stream.mask), sizeof(uint32_t),
                              hipMemcpyDeviceToHost));
    }
    return HTM_OK;
}

int htm_chains_lik_count(htm_chains *hc, int *n)
{
    if (!hc || !n) return fail(HTM_EINVAL, "NULL argument");
    *n = (int)hc->lik_iter.size();
    return HTM_OK;
}

int htm_chains_lik_read(htm_chains *hc, int32_t *iter, int32_t *chain, double *log_likelihood)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    const size_t n = hc->lik_iter.size();
    if (iter) memcpy(iter, hc->lik_iter.data(), n * sizeof(int32_t));
    if (chain) memcpy(chain, hc->lik_chain.data(), n * sizeof(int32_t));
    if (log_likelihood) memcpy(log_likelihood, hc->lik_val.data(), n * sizeof(double));
    return HTM_OK;
}

int htm_chains_sample_count(htm_chains *hc, int *n)
{
    if (!hc || !n) return fail(HTM_EINVAL, "NULL argument");
    *n = (int)hc->smp_iter.size();
    return HTM_OK;
}

int htm_chains_sample_read(htm_chains *hc, int k, int32_t *iter, int32_t *chain, double *vs, double *qs,
                           double *hypo, double *t_corr, double *a_corr)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    if (k < 0 || k >= (int)hc->smp_iter.size()) return fail(HTM_EINVAL, "sample %d out of range", k);
    const int nh = hc->dev.hypo.nx, S = hc->dev.S;
    const double *r = hc->smp_data.data() + (size_t)k * hc->rec_len;
    if (iter) *iter = hc->smp_iter[k];
    if (chain) *chain = hc->smp_chain[k];
    if (hypo) memcpy(hypo, r, nh * sizeof(double));
    if (t_corr) memcpy(t_corr, r + nh, S * sizeof(double));
    if (a_corr) memcpy(a_corr, r + nh + S, S * sizeof(double));
    if (vs) *vs = r[nh + 2 * S];
    if (qs) *qs = r[nh + 2 * S + 1];
    return HTM_OK;
}

int htm_chains_clear_records(htm_chains *hc)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    hc->lik_iter.clear(); hc->lik_chain.clear(); hc->lik_val.clear();
    hc->smp_iter.clear(); hc->smp_chain.clear(); hc->smp_data.clear();
    return HTM_OK;
}

int htm_chains_enable_steplog(htm_chains *hc, int capacity)
{
    if (!hc || capacity < 0) return fail(HTM_EINVAL, "bad argument");
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    if (capacity > 0) {
        if ((rc = dev_alloc(hc->pool, &hc->dev.slog_i, 8 * (size_t)capacity))) return rc;
        if ((rc = dev_alloc(hc->pool, &hc->dev.slog_d, 4 * (size_t)capacity))) return rc;
    }
    // the graph bakes ChainsDev by value: rebuild it with the new pointers
    if (hc->gexec) { (void)hipGraphExecDestroy(hc->gexec); hc->gexec = nullptr; }
    if (hc->graph) { (void)hipGraphDestroy(hc->graph); hc->graph = nullptr; }
    hc->dev_np.slog_i = hc->dev.slog_i; hc->dev_np.slog_d = hc->dev.slog_d;
    hc->h_ctrl.slog_n = 0; hc->h_ctrl.slog_cap = capacity;
    HIPCHK(hipMemcpy(&hc->dev.ctrl->slog_n, &hc->h_ctrl.slog_n, 2 * sizeof(int), hipMemcpyHostToDevice));
    return HTM_OK;
}

int htm_chains_steplog_read(htm_chains *hc, int *n, int32_t *irows, double *drows)
{
    if (!hc || !n) return fail(HTM_EINVAL, "NULL argument");
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    const int rows = std::min(hc->h_ctrl.slog_n, hc->h_ctrl.slog_cap);
    *n = rows;
    if (rows > 0 && irows) HIPCHK(hipMemcpy(irows, hc->dev.slog_i, 8 * (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (rows > 0 && drows) HIPCHK(hipMemcpy(drows, hc->dev.slog_d, 4 * (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
    return HTM_OK;
}

int htm_chains_last_run_stats(htm_chains *hc, double *device_us, int *graph_launches, int64_t *full_evals,
                              int64_t *partial_evals)
{
    if (!hc) return fail(HTM_EINVAL, "NULL handle");
    if (device_us) *device_us = hc->last_device_us;
    if (graph_launches) *graph_launches = hc->last_graph_launches;
    if (full_evals) *full_evals = hc->last_full;
    if (partial_evals) *partial_evals = hc->last_part;
    return HTM_OK;
}

// 1: the latest single-rank launch ran the free-running master's specialised instantiation (k_mcmc<.., 8>; master_stats reports
// loop 3 for it as for the generic one); 0: any other loop, or nothing launched yet
int htm_chains_fixed_master(htm_chains *hc, int *on, int *worker_blocks)
{
    if (!hc || !on) return fail(HTM_EINVAL, "NULL argument");
    *on = hc->last_fixed ? 1 : 0;      // (set by launch_mcmc from loop_for's answer)
    if (worker_blocks) *worker_blocks = hc->dev.n_workers;
    return HTM_OK;
}

int htm_chains_master_stats(htm_chains *hc, int *single_rank_loop, int *lockstep_loop, int64_t *flushes)
{
    if (!hc) return fail(HTM_EINVAL, "NULL argument");
    // (the specialised instantiation, 8, is reported as the free-running master it is: htm_chains_fixed_master tells them apart)
    const int run = loop_for(hc->plan, MODE_RUN, false), lock = loop_for(hc->plan, MODE_LOCKRUN, false);
    if (single_rank_loop) *single_rank_loop = !hc->plan.persist ? -1 : run == 8 ? 3 : run;
    if (lockstep_loop) *lockstep_loop = !hc->plan.persist ? -1 : lock;
    if (flushes) {
        HIPCHK(hipStreamSynchronize(hc->fwd->stream));
        unsigned long long v = 0;
        HIPCHK(hipMemcpy(&v, hc->dev.diag + 25, sizeof(v), hipMemcpyDeviceToHost));
        *flushes = (int64_t)v;
    }
    return HTM_OK;
}

int htm_chains_handoff_stats(htm_chains *hc, int64_t *orders_put_aside)
{
    if (!hc || !orders_put_aside) return fail(HTM_EINVAL, "NULL argument");
    HIPCHK(hipStreamSynchronize(hc->fwd->stream));
    unsigned long long v = 0;
    HIPCHK(hipMemcpy(&v, hc->dev.diag + 24, sizeof(v), hipMemcpyDeviceToHost));
    *orders_put_aside = (int64_t)v;
    return HTM_OK;
}

#ifdef HTM_STAMPS
/* diagnostic builds only: the pipelined master's event trace ({time, code << 48 | iteration << 8 | chain} pairs) */
int htm_chains_read_trace(htm_chains *hc, unsigned long long *out, int n_pairs)
{
#ifdef HTM_STAMPS
    if (!hc || !out || n_pairs > 8192) return fail(HTM_EINVAL, "bad argument");
    HIPCHK(hipStreamSynchronize(hc->fwd->stream));
    HIPCHK(hipMemcpy(out, hc->dev.stamps + 128, (size_t)n_pairs * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HTM_OK;
#else
    (void)hc; (void)out; (void)n_pairs;
    return fail(HTM_ESTATE, "not a diagnostic build");
#endif
}

int htm_chains_read_stamps(htm_chains *hc, unsigned long long out[128])
{
    HIPCHK(hipStreamSynchronize(hc->fwd->stream));
    HIPCHK(hipMemcpy(out, hc->dev.stamps, 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HTM_OK;
}
/* diagnostics of a wedged hand-off: out[0..7] = the order slot of `chain` (replica 0), out[8..8+2*n) = the first n workers'
 * partial-sum granules of that chain (n <= 28) */
int htm_chains_read_handoff(htm_chains *hc, int chain, unsigned long long out[64])
{
    (void)hipStreamSynchronize(hc->fwd->stream);
    const ChainsDev &d = hc->dev;
    if (chain < 0 || chain >= d.n_chains) return fail(HTM_EINVAL, "chain out of range");
    HIPCHK(hipMemcpy(out, d.slots + (size_t)chain * kGranPerSlot, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const int n = std::min(28, d.n_workers);
    for (int k = 0; k < n; ++k)
        HIPCHK(hipMemcpy(out + 8 + 2 * k, d.pgran + ((size_t)chain * d.n_workers + k) * d.pgran_stride, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HTM_OK;
}
#endif

}  // extern "C"
