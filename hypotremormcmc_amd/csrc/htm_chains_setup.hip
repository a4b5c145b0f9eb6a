// htm_chains_setup.hip -- a chain set's set-up (C ABI: include/htm_hip.h; the map of the units: htm_host.hpp): its launch plan
// (htm_plan.hpp: which chain-master loop a launch takes, and its shape), htm_chains_create and what it allocates, group by
// group, htm_chains_destroy, htm_chains_share_gpu and the inbox of the in-kernel exchange.  The one host unit that takes
// anything from the loops, and sizes only: FlowShared, MbShared and kXSlots (htm_flow.hpp), PipeShared and pipe_ring_bytes
// (htm_pipe.hpp), mcmc_threads (htm_mcmc.hpp); the barrier loop's StepSharedT is htm_handoff.hpp's, so htm_step.hpp is not
// needed.  No kernel is instantiated or defined here.
#include "htm_host.hpp"
#include "htm_flow.hpp"
#include "htm_pipe.hpp"
#include "htm_mcmc.hpp"

using namespace htm;

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

// ---- what htm_chains_create allocates and uploads, group by group.  Each returns at its first failure; the caller's guard
// ---- frees what was made.
int alloc_params(htm_chains *hc, const htm_chains_init *init, const Knobs &kn)
{
    ChainsDev &d = hc->dev;
    const size_t n = (size_t)d.n_chains;
    const ParamLayout pl = param_layout(n, (size_t)d.S, (size_t)d.E);
    const size_t total = pl.total;
    int rc;
    if ((rc = dev_alloc(hc->pool, &d.xall, total)) || (rc = dev_alloc(hc->pool, &d.muall, total)) ||
        (rc = dev_alloc(hc->pool, &d.sgall, total)) || (rc = dev_alloc(hc->pool, &d.stall, total)) ||
        (rc = dev_alloc(hc->pool, &d.ptall, total))) return rc;
    // the five per-field arrays on the host, group by group (a field that is not given: mu 0, sigma 1, step size 0, prior type 0)
    const htm_model_init *in[5] = {&init->vs, &init->t_corr, &init->qs, &init->a_corr, &init->hypo};
    ModelDev *md[5] = {&d.vs, &d.tc, &d.qs, &d.ac, &d.hypo};
    const char *name[5] = {"vs", "t_corr", "qs", "a_corr", "hypo"};
    std::vector<double> x(total), mu(total, 0.0), sg(total, 1.0), stp(total, 0.0), r2(total);
    std::vector<int32_t> pt(total, 0);
    for (int g = 0; g < 5; ++g) {
        if (!in[g]->x) return fail(HTM_EINVAL, "%s.x is NULL", name[g]);
        const size_t off = pl.g[g].off, cnt = n * pl.g[g].nx;
        std::copy(in[g]->x, in[g]->x + cnt, x.begin() + off);
        if (in[g]->mu) std::copy(in[g]->mu, in[g]->mu + cnt, mu.begin() + off);
        if (in[g]->sigma) std::copy(in[g]->sigma, in[g]->sigma + cnt, sg.begin() + off);
        if (in[g]->step_size) std::copy(in[g]->step_size, in[g]->step_size + cnt, stp.begin() + off);
        if (in[g]->prior_type) std::copy(in[g]->prior_type, in[g]->prior_type + cnt, pt.begin() + off);
        ModelDev &m = *md[g];      // the group's window of the five allocations
        m.nx = (int)pl.g[g].nx;
        m.x = d.xall + off; m.mu = d.muall + off; m.sigma = d.sgall + off; m.step = d.stall + off; m.ptype = d.ptall + off;
    }
    HIPCHK(hipMemcpy(d.xall, x.data(), total * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.muall, mu.data(), total * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.sgall, sg.data(), total * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.stall, stp.data(), total * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.ptall, pt.data(), total * sizeof(int32_t), hipMemcpyHostToDevice));
    for (size_t k = 0; k < total; ++k) r2[k] = 1.0 / (2.0 * sg[k] * sg[k]);
    if ((rc = dev_upload(hc->pool, &d.rs2all, r2.data(), total))) return rc;
    // the packed records the chain steps read (PriorRec), and whether every chain has chain 0's
    std::vector<PriorRec> pr(total);
    for (size_t k = 0; k < total; ++k) { pr[k].mu = mu[k]; pr[k].rs2 = r2[k]; pr[k].step = stp[k]; pr[k].ptype = pt[k]; pr[k].pad = 0; }
    bool same = kn.prior_same;      // (off for diagnostics: every chain reads its own records)
    for (int g = 0; g < 5 && same; ++g)
        for (size_t c = 1; c < n && same; ++c)
            same = memcmp(&pr[pl.g[g].off + c * pl.g[g].nx], &pr[pl.g[g].off], pl.g[g].nx * sizeof(PriorRec)) == 0;
    PriorRec *dp = nullptr;
    if ((rc = dev_upload(hc->pool, &dp, pr.data(), total))) return rc;
    d.prior = dp; d.prior_same = same ? 1 : 0;
    // (a Rayleigh prior, prior_type 1, on some element of the four groups before hypo)
    d.rayleigh14 = std::find(pt.begin(), pt.begin() + pl.g[4].off, 1) != pt.begin() + pl.g[4].off;
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
    if ((rc = dev_zeros(hc->pool, &d.prop, nc))) return rc;
    if ((rc = dev_zeros(hc->pool, &d.desc, 1))) return rc;
    if ((rc = dev_alloc(hc->pool, &d.partial, (size_t)nc * std::max(h->n_wg, 256)))) return rc;      // (<= 256 workers whatever the launch shape)
    return dev_zeros(hc->pool, &d.ps, 1);
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
// swap record that the rank hands to the other ranks.  (The regions and their sizes: handoff_regions, htm_host.hpp.)
int alloc_region(htm_chains *hc, int which)
{
    const HandoffRegion r = handoff_regions(hc)[which];
    return dev_zeros(hc->pool, r.p, r.words);
}

int alloc_handoff(htm_chains *hc)
{
    ChainsDev &d = hc->dev;
    int rc;
    if ((rc = alloc_region(hc, kRegSlots))) return rc;
    unsigned long long *mbw = nullptr;
    if ((rc = dev_alloc(hc->pool, &mbw, sizeof(MbShared) / sizeof(unsigned long long)))) return rc;
    d.mb = reinterpret_cast<MbShared *>(mbw);
    if ((rc = dev_zeros(hc->pool, &d.prev_mid, (size_t)d.n_chains))) return rc;
    if ((rc = alloc_region(hc, kRegLoGran))) return rc;
    if ((rc = alloc_region(hc, kRegPgran))) return rc;
    return dev_zeros(hc->pool, &d.swap_rec, swap_words(d.n_chains));
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
    if ((rc = alloc_region(hc, kRegDiag))) return rc;
    d.stamps = nullptr;
#ifdef HTM_STAMPS
    if ((rc = dev_zeros(hc->pool, &d.stamps, 128 + 2 * 8192))) return rc;      // (+ the event trace of htm_pipe.hpp)
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
    hc->sized = kn.sized;
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

}  // extern "C"

namespace htm {

// ---- persistent lock-step: swap records exchanged inside the launch (exchange_post / exchange_finish in htm_handoff.hpp) --------
int xchg_alloc(htm_chains *hc)
{
    if (hc->d_inbox) return HTM_OK;
    ChainsDev &d = hc->dev;
    d.xg = 2 * (int)swap_words(d.n_chains) + 2;
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

}  // namespace htm
