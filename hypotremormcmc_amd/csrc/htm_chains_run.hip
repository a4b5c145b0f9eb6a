// htm_chains_run.hip -- running a chain set (C ABI: include/htm_hip.h; the map of the units: htm_host.hpp): looks a launch's
// loop up in the kernel table of htm_host.hpp (the instantiations themselves are compiled by the loop units, htm_loop_*.hip,
// none here) and launches it; produces the random stream ahead of the chains; the run drivers (htm_chains_run, _profile,
// _run_lockstep, _run_lockstep_direct), the per-iteration lock-step calls, htm_chains_sync / _drain and the connection of
// the in-kernel exchange.  This unit owns the small kernels of htm_chains_kernels.hpp and is the only one to include it.
#include "htm_host.hpp"
#include "htm_chains_kernels.hpp"

#include <chrono>
#include <thread>

using namespace htm;

namespace htm {

// ---- the kernel table's two lookups (htm_host.hpp): the rows of every loop unit -------------------------------------------
// Three or more stations per lane run the instantiation for any station count (<0, ..>), as they always have; the fp32
// forward and the masters of htm_flow.hpp / htm_pipe.hpp other than MK 3 and 4 exist for one or two stations per lane only.
// (sized: a row that holds the chain count and / or the ring size as literals -- LoopRow::nc, ::ring, 0: any -- for a launch with
// `nc` chains on a ring of `ring`; the rows of before hold neither)
static const LoopRow *find_row(bool step, bool wide, int nch, bool fp32, int mk, bool sized = false, int nc = 0, int ring = 0)
{
    const int n = (nch == 1 || nch == 2) ? nch : 0;
    const LoopRows units[] = {loop_rows_free(), loop_rows_lock(), loop_rows_barrier(), loop_rows_wide(), loop_rows_pipe()};
    for (const LoopRows &u : units)
        for (size_t k = 0; k < u.n; ++k) {
            const LoopRow &r = u.rows[k];
            if (r.step == step && r.wide == wide && r.nch == n && r.fp32 == fp32 && r.mk == mk && sized == (r.nc != 0 || r.ring != 0) &&
                (r.nc == 0 || r.nc == nc) && (r.ring == 0 || r.ring == ring)) return &r;
        }
    return nullptr;
}
static const LoopKernel *kernel_of(const LoopRow *r) { return r ? &r->k : nullptr; }
const LoopKernel *mcmc_kernel(int nch, bool fp32, int mk, bool wide) { return kernel_of(find_row(false, wide, nch, fp32, mk)); }
const LoopKernel *step_kernel(int nch, bool fp32, bool wide) { return kernel_of(find_row(true, wide, nch, fp32, 0)); }
const LoopRow *sized_kernel(int nch, bool fp32, int mk, int nc, int ring) { return find_row(false, false, nch, fp32, mk, true, nc, ring); }

int no_kernel(const htm_chains *hc, const char *what, int mk)
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
    // Loop 8 with this launch's chain count and ring as literals (k_mcmc_sized), where a row holds exactly these and the mirror is the
    // full one with its step sizes (what loop 8 is planned with: checked here against the values the kernel is handed).  Any other
    // launch runs k_mcmc<.., 8> as planned -- the plan does not know the sized kernels.  HTM_SIZED=0: never.
    int sized_nc = 0, sized_ring = 0;
    if (mk == 8 && hc->sized && hc->dev.mirror_steps != 0 &&
        hc->dev.mirror_n == 2 * hc->dev.n_chains + 2 * hc->dev.n_chains * hc->dev.S && hc->dev.S == 64 * h->nch) {
        if (const LoopRow *rs = sized_kernel(h->nch, h->dev.fp32 != 0, mk, hc->dev.n_chains, lp.ring_size)) {
            k = &rs->k; sized_nc = rs->nc; sized_ring = rs->ring;
        }
    }
    // (a sized kernel holds what it is handed as literals: the launch's values must be exactly those, and its 512 threads)
    if ((sized_nc && hc->dev.n_chains != sized_nc) || (sized_ring && l.ring_size != sized_ring) || ((sized_nc || sized_ring) && k->threads != 512))
        return fail(HTM_EINVAL, "the sized chain master for %d chains and a ring of %d does not fit this launch (%d chains, ring %d, %d threads)",
                    sized_nc, sized_ring, hc->dev.n_chains, l.ring_size, k->threads);
    // (the specialised master's chain wave keeps its chain's correction pair in registers, htm_flow.hpp FlowOwn: a wave per chain)
    if (mk == 8 && hc->dev.n_chains > std::min(k->threads / 64, 8))
        return fail(HTM_EINVAL, "the specialised chain master runs one chain per wave: %d chains, %d threads", hc->dev.n_chains, k->threads);
    if (mode == MODE_RUN) { hc->last_fixed = mk == 8; hc->last_sized_nc = sized_nc; hc->last_sized_ring = sized_ring; }
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

// Wait for the chain kernels' stream, but never forever: every device-side wait is bounded (workers 30 s, master
// 5 s per hand-over), so a stream that has not drained after kWatchdogSeconds means the device is wedged -- report
// it instead of hanging the caller (HTM_WATCHDOG_S overrides the limit; 0 = wait without limit).
int bounded_stream_sync(htm_chains *hc, const char *what)
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

}  // namespace htm

namespace {

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

// ====================================================================================================
extern "C" {

static int flush_pending(htm_chains *hc)
{
    if (!hc->pending_gathered) return HTM_OK;
    const double *g = hc->pending_gathered;
    hc->pending_gathered = nullptr;
    return launch_step(hc, MODE_APPLY, hc->h_target, g);
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
    case -22: return fail(HTM_ESTATE, "a sized chain master (k_mcmc_sized) was launched with another chain count, ring size or mirror than it is built for "
                          "(%d chains, ring %d, mirror %d)", hc->dev.n_chains, hc->plan.ring_size, hc->dev.mirror_n);
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
        // (the last n records of a triple of vectors; a record's values are a row of rl doubles)
        auto sort_tail = [](size_t n, size_t rl, std::vector<int32_t> &iter, std::vector<int32_t> &chain, std::vector<double> &val) {
            if (n < 2) return;
            const size_t o = iter.size() - n;
            std::vector<size_t> idx(n);
            for (size_t k = 0; k < n; ++k) idx[k] = o + k;
            std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return iter[a] != iter[b] ? iter[a] < iter[b] : chain[a] < chain[b]; });
            std::vector<int32_t> it(n), ch(n); std::vector<double> v(n * rl);
            for (size_t k = 0; k < n; ++k) {
                it[k] = iter[idx[k]]; ch[k] = chain[idx[k]];
                std::copy(val.begin() + idx[k] * rl, val.begin() + (idx[k] + 1) * rl, v.begin() + k * rl);
            }
            std::copy(it.begin(), it.end(), iter.begin() + o); std::copy(ch.begin(), ch.end(), chain.begin() + o);
            std::copy(v.begin(), v.end(), val.begin() + o * rl);
        };
        sort_tail(std::max(nl, 0), 1, hc->lik_iter, hc->lik_chain, hc->lik_val);
        sort_tail(std::max(ns, 0), hc->rec_len, hc->smp_iter, hc->smp_chain, hc->smp_data);
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

// ---- the bracket of a run driver: the statistics of one call (htm_chains_last_run_stats), evaluations counted on the device,
// ---- HIP events on the kernels' stream.  h_ctrl is current at both ends.
static int run_open(htm_chains *hc)
{
    hc->run_full0 = hc->h_ctrl.n_full_evals; hc->run_part0 = hc->h_ctrl.n_partial_evals;
    hc->last_graph_launches = 0;
    HIPCHK(hipEventRecord(hc->ev0, hc->fwd->stream));
    return HTM_OK;
}

// (ev1 has been recorded and reached)
static int run_stats(htm_chains *hc)
{
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, hc->ev0, hc->ev1));
    hc->last_device_us = 1000.0 * ms;
    hc->last_full = hc->h_ctrl.n_full_evals - hc->run_full0;
    hc->last_part = hc->h_ctrl.n_partial_evals - hc->run_part0;
    return HTM_OK;
}

static int run_close(htm_chains *hc)
{
    HIPCHK(hipEventRecord(hc->ev1, hc->fwd->stream));
    HIPCHK(hipEventSynchronize(hc->ev1));
    const int rc = run_stats(hc);
    return rc ? rc : drain_records(hc);
}

// keep the random stream about half a ring ahead of the chains (asynchronous, on the side stream)
static int top_up_stream(htm_chains *hc)
{
    const long long ahead = hc->n_hop - hc->h_ctrl.spos;
    return ahead < hc->cap / 2 ? stream_produce(hc, std::min<long long>(hc->cap / 2 - ahead + 4096, 1 << 18)) : HTM_OK;
}

// Single-rank main loop on the persistent kernel: one k_mcmc launch runs until the target, a full record
// buffer or the end of the produced random stream; no graph, no per-hand-over launches.
static int run_persistent(htm_chains *hc, int n_iter)
{
    int rc;
    hc->h_target = hc->h_ctrl.iter_done + n_iter;
    if ((rc = run_open(hc))) return rc;
    while (hc->h_ctrl.iter_done < hc->h_target) {
        // a launch may run as far as the produced stream reaches
        const long long fed = (hc->n_hop - hc->h_ctrl.spos) / (6 * hc->dev.n_chains + 4) - 2;
        const int target = (int)std::min<long long>(hc->h_target, hc->h_ctrl.iter_done + std::max<long long>(1, fed));
        if ((rc = launch_mcmc(hc, MODE_RUN, target, nullptr))) return rc;
        hc->last_graph_launches += 1;
        if ((rc = top_up_stream(hc))) return rc;      // (while the launch runs)
        if ((rc = read_ctrl(hc))) return rc;
        if ((rc = ctrl_error(hc))) return rc;
        if (hc->h_ctrl.stop == 2) HIPCHK(hipStreamSynchronize(hc->side));
        if (hc->h_ctrl.stop) { if ((rc = drain_records(hc))) return rc; }
    }
    return run_close(hc);
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
    if ((rc = run_open(hc))) return rc;
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
        if ((rc = top_up_stream(hc))) return rc;
        if (hc->h_ctrl.stop == 2) HIPCHK(hipStreamSynchronize(hc->side));   // underrun: wait for the producer
        if (hc->h_ctrl.stop) { if ((rc = drain_records(hc))) return rc; }
    }
    return run_close(hc);
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
    const size_t words = swap_words(hc->dev.n_chains);
    // records a rank may hold on the device between drains: n_chains per iteration at most
    const int drain_every = std::max(1, std::min(hc->dev.cap_lik, hc->dev.cap_smp) / (2 * hc->dev.n_chains) - 2);
    int k = 0, since_drain = 0, rc;
    if ((rc = read_ctrl(hc))) return rc;
    if ((rc = run_open(hc))) return rc;
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
    if ((rc = read_ctrl(hc))) return rc;          // flushes the last swap, waits for the stream (ev1 lies before both)
    if ((rc = ctrl_error(hc))) return rc;
    return run_stats(hc);                         // (the records stay on the device: the caller drains)
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
    if ((size_t)d0.n_procs * swap_words(d0.n_chains) > (size_t)kGathStage)
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
    int rc = dev_zeros(hc->pool, &d_res, 1);
    if (rc) return rc;
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
    if ((rc = run_open(hc))) return rc;
    while (hc->h_ctrl.iter_done < hc->h_target) {
        // the launch reads the produced stream's extent once, at its start: have a good stretch ready
        if ((rc = top_up_stream(hc))) return rc;
        HIPCHK(hipStreamWaitEvent(h->stream, hc->ev_side, 0));      // (the producer takes ~0.1 ms per 2^18 positions)
        const int before = hc->h_ctrl.iter_done;
        if ((rc = launch_mcmc(hc, MODE_LOCKRUN, hc->h_target, nullptr))) return rc;
        hc->last_graph_launches += 1;
        if ((rc = top_up_stream(hc))) return rc;        // again while the launch runs (for the next one)
        if ((rc = read_ctrl(hc))) return rc;
        if ((rc = ctrl_error(hc))) return rc;
        if (hc->h_ctrl.stop) { if ((rc = drain_records(hc))) return rc; }
        else if (hc->h_ctrl.iter_done == before && hc->h_ctrl.iter_done < hc->h_target)
            return fail(HTM_ESTATE, "lock-step launch made no progress at iteration %d", before);
    }
    return run_close(hc);
}

int htm_chains_swap_record(htm_chains *hc, void **d_record, size_t *record_bytes)
{
    if (!hc || !d_record || !record_bytes) return fail(HTM_EINVAL, "NULL argument");
    *d_record = hc->dev.swap_rec;
    *record_bytes = swap_words(hc->dev.n_chains) * sizeof(double);
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
    const size_t words = swap_words(hc->dev.n_chains);
    HIPCHK(hipMemcpyAsync(record, hc->dev.swap_rec, words * sizeof(double), hipMemcpyDeviceToHost, hc->fwd->stream));
    return bounded_stream_sync(hc, "waiting for the iteration's swap record");
}

int htm_chains_step_end_host(htm_chains *hc, const double *gathered_records)
{
    if (!hc || !gathered_records) return fail(HTM_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(hc->fwd->device));
    const size_t words = swap_words(hc->dev.n_chains) * (size_t)hc->dev.n_procs;
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

}  // extern "C"
