// htm_chains_state.hip -- what is read of a chain set, and what is put back (C ABI: include/htm_hip.h; the map of the units:
// htm_host.hpp): checkpoints, the chains' state, the drained records, the step log and the statistics of the last run.  Plain
// copies between the handle's buffers and the caller: nothing here launches a kernel or knows a loop, so the unit sees the types
// of htm_host.hpp only.  What needs the kernels' stream goes through htm_chains_sync and the few functions that cross units.
#include "htm_host.hpp"

using namespace htm;

// ---- checkpoint / resume ------------------------------------------------------------------------------
// A blob (version 2) is this header, 80 bytes in the host's byte order, and then the fields of ckpt_fields back to back.
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

// the body in file order: the parameter vector (param_layout, htm_host.hpp), [n] temperatures, [n] log-likelihoods, the
// [n][7] proposal and acceptance counters, and [n] what each chain's last step was (prev_mid: decides which event its next
// full evaluation leaves to the chain's own wave, so that a continued run sums in the order of the uninterrupted one)
struct CkptField { void *p; size_t bytes; };
size_t ckpt_total(const htm_chains *hc) { return param_layout(hc->dev.n_chains, hc->dev.S, hc->dev.E).total; }
std::array<CkptField, 6> ckpt_fields(const htm_chains *hc)
{
    const ChainsDev &d = hc->dev;
    const size_t n = d.n_chains;
    return {{{d.xall, ckpt_total(hc) * sizeof(double)}, {d.temp, n * sizeof(double)}, {d.L, n * sizeof(double)},
             {d.n_propose, 7 * n * sizeof(int32_t)}, {d.n_accept, 7 * n * sizeof(int32_t)}, {d.prev_mid, n * sizeof(int32_t)}}};
}
size_t ckpt_bytes(const htm_chains *hc)
{
    size_t b = sizeof(CkptHeader);
    for (const CkptField &f : ckpt_fields(hc)) b += f.bytes;
    return b;
}
}  // namespace

// ====================================================================================================
extern "C" {

int htm_chains_iterations_done(htm_chains *hc, int *n)
{
    if (!hc || !n) return fail(HTM_EINVAL, "NULL argument");
    int rc = htm_chains_sync(hc);
    if (rc) return rc;
    *n = hc->h_ctrl.iter_done;
    return HTM_OK;
}

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
    for (const CkptField &f : ckpt_fields(hc)) { HIPCHK(hipMemcpy(p, f.p, f.bytes, hipMemcpyDeviceToHost)); p += f.bytes; }
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
    for (const CkptField &f : ckpt_fields(hc)) { HIPCHK(hipMemcpy(f.p, p, f.bytes, hipMemcpyHostToDevice)); p += f.bytes; }
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
    // a roll-back repeats -- nothing an earlier run left there may match (of diag: what a failed wait left for the error message).
    // The swap-record inbox too: its tags are bare iteration numbers, and the iterations after the saved one are about
    // to be run again (records and stop / error words of the first time must not be taken for the second).  For a
    // multi-rank job a load is therefore COLLECTIVE: every rank loads, then the ranks meet at a barrier before the next
    // htm_chains_run_lockstep_direct (no peer posts outside a run, so nothing lands in a cleared inbox before that).
    for (const HandoffRegion &r : handoff_regions(hc))
        if (*r.p && r.words) HIPCHK(hipMemset(*r.p, 0, (r.words - r.kept) * sizeof(unsigned long long)));
    clear_host_records(hc);
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
    clear_host_records(hc);
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

// the chain count and the ring size the latest single-rank launch held as literals (k_mcmc_sized); 0, 0: it was no sized launch
int htm_chains_sized_master(htm_chains *hc, int *n_chains, int *ring)
{
    if (!hc || !n_chains || !ring) return fail(HTM_EINVAL, "NULL argument");
    *n_chains = hc->last_sized_nc; *ring = hc->last_sized_ring;      // (set by launch_mcmc with last_fixed)
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
