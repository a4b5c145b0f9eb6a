// htm_host.hpp -- what the host translation units of libhtm_hip.so share.  Internal: not installed, not part of the ABI
// (include/htm_hip.h is).
//
//   htm_forward.hip        htm_forward_* of step 5, htm_device_*, the last-error string, the self-tests and htm_rng_jump
//   htm_locate.hip         htm_forward_locate* (the location posteriors on a grid, their marginal over draws, the draws' evidences,
//                          the stacked density) on a forward handle; the one unit with the kernels of htm_locate.hpp
//   htm_locate_plan.hpp    the batch plan of a locate call: the grid's tiles, every device array's length, the bytes under
//                          HTM_LOCATE_MB and the events per batch, worked out by plain functions without a device and without
//                          HIP.  Ask for the plan of a shape with htm_forward_locate_plan (no GPU needed)
//   htm_chains_setup.hip   the chain sets' part of the C ABI, four units, none of which instantiates a k_mcmc.  Set-up: the plan
//                          (htm_chains_plan, htm_chains_get_plan), htm_chains_create / _destroy / _share_gpu, the inbox of
//                          the in-kernel exchange.  The only unit that takes sizes from the loops (htm_flow.hpp, htm_pipe.hpp,
//                          htm_mcmc.hpp); emits no kernel
//   htm_chains_run.hip     the kernel table's lookups, the launches, the random-stream producer, the run drivers, the
//                          lock-step calls and the exchange's connection; the one unit with htm_chains_kernels.hpp
//   htm_chains_state.hip   checkpoints and everything that reads a chain set: getters, records, step log, statistics
//   htm_comm.hip           RCCL bound at run time: htm_comm_*, htm_chains_run_lockstep_comm.  These two see the types of
//                          this header and nothing of the hand-off, the workers or the loops
//   htm_plan.hpp          the launch plan of a chain set: which loop each mode takes (loop_for) and the launch shape, worked out
//                          by plain functions without a device; kept in htm_chains::plan.  Ask for the plan of a shape with
//                          htm_chains_plan (no GPU needed), for the plan of a chain set with htm_chains_get_plan
//   htm_loop_*.hip         one unit per family of chain-master loops: nothing but its rows of the kernel table below
//                          (made with htm_loop_rows.hpp).  A unit includes htm_loop_rows.hpp and the header of the ONE loop it builds
//   device headers         htm_device.hpp -> htm_stream.hpp -> htm_handoff.hpp (what the loops and the workers share) ->
//                          htm_worker.hpp (worker_body) -> htm_mcmc.hpp (k_mcmc, k_mcmc_wide: declares the loops, includes none).
//                          The loops, each on htm_handoff.hpp: htm_step.hpp (with barriers: step_body, k_step, k_step_wide),
//                          htm_flow.hpp (free-running: flow_body), htm_pipe.hpp (pipelined: pipe_body; takes flow_swap_at from
//                          htm_flow.hpp).  tests/test_loop_unit_headers.py holds every unit to the headers of its loop
//   htm_steps.hip          steps 1-4, 6, the convergence diagnostics and the location error ellipsoids (htm_hypo_ellipsoid*);
//                          touches neither htm_forward nor htm_chains
//   htm_steps_host.hpp     the host idioms of htm_steps.hip and htm_locate.hip: StreamBuf, a stream-ordered workspace that
//                          hands out typed pieces; DevPool, the device arrays of a host-pointer form (alloc, upload, download)
//   htm_limits.hpp         kMaxWorkItems, the limit of one launch; env_mib, an HTM_x_MB switch.  Without HIP, for the plans
//
// Host code is plain C++17 + the HIP runtime: no torch, no third-party dependency.  There is no CPU fallback on purpose:
// every entry point needs a usable HIP device and fails with HTM_ENODEVICE otherwise.
#pragma once
#include "htm_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "htm_kernels.hpp"
#include "htm_plan.hpp"
#include "htm_stream.hpp"

// (nothing declared here is exported from the shared library: the C ABI is)
#pragma GCC visibility push(hidden)

namespace htm {

// Sets the calling thread's last-error string (htm_last_error: one object for the whole library, htm_forward.hip) and returns `code`.
int fail(int code, const char *fmt, ...);

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(HTM_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,     \
                        __LINE__);                                                                     \
    } while (0)

int use_device(int device);

template <typename T>
int dev_alloc(std::vector<void *> &pool, T **p, size_t n)
{
    void *q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
    pool.push_back(q);
    *p = static_cast<T *>(q);
    return HTM_OK;
}

template <typename T>
int dev_upload(std::vector<void *> &pool, T **p, const T *src, size_t n)
{
    int rc = dev_alloc(pool, p, n);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return HTM_OK;
}

template <typename T>
int dev_zeros(std::vector<void *> &pool, T **p, size_t n)
{
    int rc = dev_alloc(pool, p, n);
    if (rc) return rc;
    HIPCHK(hipMemset(*p, 0, n * sizeof(T)));
    return HTM_OK;
}

inline int nch_for(int S) { return S <= 64 ? 1 : S <= 128 ? 2 : S <= 256 ? 4 : 0; }

// ---- GF(2) algebra of mod_random's xorshift128 (reference src/mod_random.f90:63-71) ----------------------------
// One step is linear in the 128 state bits (x | y << 32 | z << 64 | w << 96): state' = T * state.  Powers of T let
// the device start any 64-draw segment of the stream directly (htm_stream.hpp, k_rawgen) and the host jump over any
// number of draws (htm_rng_jump).  A matrix is stored as its 128 columns.
struct Bits128 { uint32_t w[4]; };
using Mat128 = std::array<Bits128, 128>;
Bits128 gf2_matvec(const Mat128 &M, const Bits128 &v);
const std::vector<Mat128> &xs_powers();      // P[k] = T^(2^k), k = 0..63

}  // namespace htm

struct htm_forward {
    int device = 0, S = 0, E = 0, nch = 1;
    hipStream_t own_stream = nullptr, stream = nullptr;
    htm::FwdDev dev{};
    std::vector<void *> pool;
    int n_wg = 0, epw = 1;
    // scratch for the host-pointer entry points (one model)
    double *d_hypo = nullptr, *d_tc = nullptr, *d_ac = nullptr, *d_scal = nullptr, *d_partial = nullptr;
    double *d_syn = nullptr;
    // scratch for batches
    double *d_bpartial = nullptr; size_t bpartial_cap = 0;
    double *d_bmodels = nullptr;  size_t bmodels_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_wd = nullptr;
    // packed per-event records of the specialised chain master (FwdDev::obs_pack), fp64 and fp32 forward: built when a chain set
    // that can run that master is created on this forward (ensure_obs_pack), and for the other precision when it is switched to
    void *d_pack64 = nullptr, *d_pack32 = nullptr;
    bool pack_wanted = false;
    // [E] every event's own share of dev.const_sum, per data type: sum_j (log_2pi_half + log stdv(j, event)) in station order
    // (htm_forward_locate: an event's term of the log-likelihood)
    double *d_lconst_t = nullptr, *d_lconst_a = nullptr;
    // htm_forward_locate_set_precision: the three locate entry points evaluate the synthetics in fp32 (dev.fp32 is step 5's)
    bool loc_fp32 = false;
};

struct htm_chains {
    htm_forward *fwd = nullptr;
    htm::ChainsDev dev{};
    htm::Ctrl h_ctrl{};
    std::vector<void *> pool;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    int pairs = 32;
    htm::LoopPlan plan;        // which loop a launch takes and its shape (htm_plan.hpp), as htm_chains_create planned it
    htm::PlanDevice seen;      // the device facts it planned with
    int h_target = 0;          // host copy of the iteration target
    int rec_len = 0;
    std::vector<int32_t> lik_iter, lik_chain, smp_iter, smp_chain;
    std::vector<double> lik_val, smp_data;
    double last_device_us = 0.0;
    int last_graph_launches = 0;
    long long run_full0 = 0, run_part0 = 0, last_full = 0, last_part = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_wd = nullptr;
    // random-stream service (htm_stream.hpp): produced on a side stream ahead of consumption
    hipStream_t side = nullptr;
    hipEvent_t ev_side = nullptr;
    long long cap = 0;                         // ring capacity (positions)
    long long n_raw = 0, n_tr = 0, n_rec = 0, n_hop = 0;   // positions produced per stage (host view)
    long long spos_lo = 0, spos_hi = 0;        // bounds on the consumed position since the last sync
    const double *pending_gathered = nullptr;  // lock-step: records whose swap the next k_step applies
    double *d_gath_host = nullptr, *h_gath_pinned = nullptr;   // staging buffers of htm_chains_step_end_host
    unsigned long long launch_seq = 0;         // k_mcmc launches of this chain set so far (the kernels' launch index)
    bool last_fixed = false;                   // the latest MODE_RUN launch was the specialised instantiation (k_mcmc<.., 8>, sized or not)
    int last_sized_nc = 0, last_sized_ring = 0;      // ... the sized one (k_mcmc_sized) with these literals; 0, 0: not
    bool sized = true;                         // HTM_SIZED=0 at htm_chains_create: never the sized instantiation (A/B runs, tests)
    bool ctrl_fresh = false;                   // h_ctrl is the device's control block as of an idle stream (no launch since it was read)
    htm::ChainsDev dev_np{};                   // view for the non-persistent kernels (partial sums per k_full tile)
    uint32_t init_state[4] = {0, 0, 0, 0};     // mod_random state at stream position 0
    // in-kernel exchange of the swap records (persistent lock-step): this rank's inbox, the peers' inboxes as mapped here
    unsigned long long *d_inbox = nullptr;
    size_t inbox_bytes = 0;
    std::vector<void *> peer_maps;             // hipIpcOpenMemHandle mappings to close
    unsigned probe_calls = 0;                  // htm_chains_xchg_probe calls so far (part of the probe's tokens)
    unsigned long long **d_outbox = nullptr;
    bool xchg_ready = false;
    htm::u32x4 *d_jump = nullptr;              // [kJumpLevels][128] columns of T^(64 * 2^b) (k_rawgen)
    int gen_par = 0;                           // which half of StreamDev::gen holds the current generator state
    double th[4] = {0, 0, 0, 0};
};

namespace htm {

// ---- the functions that cross units -------------------------------------------------------------------------------
// htm_forward.hip
int launch_full(htm_forward *h, const FullJob &jb, int gy);
int full_batch_dev(htm_forward *h, int n_models, const double *d_hypo, const double *d_tc, const double *d_vs,
                   const double *d_ac, const double *d_qs, double *d_L);
int ensure_obs_pack(htm_forward *h);
// htm_chains_run.hip
int launch_mcmc(htm_chains *hc, int mode, int target, const double *gathered);
int launch_step(htm_chains *hc, int mode, int target, const double *gathered);
int no_kernel(const htm_chains *hc, const char *what, int mk);
int stream_produce(htm_chains *hc, long long n);
int bounded_stream_sync(htm_chains *hc, const char *what);
// htm_chains_setup.hip
int xchg_alloc(htm_chains *hc);

// ---- a chain set's layouts, each written down once ----------------------------------------------------------------
// The rank's parameter vector (ChainsDev::xall and the per-field arrays beside it): five groups in the order of the
// proposal types, [vs | t_corr | qs | a_corr | hypo], group k holding n_chains rows of nx elements from `off` on.  (The
// kernels work the same offsets out for themselves: group_offsets in htm_handoff.hpp, chain_pass in htm_step.hpp.)
struct ParamLayout {
    struct Group { size_t off, nx; } g[5];
    size_t total;
};
inline ParamLayout param_layout(size_t n_chains, size_t S, size_t E)
{
    ParamLayout l{};
    const size_t nx[5] = {1, S, 1, S, 3 * E};
    for (int k = 0; k < 5; ++k) { l.g[k] = {l.total, nx[k]}; l.total += n_chains * nx[k]; }
    return l;
}

// The hand-off regions: tagged words that the master, the workers and the peers leave for each other.  Set-up allocates
// each zeroed (`words`); a checkpoint load zeroes them again, all but the last `kept` words (diag[24], [25] are counters
// that survive a load).  The inbox exists once the exchange has been asked for (xchg_alloc, which sizes it).
enum { kRegSlots, kRegLoGran, kRegPgran, kRegDiag, kRegInbox, kRegions };
struct HandoffRegion { unsigned long long **p; size_t words, kept; };
inline std::array<HandoffRegion, kRegions> handoff_regions(htm_chains *hc)
{
    ChainsDev &d = hc->dev;
    return {{{&d.slots, (size_t)d.slot_rep * d.slot_stride, 0},
             {&d.lo_gran, (size_t)d.n_chains * 16, 0},
             {&d.pgran, (size_t)d.n_chains * 256 * d.pgran_stride, 0},      // (<= 256 workers whatever the launch shape)
             {&d.diag, 32, 8},
             {&hc->d_inbox, hc->inbox_bytes / sizeof(unsigned long long), 0}}};
}

inline void clear_host_records(htm_chains *hc)
{
    hc->lik_iter.clear(); hc->lik_chain.clear(); hc->lik_val.clear();
    hc->smp_iter.clear(); hc->smp_chain.clear(); hc->smp_data.clear();
}

// ---- the kernel table ---------------------------------------------------------------------------------------------
// Every instantiation of a chain-master kernel is written down once, as a row of the loop unit that compiles it
// (htm_loop_*.hip, through the row templates of htm_loop_rows.hpp): the kernel's address (attributes, occupancy), the block size it is launched with and its typed launch.
// htm_plan.hpp decides WHICH loop a launch takes (loop_for); launch_mcmc looks the instantiation up here; a combination that
// no unit builds gives nullptr, which the caller reports -- never another instantiation in its place.
struct LoopLaunch {
    dim3 grid, block;
    size_t smem;
    hipStream_t stream;
    const FwdDev *f;
    const ChainsDev *cs;
    int mode, target;
    const double *gathered;
    int ring_size, wmax;
    unsigned long long seq;      // the chain set's count of k_mcmc launches (k_step takes none)
};
struct LoopKernel { const void *fn; int threads; int (*launch)(const LoopLaunch &); };      // threads 0: the caller chooses (k_step)
// (nc, ring: the chain count and the ring size a sized instantiation holds as literals -- 0: any, read at run time)
struct LoopRow { bool step, wide; int nch; bool fp32; int mk; int nc, ring; LoopKernel k; };
struct LoopRows { const LoopRow *rows; size_t n; };

const LoopKernel *mcmc_kernel(int nch, bool fp32, int mk, bool wide);      // nullptr: not built
const LoopRow *sized_kernel(int nch, bool fp32, int mk, int nc, int ring);  // loop mk's row whose literals are these (0 in a row: any); nullptr: none
const LoopKernel *step_kernel(int nch, bool fp32, bool wide);

// one per loop unit, all searched by the two lookups above (htm_chains_run.hip)
LoopRows loop_rows_free();         // MK 3, 8: the free-running master of a single rank, generic, specialised and sized
LoopRows loop_rows_lock();         // MK 4, 7: the free-running master in lock-step, and with several master workgroups
LoopRows loop_rows_barrier();      // MK 0, 1, 2 and k_step: the loop with barriers
LoopRows loop_rows_wide();         // k_mcmc_wide, k_step_wide: the loop with barriers for up to kMaxWideChains chains
LoopRows loop_rows_pipe();         // MK 5, 6: the pipelined master

}  // namespace htm

#pragma GCC visibility pop
