// htm_plan.hpp -- a chain set's launch plan: which chain-master loop each mode runs and the shape it is launched with (worker
// blocks, LDS, stream ring, LDS mirror).  Plain structs and functions: no HIP runtime call, no handle, no device header, so
// every rule can be asked on a machine without a GPU (htm_chains_plan, include/htm_hip.h).  htm_chains_create runs
//     read_knobs -> plan_phase_a -> [allocations; the device facts] -> plan_phase_b
// and keeps the result (htm_chains::plan); launch_mcmc and htm_chains_master_stats ask loop_for (htm_chains_fixed_master reports
// what launch_mcmc was answered).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

namespace htm {

// (the values of Mode, htm_device.hpp, that launch a chain-master loop; htm_chains_setup.hip asserts that they agree)
constexpr int kPlanModeRun = 0, kPlanModeAdvance = 1, kPlanModeLockrun = 4;

// doubles in a rank's swap record: {the pair, its swap draw, the iteration | temperature and log-likelihood of every chain}
// (the device headers write the same length out: RW in htm_handoff.hpp)
constexpr size_t swap_words(int n_chains) { return 4 + 2 * (size_t)n_chains; }

// ---- the environment switches of htm_chains_create, read once ------------------------------------------------------------------
struct Knobs {
    int worker_cap = 250;          // HTM_WORKER_CAP (tuning).  Of 256 CUs: the master's, and a few to spare
    bool max_workers_set = false; int max_workers = 0;      // HTM_MAX_WORKERS: GPUs shared between ranks
    bool ranks_set = false; int ranks = 0;                  // HTM_RANKS_PER_GPU (htm_chains_share_gpu reads it again)
    // hand-off geometry (tuning knobs; defaults measured on MI355X); the first two are clamped against the job
    int slot_replicas = 1, slot_stride_bytes = 4096, pgran_stride_bytes = 16, npoll = 1;
    bool persist = true;           // HTM_PERSIST=0: k_step + k_full instead of k_mcmc
    int dbg = 0;                   // HTM_DEBUG_NO_DROP
    unsigned long long xwait_ticks = 0;      // HTM_XCHG_TIMEOUT_MS
    int xfail_iter = 0;            // HTM_DEBUG_XCHG_FAIL_ITER
    int xown = 1;                  // HTM_XOWN
    long long stream_cap = 1 << 20;          // HTM_STREAM_CAP: stream positions kept in HBM (~100 B each)
    bool prior_same = true;        // HTM_PRIOR_SAME=0 (diagnostics): every chain reads its own prior records
    bool mb = true;                // HTM_MB=0: one master workgroup
    bool ring_slack = true;        // HTM_RING_SLACK=0 keeps the old ring sizes of up to eight chains (A/B only)
    bool flow = true;              // HTM_FLOW=0 keeps the loop with barriers (step_body)
    bool fast = true;              // HTM_FAST=0 forces the free-running master's generic instantiation (A/B runs, tests)
    bool sized = true;             // HTM_SIZED=0: loop 8 never takes its sized instantiation (k_mcmc_sized; A/B runs, tests).  No part of the plan
    bool flow_lock = true;         // HTM_FLOW_LOCK=0
    bool pipe = false, pipe_lock = false;    // HTM_PIPE=1 / HTM_PIPE_LOCK=1 (opt-in)
};

// HTM_RANKS_PER_GPU: whether it is set and, if `k` is not NULL, its value.  Read at creation and again by htm_chains_share_gpu.
inline bool ranks_per_gpu_knob(int *k)
{
    const char *e = getenv("HTM_RANKS_PER_GPU");
    if (e && k) *k = atoi(e);
    return e != nullptr;
}

inline Knobs read_knobs()
{
    auto env_int = [](const char *name, int dflt, int lo, int hi) {
        const char *e = getenv(name);
        const int v = e ? atoi(e) : dflt;
        return std::max(lo, std::min(hi, v));
    };
    auto starts = [](const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; };
    Knobs k;
    if (getenv("HTM_WORKER_CAP")) k.worker_cap = env_int("HTM_WORKER_CAP", 250, 1, 255);
    if (const char *e = getenv("HTM_MAX_WORKERS")) { k.max_workers_set = true; k.max_workers = atoi(e); }
    k.ranks_set = ranks_per_gpu_knob(&k.ranks);
    k.slot_replicas = env_int("HTM_SLOT_REPLICAS", 1, 1, 1 << 30);
    k.slot_stride_bytes = env_int("HTM_SLOT_STRIDE", 4096, 0, 1 << 22);
    k.pgran_stride_bytes = env_int("HTM_PGRAN_STRIDE", 16, 16, 4096);
    k.npoll = env_int("HTM_NPOLL", 1, 1, 3);
    k.persist = !starts("HTM_PERSIST", '0');
    { const char *e = getenv("HTM_DEBUG_NO_DROP"); k.dbg = (e && atoi(e) != 0) ? 1 : 0; }
    { const char *e = getenv("HTM_XCHG_TIMEOUT_MS"); const double ms = e ? atof(e) : 20000.0; k.xwait_ticks = (unsigned long long)(std::max(1.0, ms) * 1.0e5); }
    { const char *e = getenv("HTM_DEBUG_XCHG_FAIL_ITER"); k.xfail_iter = e ? atoi(e) : 0; }
    k.xown = starts("HTM_XOWN", '0') ? 0 : 1;
    if (const char *e = getenv("HTM_STREAM_CAP")) {          // power of two >= 2^17 (tests: ring wrap-around in short runs)
        long long v = atoll(e), c2 = 1 << 17;
        while (c2 < v && c2 < (1ll << 24)) c2 <<= 1;
        k.stream_cap = c2;
    }
    k.prior_same = !starts("HTM_PRIOR_SAME", '0');
    k.mb = !starts("HTM_MB", '0');
    k.ring_slack = !starts("HTM_RING_SLACK", '0');
    k.flow = !starts("HTM_FLOW", '0');
    k.fast = !starts("HTM_FAST", '0');
    k.sized = !starts("HTM_SIZED", '0');
    k.flow_lock = !starts("HTM_FLOW_LOCK", '0');
    k.pipe = starts("HTM_PIPE", '1');
    k.pipe_lock = starts("HTM_PIPE_LOCK", '1');
    return k;
}

// ---- what is planned for ---------------------------------------------------------------------------------------------------------
struct PlanJob {
    int nc = 0, n_procs = 1, S = 0, E = 0, nch = 1;      // chains, ranks, stations, events, stations per lane
    bool fp32 = false, use_time = true, use_amp = true;
};

// what the rules need from the device headers (filled in by htm_chains_setup.hip, plan_sizes)
struct PlanSizes {
    size_t flow_shared = 0, wide_shared = 0, pipe_shared = 0;      // sizeof FlowShared, StepSharedT<kMaxWideChains>, PipeShared
    size_t pipe_ring_bytes = 0;                                    // pipe_ring_bytes(n_chains)
    int gath_stage = 0, hops = 0, pipe_threads_nch1 = 0;           // kGathStage, kHops, mcmc_threads<1, 5>()
    int max_chains = 0, gran_per_slot = 0, max_slot_replicas = 0;
};

// what htm_chains_create asks the device between the two phases (all 0 where it does not ask)
struct PlanDevice {
    int n_cu = 0;
    int blocks_per_cu = 0;              // the smallest occupancy of the candidate k_mcmc instantiations at (512 threads, step_smem)
    int pipe_blocks_per_cu[2] = {0, 0}; // of MK 5 and 6 at (pipe_threads, pipe_smem_want): only when a pipelined loop is asked for
};

// The part of the plan a launch reads: a member of htm_chains.
struct LoopPlan {
    bool persist = true;           // k_mcmc (master + resident full-evaluation workers) vs k_step + k_full
    bool flow = false;             // single-rank loop on the free-running master (htm_flow.hpp) instead of step_body
    bool flow_fixed = false;       // ... and the job's shape allows its specialised instantiation (k_mcmc<.., 8>; loop_for decides per launch)
    bool wide = false;             // more than kMaxChains chains: the loop with barriers at kMaxWideChains (k_mcmc_wide, k_step_wide)
    bool flow_lock = false;        // lock-step ranks (MODE_LOCKRUN) on the free-running master too
    int mb_blocks = 1;             // master workgroups of the single-rank loop (> 1: k_mcmc<.., 7>, eight chains each)
    bool pipe = false;             // single-rank loop on the pipelined master (htm_pipe.hpp)
    bool pipe_lock = false;        // lock-step ranks (MODE_LOCKRUN) on it too
    size_t pipe_smem = 0; int pipe_ring = 512;      // its LDS size and stream window
    int ring_size = 512, wmax = 64;
    size_t step_smem = 0;
    int worker_cap = 250;          // most worker blocks a launch takes (HTM_WORKER_CAP)
    long blocks_fit = 0;           // resident blocks of a k_mcmc launch on this device (htm_chains_share_gpu)
    int nw = 1;                    // chain waves of k_step (one more wave is the RNG producer)
};

struct Plan {
    LoopPlan loop;
    int n_workers = 1;             // worker blocks of a persistent launch
    int mirror_n = 0, mirror_steps = 0;      // the LDS mirror of (vs, t_corr, qs, a_corr) x all chains, and whether their step sizes are in it
    // hand-off geometry and stream capacity (ChainsDev / htm_chains)
    int slot_rep = 1, slot_stride = 512, pgran_stride = 2, npoll = 1;
    long long stream_cap = 0;
    // carried from phase A to phase B
    bool mb_want = false; int mb_need = 0;
    size_t mir = 0;
    bool pipe_asked = false;       // a pipelined loop is asked for and its LDS fits (htm_chains_create then asks for its occupancies)
    size_t pipe_smem_want = 0; int pipe_ring_want = 512, pipe_threads = 512;
    char refused[192] = "";        // not empty: the shape exceeds the LDS budget (HTM_EINVAL with this text)
};

constexpr size_t kLdsCap = 156 * 1024;

// Worker blocks of a persistent launch: as many as fit (one per CU next to the master's), at most one per `waves_per_block` events.
// A full evaluation takes as long as its busiest wave, which evaluates ceil(E / (waves per block x blocks)) events: at 10 000
// events and 8 waves per block 250 blocks give five rounds where 240 gave six (+8 % at 10 000 x 128 x 16 fp32, +6 % at 10 000 x 64 x 8).
// (Taking the SMALLEST block count that reaches the same number of rounds was measured too: -1 % -- the waves with a round less
// leave the memory system to the others sooner.)
inline int worker_blocks(int E, int waves_per_block, long cap)
{
    return (int)std::max<long>(1, std::min<long>(std::max<long>(1, cap), (E + waves_per_block - 1) / waves_per_block));
}

// Several ranks on one GPU (more masters instead of more rounds per master: 4 ranks x 8 chains run 2.7 M steps/s where one rank x
// 32 chains runs 1.7 M): every rank's blocks must be resident at once, so each takes its share of the CUs.  Blocks go to the 8
// XCDs of the GPU in turn, every launch starting with the first: a rank's blocks must be spread evenly over them (a multiple
// of 8) and the ranks' shares of one XCD's CUs must add up to no more than it has -- 5 ranks x 51 blocks are 255 of 256 CUs
// and still do not fit (7 blocks x 5 ranks on XCDs 0..2: the launches wait for each other's CUs forever).
inline long room_for_workers(long blocks_fit, int ranks_on_gpu)
{
    const long per_xcd = blocks_fit / 8;
    return per_xcd >= ranks_on_gpu ? 8 * (per_xcd / ranks_on_gpu) - 1 : blocks_fit / ranks_on_gpu - 1;
}

// ---- phase A: everything that needs no device fact -----------------------------------------------------------------------------
inline Plan plan_phase_a(const PlanJob &j, const Knobs &kn, const PlanSizes &sz)
{
    Plan p;
    LoopPlan &lp = p.loop;
    const int nc = j.nc;
    const bool nch12 = j.nch == 1 || j.nch == 2;
    lp.wide = nc > sz.max_chains;
    lp.persist = kn.persist;
    lp.worker_cap = kn.worker_cap;
    p.n_workers = worker_blocks(j.E, 8, kn.worker_cap);
    if (kn.max_workers_set) p.n_workers = std::max(1, std::min(p.n_workers, kn.max_workers));
    p.slot_rep = std::min(sz.max_slot_replicas, kn.slot_replicas);
    p.slot_stride = std::max(std::max(nc, sz.max_chains) * sz.gran_per_slot * 8, kn.slot_stride_bytes) / 8;     // bytes -> words
    p.pgran_stride = kn.pgran_stride_bytes / 8;
    p.npoll = kn.npoll;
    p.stream_cap = kn.stream_cap;

    lp.nw = std::min(nc, 8);
    // stream window: a chain step draws <= 6 numbers, select_pair/judge_swap a few more (cls_parallel.f90:226-230)
    lp.wmax = ((6 * nc + 16 + 63) / 64) * 64;
    // LDS of the master: the stream window -- two iterations + their swaps ahead where it fits (role P sends orders two
    // iterations ahead), else one -- and the mirror of (vs, t_corr, qs, a_corr) x all chains + their step sizes that
    // role P reads (without it no orders are sent ahead).  Per ring position: U, LOGU, pg, pr, plogr (5 doubles), dec,
    // sw (int4), hop (kHops ints).
    // (the wide kernels' LDS layout is step_body's at kMaxWideChains; every narrow loop shares FlowShared's)
    const size_t shared_bytes = lp.wide ? sz.wide_shared : sz.flow_shared;
    const size_t lds_fixed = ((shared_bytes + 15) & ~size_t(15)) + 3 * (size_t)j.S * sizeof(double) + sz.gath_stage * sizeof(double);
    const size_t lds_pos = 5 * sizeof(double) + 2 * 16 + sz.hops * sizeof(int);
    const size_t mir = p.mir = 2 * (size_t)nc + 2 * (size_t)nc * j.S;
    // (sized by what an iteration can really draw, 6 per chain step + the swap's, not by wmax's rounding to 64: at 16 chains
    // the two-iteration window then fits a 512-position ring instead of 1024 -- half the LDS, so the mirror fits too)
    const int wdraw = 6 * nc + 16;
    // Several master workgroups (9..16 chains, k_mcmc<.., 7>): a workgroup's window is kept by the wave of its FIRST chain, and
    // that chain can be two iterations ahead of a chain of its own workgroup that sat in a full evaluation (its turn asks the
    // later chains for their checks of the iteration before only).  The late chain then adopts an anchor that lies up to three
    // iterations behind the keeper's position: the ring must hold the look-ahead (3 wd + 24) AND three iterations + the spread of
    // eight chains behind it, or the anchor's table entries have been overwritten by positions one ring further on (the
    // mismatch of profiles/r04_z_mb_open_issue.txt: a base computed from evicted entries).  With two chains per wave -- one
    // workgroup -- the keeper cannot get further than one iteration ahead, and up to eight chains leave the ring mostly empty.
    p.mb_need = (3 * wdraw + 24) + (3 * wdraw + 16) + 6 * 8 + 16;
    p.mb_want = nc > 8 && nc <= 16 && j.n_procs == 1 && nch12 && kn.mb;
    // The same rule for the free-running loop of ONE workgroup with a wave per chain (up to eight chains; single rank and lock-step
    // ranks): the keeper's wave runs chain 0 only and gets as far ahead of a late chain.  (More than eight chains on one
    // workgroup: the keeper's wave has two chains and meets every other chain's check within an iteration.)  Rings of 256
    // positions -- 4 and 5 chains -- were too short for it by this count; HTM_RING_SLACK=0 keeps the old sizes (A/B only).
    const int fr_need = (nc <= 8 && kn.ring_slack) ? (3 * wdraw + 24) + (3 * wdraw + 16) : 0;
    auto ring_for = [&](int look) { int r = 256; while (r < look * wdraw + 64 || r < fr_need || (p.mb_want && r < p.mb_need)) r *= 2; return r; };
    for (int pass = 0; pass < 2; ++pass) {
        lp.ring_size = ring_for(2);
        // preference: long window + values + step sizes, long window + values, short window + both, short + values, nothing
        const int looks[4] = {4, 4, 2, 2}, steps[4] = {1, 0, 1, 0};
        for (int k = 0; k < 4; ++k)
            if (lds_fixed + (size_t)ring_for(looks[k]) * lds_pos + (1 + steps[k]) * mir * sizeof(double) <= kLdsCap) {
                lp.ring_size = ring_for(looks[k]); p.mirror_n = (int)mir; p.mirror_steps = steps[k];
                break;
            }
        if (p.mirror_n > 0 || !p.mb_want) break;
        p.mb_want = false;      // (the longer ring does not fit beside the mirror: one workgroup, the usual ring)
    }
    lp.step_smem = lds_fixed + (size_t)lp.ring_size * lds_pos + (1 + p.mirror_steps) * (size_t)p.mirror_n * sizeof(double);
    if (lp.step_smem > kLdsCap && lp.wide)
        snprintf(p.refused, sizeof(p.refused), "%d chains x %d stations: the loop with barriers needs %zu B of LDS, more than the %zu B budget",
                 nc, j.S, lp.step_smem, kLdsCap);
    else if (lp.step_smem > kLdsCap) snprintf(p.refused, sizeof(p.refused), "n_chains / n_sta too large for k_step's LDS budget");
    if (lp.step_smem < 1024) lp.step_smem = 1024;

    // The pipelined master (htm_pipe.hpp; HTM_PIPE=0 keeps the free-running one): front / evaluators / decider over an LDS ring
    // of iteration slots.  Needs the LDS mirror of the non-hypocentre parameters (what its evaluators read) and one or two
    // stations per lane.
    // (opt-in, HTM_PIPE=1 / HTM_PIPE_LOCK=1: on one CU it matches the free-running master -- 4.8 us per iteration at 1000 x 64 x 8,
    // +8 % at 16 chains, profiles/r04_pipe_*.txt -- and does not beat it; DESIGN.md 3.6 says what it is for)
    p.pipe_ring_want = 512;
    while (p.pipe_ring_want < 2 * wdraw + 160) p.pipe_ring_want *= 2;
    p.pipe_smem_want = ((sz.pipe_shared + 15) & ~size_t(15)) + (size_t)p.pipe_ring_want * lds_pos + (3 * (size_t)j.S + sz.gath_stage) * sizeof(double) +
                       mir * sizeof(double) + sz.pipe_ring_bytes;
    p.pipe_threads = j.nch == 1 ? sz.pipe_threads_nch1 : 512;
    const bool usable = !lp.wide && kn.dbg == 0 && nch12 && p.pipe_smem_want <= kLdsCap &&
                        p.mirror_n == (int)mir;      // (the mirror is part of every loop's LDS layout: one size for all)
    lp.pipe = usable && j.n_procs == 1 && kn.pipe;
    lp.pipe_lock = usable && kn.pipe_lock &&
                   (size_t)j.n_procs * swap_words(nc) <= (size_t)sz.gath_stage;      // (MODE_LOCKRUN: any number of ranks)
    p.pipe_asked = lp.persist && (lp.pipe || lp.pipe_lock);
    return p;
}

// ---- phase B: what the device can hold decides the rest -----------------------------------------------------------------------
// Its first part, from n_cu and blocks_per_cu alone: persist, blocks_fit and the worker count.  (htm_chains_create asks for the
// pipelined master's occupancies only where the persistent launch stands.)
inline void plan_residency(Plan &p, const PlanJob &j, const Knobs &kn, const PlanDevice &f)
{
    LoopPlan &lp = p.loop;
    if (!lp.persist) return;
    // Master and workers of a k_mcmc launch wait for each other, so every block must be RESIDENT: never ask for more
    // worker blocks than the device can hold next to the master (a partitioned or CU-masked GPU has fewer CUs; every
    // block carries the master's LDS size).  Workers take events round-robin, so fewer of them only take longer.
    lp.blocks_fit = (long)f.blocks_per_cu * f.n_cu;
    const long room = (kn.ranks_set && kn.ranks > 1) ? room_for_workers(lp.blocks_fit, kn.ranks) : lp.blocks_fit - 1;
    if (room < 1) lp.persist = false;      // not even one worker fits next to the master: two-kernel path
    else if (p.n_workers > room) p.n_workers = worker_blocks(j.E, 8, room);
}

inline Plan plan_phase_b(const Plan &a, const PlanJob &j, const Knobs &kn, const PlanDevice &f)
{
    Plan p = a;
    LoopPlan &lp = p.loop;
    const int nc = j.nc;
    const bool nch12 = j.nch == 1 || j.nch == 2;
    plan_residency(p, j, kn, f);
    // The free-running master (htm_flow.hpp) runs the single-rank loop when its stream window fits: three iterations of
    // look-ahead + one behind + the spread of chain 0's wave over its chains (flow_step's window extension), and the LDS
    // mirror the orders are computed from.  HTM_FLOW=0 keeps the loop with barriers (step_body); so do the hand-off tests'
    // debug switches.
    const int wd = 6 * nc + 16, c_max = 8 * ((nc - 1) / 8);
    // More than kMaxChains chains: the loop with barriers whatever HTM_FLOW / HTM_MB / HTM_PIPE say (wide).
    const bool window_ok = lp.persist && !lp.wide && kn.flow && kn.dbg == 0 && p.mirror_n > 0 && lp.ring_size >= 4 * wd + 32 + 2 * c_max + 16;
    lp.flow = window_ok && j.n_procs == 1;
    // Its instantiation specialised on what the job fixes (FlowFixed, htm_flow.hpp): one rank, up to eight chains (a wave per
    // chain: the shapes it is tested and measured at), full rows of 64 or 128 stations with both data types, the mirror with its
    // step sizes.  Chosen from what the library observes; HTM_FAST=0 only forces the generic instantiation (A/B runs, tests).
    // The step log can be switched on after this point: loop_for looks at it.
    lp.flow_fixed = lp.flow && kn.fast && nc <= 8 && nch12 && j.S == 64 * j.nch && j.use_time && j.use_amp &&
                    p.mirror_n == (int)p.mir && p.mirror_steps != 0;
    // More than eight chains on a rank: a master workgroup for every eight (k_mcmc<.., 7>, htm_flow.hpp MbShared) instead of
    // rounds on the same eight waves.  (HTM_MB=0: one workgroup.  The ring was sized for several in phase A: mb_want, mb_need.)
    // 9..16 chains: two workgroups.  More would need more of the stream window per step than the one wave of a workgroup that
    // keeps it can load -- 128 positions, an iteration of 16 chains takes ~90.
    if (lp.flow && p.mb_want && lp.ring_size >= p.mb_need && nc > 8 && nc <= 16 && nch12) {
        const int nb = (nc + 7) / 8;
        if (lp.blocks_fit - nb >= 1) {
            lp.mb_blocks = nb;
            const long room = lp.blocks_fit - nb;
            if (p.n_workers > room) p.n_workers = worker_blocks(j.E, 8, room);
        }
    }
    lp.flow_lock = window_ok && j.n_procs <= 60 && kn.flow_lock;      // (MODE_LOCKRUN: up to 60 ranks -- a lane per rank reads its stop word, flow_xload)
    // the pipelined master: phase A found it asked for and its LDS fitting
    lp.pipe = lp.pipe && lp.persist;
    lp.pipe_lock = lp.pipe_lock && lp.persist;
    if (lp.pipe || lp.pipe_lock) {
        lp.pipe_smem = p.pipe_smem_want; lp.pipe_ring = p.pipe_ring_want;
        if (p.pipe_threads == 768) {
            // (12-wave blocks: a worker block takes 12 events; every loop of this chain set then runs with this many blocks.
            // HTM_RANKS_PER_GPU used to bound this count by blocks_fit / k - 1; it now goes through room_for_workers like every
            // other share of the GPU.  That changes no result: plan_residency has already brought n_workers to or below
            // room_for_workers, which is never above blocks_fit / k - 1, and the count below is the smaller of the two.)
            int nw = worker_blocks(j.E, 12, lp.worker_cap);
            if (kn.max_workers_set) nw = std::max(1, std::min(nw, kn.max_workers));
            if (kn.ranks_set && kn.ranks > 1) nw = std::min<long>(nw, std::max<long>(1, room_for_workers(lp.blocks_fit, kn.ranks)));
            p.n_workers = std::min(p.n_workers, nw);
        }
        for (int lk = 5; lk <= 6; ++lk) {
            const long fit = (long)f.pipe_blocks_per_cu[lk - 5] * f.n_cu;
            lp.blocks_fit = std::min<long>(lp.blocks_fit, fit);
            if (fit - 1 < p.n_workers) { if (lk == 5) lp.pipe = false; else lp.pipe_lock = false; }      // (the launch shape was sized for the other loops: keep it)
        }
    }
    return p;
}

// ---- the ladder: the chain-master loop (MK, htm_mcmc.hpp k_mcmc) a launch in `mode` takes -------------------------------------
// 0 the single-rank loop with barriers, 1 one lock-step iteration per launch, 2 persistent lock-step, 3 / 4 the free-running
// master (single rank / lock-step), 5 / 6 the pipelined master, 7 several master workgroups, 8 the free-running master
// specialised on what the job fixes (one or two stations per lane; diagnostic runs with a step log take the generic 3).
inline int loop_for(const LoopPlan &lp, int mode, bool steplog_on)
{
    const bool run = mode == kPlanModeRun, lockrun = mode == kPlanModeLockrun;
    if (lp.wide) return run ? 0 : lockrun ? 2 : 1;
    if (run && lp.pipe) return 5;      // the pipelined master (htm_pipe.hpp): one or two stations per lane only
    if (lockrun && lp.pipe_lock) return 6;
    if (run && lp.flow && lp.mb_blocks > 1) return 7;
    if (run && lp.flow && lp.flow_fixed && !steplog_on) return 8;
    if (run && lp.flow) return 3;
    if (run) return 0;
    if (lockrun && lp.flow_lock) return 4;
    if (lockrun) return 2;
    return 1;
}

}  // namespace htm
