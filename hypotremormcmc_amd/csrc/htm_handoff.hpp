// htm_handoff.hpp -- what more than one chain-master loop, or a loop and the full-evaluation workers, use; no loop is defined here.
//
//   kernel arguments   CsRef / FwRef / SdRef + rebase: read through the kernarg segment where they are used; KArgLayout
//   LDS                StepSharedT (the state every loop keeps, FlowShared and PipeShared extend it), Ring (the window of the
//                      stream rings) and its fill: pf_load / pf_store / prefetch_all
//   parameter vector   group_offsets / elem_offset, opaque_zero + ld_state (mutable state wants VECTOR loads), rl_f64
//   hand-off           the agent- and system-scope loads and stores, the tagged granules of the orders and of the workers' partial
//                      sums (st_gran, gran_f64), drain_vmem, void_slot
//   a step's pieces    wave_incl_scan, metropolis, hop_ahead
//   lock-step ranks    apply_swap, exchange_post / exchange_finish: the swap records exchanged inside the launch
// The loops: htm_step.hpp (with barriers), htm_flow.hpp (free-running), htm_pipe.hpp (pipelined).  The workers: htm_worker.hpp.
// The kernel of them all: htm_mcmc.hpp.
#pragma once
#include "htm_device.hpp"
#include "htm_stream.hpp"

#ifndef HTM_ALLOW2
#define HTM_ALLOW2 1     // diagnostics: 0 = role P sends orders one iteration ahead only
#endif

namespace htm {

// Kernel arguments are read where they are used, through references into the kernarg segment (constant address space:
// scalar loads), re-based at the entry of every phase by an opaque move -- so the ~190 dwords of FwdDev + ChainsDev are
// never all alive at once.  (Taken by value they are loaded at kernel entry, hoisted out of the iteration loop and
// carried through it in spilled lanes: ~800 v_readlane reloads in the master's loop.)
typedef const ChainsDev __attribute__((address_space(4))) &CsRef;
typedef const FwdDev __attribute__((address_space(4))) &FwRef;
typedef const StreamDev __attribute__((address_space(4))) &SdRef;
template <class T>
__device__ __forceinline__ const T __attribute__((address_space(4))) &rebase(const T __attribute__((address_space(4))) &r)
{
    const T __attribute__((address_space(4))) *p = &r;
    asm volatile("" : "+s"(p));
    return *p;
}
struct KArgLayout { FwdDev f; ChainsDev cs; };

constexpr int kGathStage = 512;   // doubles of LDS for the gathered swap records (else they are read in place)

template <int CAP>
struct StepSharedT {
    static constexpr int kCap = CAP;
    Proposal prop[CAP];
    double temp[CAP], L[CAP];
    double rtemp[CAP];     // 1 / temperature (the Metropolis ratio multiplies by it), renewed wherever temp is written
    int start[CAP];        // stream position (relative) at which each chain step started
    int start_fix[CAP];    // corrected starts for a repeat pass (written by wave 0)
    int cnt[CAP];          // draws the step consumed (judge draw included iff prior_ok)
    int slot_l[CAP], slot_s[CAP];
    int redone[CAP];       // the chain repeated its step in this iteration (undo + new commit: role P stays out)
    // role P (k_mcmc): [iteration & 1][chain]: the chain's step of that iteration, starting at position pre_p, already
    // has its order out under pre_tag; pre_mode 1: sent one iteration ahead, 2: two iterations ahead (evaluated on
    // the state before the step in between; see chain_pass)
    int pre_p[2][CAP];
    unsigned pre_tag[2][CAP];
    int pre_mode[2][CAP];
    int pre_pa[2][CAP];   // two-ahead orders: where the step in between was expected to start
    int np[CAP * 7], na[CAP * 7];   // proposal / acceptance counters of this launch
    int sw_do, sw_c1, sw_c2;      // swap decided between the barriers; applied by the waves owning the chains
    double sw_T1, sw_T2;          // new temperatures of chains sw_c1 / sw_c2
    long long origin;             // absolute stream position of relative position 0 (= spos at launch)
    long long hop_end;            // StreamDev::hop_end when this launch started
    int avail;                    // the produced stream covers relative positions < avail
    int fill;                     // the LDS ring holds relative positions < fill
    int base;                     // relative position at which the current iteration starts
    int redo;                     // >= 0: chains >= redo repeat their pass; -1: validated; -2: aborted
    int catchup;                  // written between the barriers: the LDS window must be extended first
    int rolep_iter;               // role P has finished for this iteration (see step_body)
    double xrec[4 + 2 * CAP];   // MODE_LOCKRUN: this rank's swap record of the iteration (what goes to every rank's inbox)
    int xdone;                    // MODE_LOCKRUN: the swap of every iteration <= xdone has been applied (see exchange_finish)
    int xstop, xspec;             // decided by role V: this rank asks for a stop; the next iteration starts before the swap is known
    unsigned xctl;                // the control word this rank posted with its latest record (exchange_post; read back by exchange_finish)
    int xctl_iter;                // ... and the iteration it belongs to
    Ctrl c;
#ifdef HTM_STAMPS
    unsigned long long stamp_acc[96];   // diagnostic cycle accounting of this launch, flushed to ChainsDev::stamps at its end
#endif
};
// the narrow loops (htm_flow.hpp, htm_pipe.hpp and step_body up to kMaxChains); step_body at kMaxWideChains: the wide kernels
using StepShared = StepSharedT<kMaxChains>;

struct Ring {                     // LDS window of the stream rings, index = relative position & mask
    double *U, *LOGU, *pg, *pr, *plogr;
    int4 *dec, *sw;
    int *hop;
    int mask;
    // k_mcmc only: LDS mirror of the non-hypocentre part of the rank's parameter vector (vs, t_corr, qs, a_corr
    // of every chain; same offsets as ChainsDev::xall) and of its step sizes, kept current by the commits, so
    // that role P needs no memory round trip.  mir_n = 0: no mirror (too large, or not the persistent kernel)
    double *mx, *mstep;
    int mir_n;
    bool mir_steps;
    int lock;                     // htm_flow.hpp: 1 = a lock-step rank (select_pair is rank 0's, judge_swap's draw the pair's first rank's)
};

// one stream position in flight from the global rings to the LDS window
typedef int i32x4 __attribute__((ext_vector_type(4)));      // (a plain vector: HIP's int4 class keeps temporaries in private memory)
struct PfRegs {
    double U, LOGU, pg, pr, plogr;
    i32x4 dec, sw, h0, h1;
    int p;                        // relative position, -1: nothing to store
};

template <int CAP>
__device__ __forceinline__ void pf_load(PfRegs &r, CsRef cs_, const StepSharedT<CAP> &sh, int p, int limit)
{
    CsRef cs = rebase(cs_);
    r.p = -1;
    if (p < limit) {
        SdRef sd = cs.stream;
        const long long g = (sh.origin + p) & sd.mask;
        r.U = sd.U[g]; r.LOGU = sd.LOGU[g]; r.pg = sd.pg[g]; r.pr = sd.pr[g]; r.plogr = sd.plogr[g];
        r.dec = reinterpret_cast<const i32x4 *>(sd.dec)[g]; r.sw = reinterpret_cast<const i32x4 *>(sd.sw)[g];
        const i32x4 *hs = reinterpret_cast<const i32x4 *>(sd.hop + g * kHops);
        r.h0 = hs[0]; r.h1 = hs[1];
        r.p = p;
    }
}

__device__ __forceinline__ void pf_store(const PfRegs &r, const Ring &rg)
{
    if (r.p >= 0) {
        const int l = r.p & rg.mask;
        rg.U[l] = r.U; rg.LOGU[l] = r.LOGU; rg.pg[l] = r.pg; rg.pr[l] = r.pr; rg.plogr[l] = r.plogr;
        reinterpret_cast<i32x4 *>(rg.dec)[l] = r.dec; reinterpret_cast<i32x4 *>(rg.sw)[l] = r.sw;
        i32x4 *hd = reinterpret_cast<i32x4 *>(rg.hop + l * kHops);
        hd[0] = r.h0; hd[1] = r.h1;
    }
}

// every thread of the workgroup: extend the LDS window to cover relative positions < target
// (kernel start; later only if a long select_pair redraw run ate the look-ahead)
template <int CAP>
__device__ __forceinline__ void prefetch_all(CsRef cs_, StepSharedT<CAP> &sh, const Ring &rg, int target)
{
    CsRef cs = rebase(cs_);
    if (target > sh.avail) target = sh.avail;
    if (target > sh.base + rg.mask + 1 - 8) target = sh.base + rg.mask + 1 - 8;
    const int fl = sh.fill;
    for (int p = fl + (int)threadIdx.x; p < target; p += (int)blockDim.x) {
        PfRegs r;
        pf_load(r, cs, sh, p, target);
        pf_store(r, rg);
    }
    __syncthreads();
    if (threadIdx.x == 0 && target > sh.fill) sh.fill = target;
    __syncthreads();
}

// The rank's parameter vector is ONE allocation per field, groups in proposal-type order [vs | t_corr | qs | a_corr | hypo],
// each [n_chains][nx] (ChainsDev::xall and friends): every element is base + integer offset -- scalar arithmetic on one
// pointer instead of a choice between the five ModelDev windows (fewer kernel arguments alive in the loop).
struct GroupOff { int tc, qs, ac, hy, nh; };
__device__ __forceinline__ GroupOff group_offsets(CsRef cs_)
{
    CsRef cs = rebase(cs_);
    const int nc = cs.n_chains, S = cs.S;
    GroupOff g;
    g.tc = nc; g.qs = nc + nc * S; g.ac = 2 * nc + nc * S; g.hy = 2 * nc + 2 * nc * S; g.nh = 3 * cs.E;
    return g;
}
// element idx of chain c's model of proposal type `type` (1 vs, 2 t_corr, 3 qs, 4 a_corr, 5..7 hypo)
__device__ __forceinline__ int elem_offset(CsRef cs_, int type, int c, int idx)
{
    CsRef cs = rebase(cs_);
    const GroupOff g = group_offsets(cs);
    const int goff = type == 1 ? 0 : type == 2 ? g.tc : type == 3 ? g.qs : type == 4 ? g.ac : g.hy;
    const int gnx = (type == 1 || type == 3) ? 1 : (type == 2 || type == 4) ? cs.S : g.nh;
    return goff + c * gnx + idx;
}

// inclusive prefix sum over the 64 lanes (DPP row_shr scan + row_bcast, ints)
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return v;
}

// Chain state (x vectors, temperatures, log-likelihoods) is rewritten by this kernel while it loops over
// iterations.  hipcc turns uniform-address loads into scalar (K$) loads, and the scalar cache is not
// coherent with vector stores, so mutable state must be read with VECTOR loads.  `volatile` would do that but
// also makes the backend wait for every single load (s_waitcnt vmcnt(0) after each), serialising ~700-cycle
// latencies; instead the address gets a per-lane zero the compiler cannot see through, which keeps the loads
// ordinary (L1-cached, freely overlapped) vector loads.
__device__ __forceinline__ int opaque_zero()
{
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return z;
}
__device__ __forceinline__ double ld_state(const double *p, int vz) { return p[vz]; }

// lane l of a double, as a wave-uniform value
__device__ __forceinline__ double rl_f64(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// agent-scope relaxed accesses: sc1 write-through stores / L1-bypassing loads (MI355X_MICROARCH.md,
// inter-workgroup visibility).  Used for everything another workgroup of the same launch reads or writes.
__device__ __forceinline__ void st_agent(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_agent(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_gran(unsigned long long *g, unsigned tag, unsigned payload)
{
    st_agent(g, ((unsigned long long)tag << 32) | payload);
}
__device__ __forceinline__ void st_gran_f64(unsigned long long *g, unsigned tag, double v)   // two granules
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    st_gran(g, tag, (unsigned)(b >> 32));
    st_gran(g + 1, tag, (unsigned)b);
}
__device__ __forceinline__ double gran_f64(unsigned long long hi, unsigned long long lo)
{
    return __longlong_as_double((long long)(((hi & 0xffffffffull) << 32) | (lo & 0xffffffffull)));
}
__device__ __forceinline__ void drain_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// system-scope relaxed accesses: what another GPU (or another process on this one) writes into / reads from this
// rank's memory over xGMI while the kernel runs (swap-record inboxes, fine-grained allocations)
__device__ __forceinline__ void st_sys(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ unsigned long long ld_sys(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// The master takes back whatever order chain c's slot holds (k_mcmc): granule 0 loses its tag, so the slot is no longer
// a complete order -- a worker that has not looked yet never takes it, a worker waiting for the order's named commit
// sees the slot change and drops it.  This is how a void order is SIGNALLED (the chain repeated a pass, or the order
// was written for a stream position the step does not start at); nothing on the hand-off path is decided by a clock.
__device__ __forceinline__ void void_slot(CsRef cs_, int c)
{
    CsRef cs = rebase(cs_);
    for (int r = 0; r < cs.slot_rep; ++r) st_gran(cs.slots + (size_t)r * cs.slot_stride + c * kGranPerSlot, 0u, 0u);
}

__device__ __forceinline__ bool metropolis(double L_new, double L_cur, double T, double lpr, double r,
                                           double logr)
{
    double ratio = (L_new - L_cur) * T;     // cls_mcmc.f90:194-195; T = 1 / temperature here (formed once per swap, not per step)
    ratio = ratio + lpr;
    return r >= kEps && logr <= ratio;      // :198-199
}

// start of the chain step n steps after the one that starts at pos (hop tables cover kHops steps at a time)
__device__ __forceinline__ int hop_ahead(const Ring &rg, int pos, int n)
{
    int p = pos;
    while (n > kHops) { p += rg.hop[(p & rg.mask) * kHops + kHops - 1]; n -= kHops; }
    if (n > 0) p += rg.hop[(p & rg.mask) * kHops + n - 1];
    return p;
}

// thread 0: temperature swap between chains of any two ranks from the all-gathered records
// (cls_parallel.f90:118-213, :285-302).  Every rank evaluates the same decision from the same records.
template <int CAP>
__device__ __forceinline__ void apply_swap(CsRef cs_, StepSharedT<CAP> &sh, const double *gathered)
{
    CsRef cs = rebase(cs_);
    const int nc = cs.n_chains, RW = 4 + 2 * nc;
    const int iter = sh.c.iter_done + 1;
    if (cs.n_procs * nc > 1) {
        for (int r = 0; r < cs.n_procs; ++r)
            if ((int)gathered[(size_t)r * RW + 3] != iter) sh.c.err = -6;
        const int i1 = (int)gathered[0], i2 = (int)gathered[1];
        const int rank1 = i1 / nc, chain1 = i1 % nc, rank2 = i2 / nc, chain2 = i2 % nc;
        const double T1 = gathered[(size_t)rank1 * RW + 4 + 2 * chain1];
        const double L1 = gathered[(size_t)rank1 * RW + 5 + 2 * chain1];
        const double T2 = gathered[(size_t)rank2 * RW + 4 + 2 * chain2];
        const double L2 = gathered[(size_t)rank2 * RW + 5 + 2 * chain2];
        const double r = gathered[(size_t)rank1 * RW + 2];
        const double del_s = (L2 - L1) * (1.0 / T1 - 1.0 / T2);
        bool acc = false;
        if (r >= kEps) { if (log(r) <= del_s) acc = true; }
        if (acc) {
            if (cs.rank == rank1) { cs.temp[chain1] = T2; sh.temp[chain1] = T2; sh.rtemp[chain1] = 1.0 / T2; }
            if (cs.rank == rank2) { cs.temp[chain2] = T1; sh.temp[chain2] = T1; sh.rtemp[chain2] = 1.0 / T1; }
        }
        if (cs.rank == rank1) sh.c.spos += 1;       // judge_swap's rand_u() came from rank1's stream
    }
    sh.c.iter_done = iter;
    sh.c.stage = ST_IDLE;
}

// MODE_LOCKRUN, wave 0, after the roles of iteration `iter`: this rank's swap record goes into EVERY rank's inbox
// (its own included) as tagged 8-byte granules {iteration : 32, payload : 32} written with system-scope stores -- over
// xGMI into the peers' memory, no collective, no kernel boundary --, then the wave polls its own inbox until all
// n_procs records of this iteration are complete, stages them in LDS as the doubles apply_swap reads, and lane 0
// decides the swap exactly as every other rank does (cls_parallel.f90:118-213).  Record = the (4 + 2 n_chains) words
// of the all-gather protocol + one control word: bit 0 = this rank asks everybody to stop after this iteration
// (record buffers or produced random stream nearly used up: the host drains / refills and launches again), bit 1 = it
// has failed.  Inbox parity = iter & 1: a rank can be at most one iteration ahead of the slowest one.
constexpr int kXLoads = 8;        // granule loads per lane in flight while polling

// one wave: this rank's record of iteration `iter` into every rank's inbox
template <int CAP>
__device__ __forceinline__ void exchange_post(CsRef cs_, StepSharedT<CAP> &sh, int iter, int lane, bool want_stop)
{
    CsRef cs = rebase(cs_);
    const int nc = cs.n_chains, RW = 4 + 2 * nc, G = cs.xg, np = cs.n_procs, par = iter & 1;
    const unsigned tag = (unsigned)iter;
    const unsigned ctl = (want_stop ? 1u : 0u) | (sh.c.err ? 2u : 0u);
    if (lane == 0) { sh.xctl = ctl; sh.xctl_iter = iter; }      // (this rank's own record is taken from LDS when the records are collected)
    if (__builtin_expect(cs.dbg_xfail_iter > 0 && iter >= cs.dbg_xfail_iter, 0)) return;      // (fault injection: the peers never see this record)
    for (int g0 = 0; g0 < G; g0 += 64) {
        const int g = g0 + lane;
        if (g < G) {
            const int w = g >> 1;
            unsigned pay;
            if (w < RW) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(sh.xrec[w]);
                pay = (g & 1) ? (unsigned)b : (unsigned)(b >> 32);
            } else pay = (g & 1) ? 0u : ctl;
            const unsigned long long v = ((unsigned long long)tag << 32) | pay;
            for (int q = 0; q < np; ++q) st_sys(ld_const(cs.outbox + q) + (size_t)(par * np + cs.rank) * G + g, v);
        }
    }
}

// the same wave, later: wait for the n_procs records of iteration `iter`, decide the swap, publish sh.xdone = iter.
// Rows of 64 granules, row = (rank r, chunk k of its record); kXLoads rows in flight.
template <int CAP>
__device__ __forceinline__ void exchange_finish(CsRef cs_, StepSharedT<CAP> &sh, double *s_gath, int iter, int lane, bool publish = true)
{
    CsRef cs = rebase(cs_);
    const int nc = cs.n_chains, RW = 4 + 2 * nc, G = cs.xg, np = cs.n_procs, par = iter & 1;
    const unsigned tag = (unsigned)iter;
    const unsigned long long *in = cs.inbox + (size_t)par * np * G;
    unsigned *gu = reinterpret_cast<unsigned *>(s_gath);
    const int chunks = (G + 63) >> 6, rows = np * chunks;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();       // 100 MHz
    unsigned anyctl = 0;
    bool dead = false;
    // This rank's own record does not travel: it is read from LDS where exchange_post took it from (sh.xrec, sh.xctl) -- the round
    // trip of the rank's own stores through fine-grained memory was on the path of every lock-step iteration (HTM_XOWN=0 restores it).
    const bool own_lds = cs.xown != 0 && sh.xctl_iter == iter;
    for (int row0 = 0; row0 < rows && !dead; row0 += kXLoads) {
        unsigned long long v[kXLoads];
        for (;;) {
            bool ok = true;
#pragma unroll
            for (int j = 0; j < kXLoads; ++j) {
                const int row = row0 + j, r = row / chunks, k = (row - r * chunks) * 64 + lane;
                v[j] = (unsigned long long)tag << 32;
                if (row < rows && k < G) {
                    if (own_lds && r == cs.rank) {
                        const int w = k >> 1;
                        unsigned pay;
                        if (w < RW) {
                            const unsigned long long b = (unsigned long long)__double_as_longlong(sh.xrec[w]);
                            pay = (k & 1) ? (unsigned)b : (unsigned)(b >> 32);
                        } else pay = (k & 1) ? 0u : sh.xctl;
                        v[j] = ((unsigned long long)tag << 32) | pay;
                    } else v[j] = ld_sys(in + (size_t)r * G + k);
                }
            }
#pragma unroll
            for (int j = 0; j < kXLoads; ++j) ok = ok && (unsigned)(v[j] >> 32) == tag;
            if (__all(ok)) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > cs.xwait_ticks) {       // 20 s: a peer is gone
                if (lane == 0) sh.c.err = -10;
                dead = true;
                break;
            }
        }
        if (dead) break;
#pragma unroll
        for (int j = 0; j < kXLoads; ++j) {
            const int row = row0 + j, r = row / chunks, k = (row - r * chunks) * 64 + lane;
            if (row < rows && k < G) {
                const int w = k >> 1;
                if (w < RW) gu[2 * (r * RW + w) + ((k & 1) ? 0 : 1)] = (unsigned)v[j];      // little-endian halves of the double
                else if (!(k & 1)) anyctl |= (unsigned)v[j];
            }
        }
    }
    const bool stop_any = __ballot((anyctl & 1u) != 0) != 0ull, err_any = __ballot((anyctl & 2u) != 0) != 0ull;
    if (lane == 0) {
        if (!dead && sh.c.err == 0 && sh.c.stage == ST_WAIT_SWAP) {
            apply_swap(cs, sh, s_gath);                         // iteration done; rank1 consumed its judge_swap draw
            sh.base = (int)(sh.c.spos - sh.origin);
        }
        if (stop_any && sh.c.stop == 0) sh.c.stop = 3;          // everybody leaves after this iteration
        if (err_any && sh.c.err == 0) sh.c.err = -11;           // a peer reported a failure
        if (publish) __hip_atomic_store(&sh.xdone, iter, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

}  // namespace htm
