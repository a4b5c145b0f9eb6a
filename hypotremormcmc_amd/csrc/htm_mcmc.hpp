// htm_mcmc.hpp -- k_mcmc, k_mcmc_sized, k_mcmc_wide: the kernel of every persistent launch of the main loop -- the chain master's workgroup(s) in
// front, the full-evaluation workers (htm_worker.hpp) behind them.  MK names the master's loop.  No loop is defined or included
// here: the three bodies are only declared, and a unit defines the one it instantiates by including that loop's header
// (htm_step.hpp, htm_flow.hpp or htm_pipe.hpp) next to this one (htm_loop_*.hip).
#pragma once
#include "htm_handoff.hpp"
#include "htm_worker.hpp"

namespace htm {

// the loops (their default template arguments stay with their definitions: k_mcmc names every argument)
struct FlowGeneric; struct FlowFixed;
template <int NC, int RING> struct FlowSized;
template <int NCH, bool PERSIST, bool F32, int MK, int CAP>
__device__ __forceinline__ void step_body(FwRef f_, CsRef cs_, int mode, int target_arg, const double *gathered, int ring_size, int wmax, unsigned long long launch);
template <int NCH, bool F32, bool LOCK, bool MB, class TR>
__device__ __forceinline__ bool flow_body(FwRef f_, CsRef cs_, int target_arg, int ring_size, int wmax, unsigned long long launch);
template <int NCH, bool F32, bool LOCK>
__device__ __forceinline__ void pipe_body(FwRef f_, CsRef cs_, int target_arg, int ring_size, int wmax, unsigned long long launch);

// One launch = the chain master (block 0) + W full-evaluation workers (blocks 1..W), all resident.
// `launch` = the host's count of k_mcmc launches of this chain set (1, 2, ...): orders and the quit word carry it, so
// nothing a previous launch left in memory can be mistaken for this launch's.
// Blocks of 8 waves; the pipelined master with one station per lane takes 12 (three per SIMD, 168 registers a wave): nine
// evaluators instead of five -- its throughput is the evaluators' (and the worker blocks take 12 events each).
#ifndef HTM_PIPE_THREADS
#define HTM_PIPE_THREADS 512
#endif
template <int NCH, int MK> constexpr int mcmc_threads() { return (MK >= 5 && MK <= 7 && NCH == 1) ? HTM_PIPE_THREADS : 512; }
template <int NCH, bool F32 = false, int MK = 0>
__global__ __launch_bounds__((mcmc_threads<NCH, MK>())) void k_mcmc(FwdDev f, ChainsDev cs, int mode, int target_arg,
                                               const double *gathered, int ring_size, int wmax,
                                               unsigned long long launch)
{
    const KArgLayout __attribute__((address_space(4))) &ka = *(const KArgLayout __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    // MK 7: several master workgroups (blocks 0 .. n_mb - 1, eight chains each: flow_body<.., MB>); the workers follow them
    const int n_mb = MK == 7 ? (ka.cs.n_chains + 7) / 8 : 1;
    if ((int)blockIdx.x < n_mb) {
        // MK 0: the single-rank loop with barriers (step_body, htm_step.hpp); 1: one lock-step iteration per launch; 2: a lock-step rank, swap records exchanged inside the launch (MODE_LOCKRUN)
        // 3: the single-rank loop on the free-running master (flow_body, htm_flow.hpp); 4: a lock-step rank (MODE_LOCKRUN) on it; 7: above
        // 8: MK 3 for a job whose shape the host has found fixed (flow_body<.., FlowFixed>: htm_flow.hpp, htm_plan.hpp loop_for)
        // 5: the pipelined master (pipe_body, htm_pipe.hpp), single rank; 6: a lock-step rank (MODE_LOCKRUN) on it
        if constexpr (MK == 3) flow_body<NCH, F32, false, false, FlowGeneric>(ka.f, ka.cs, target_arg, ring_size, wmax, launch);
        else if constexpr (MK == 8) flow_body<NCH, F32, false, false, FlowFixed>(ka.f, ka.cs, target_arg, ring_size, wmax, launch);
        else if constexpr (MK == 4) flow_body<NCH, F32, true, false, FlowGeneric>(ka.f, ka.cs, target_arg, ring_size, wmax, launch);
        else if constexpr (MK == 5) pipe_body<NCH, F32, false>(ka.f, ka.cs, target_arg, ring_size, wmax, launch);
        else if constexpr (MK == 6) pipe_body<NCH, F32, true>(ka.f, ka.cs, target_arg, ring_size, wmax, launch);
        else if constexpr (MK == 7) { if (!flow_body<NCH, F32, false, true, FlowGeneric>(ka.f, ka.cs, target_arg, ring_size, wmax, launch)) return; }      // (only the workgroup that finishes last goes on)
        else step_body<NCH, true, F32, MK, kMaxChains>(ka.f, ka.cs, mode, target_arg, gathered, ring_size, wmax, launch);
        // every exit of the master comes through here (its returns are uniform over the block): release the workers
        __syncthreads();
        if (threadIdx.x == 0) st_agent(&ka.cs.ps->quit, launch + 1ull);
    } else {
        worker_body<NCH, F32, mcmc_threads<NCH, MK>() / 64, (MK == 5 || MK == 6)>(ka.f, ka.cs, launch, (int)blockIdx.x - n_mb);
    }
}

// k_mcmc<.., 8> with the chain count and the stream window's ring as literals too (htm_flow.hpp FlowSized): the same arguments,
// the same 512 threads, the same workers.  launch_mcmc takes it for a launch of loop 8 whose run-time values are exactly these
// (the kernel table's rows carry them: LoopRow::nc, ::ring); the master checks them once more before it touches anything.
template <int NCH, bool F32, int NC, int RING>
__global__ __launch_bounds__(512) void k_mcmc_sized(FwdDev f, ChainsDev cs, int mode, int target_arg,
                                                     const double *gathered, int ring_size, int wmax,
                                                     unsigned long long launch)
{
    const KArgLayout __attribute__((address_space(4))) &ka = *(const KArgLayout __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    if (blockIdx.x == 0) {
        flow_body<NCH, F32, false, false, FlowSized<NC, RING>>(ka.f, ka.cs, target_arg, ring_size, wmax, launch);
        __syncthreads();
        if (threadIdx.x == 0) st_agent(&ka.cs.ps->quit, launch + 1ull);
    } else {
        worker_body<NCH, F32, 8, false>(ka.f, ka.cs, launch, (int)blockIdx.x - 1);
    }
}

// k_mcmc for 33..64 chains: the loop with barriers only (MK 0 single rank, 1 one lock-step iteration per launch, 2 persistent
// lock-step), its StepShared and the workers' order polls sized for kMaxWideChains.  The free-running, several-workgroup and
// pipelined masters keep kMaxChains: their stream windows do not fit the LDS above ~35 chains.
template <int NCH, bool F32, int MK>
__global__ __launch_bounds__(512) void k_mcmc_wide(FwdDev f, ChainsDev cs, int mode, int target_arg,
                                                    const double *gathered, int ring_size, int wmax,
                                                    unsigned long long launch)
{
    static_assert(MK >= 0 && MK <= 2, "the wide kernels run the loop with barriers only");
    const KArgLayout __attribute__((address_space(4))) &ka = *(const KArgLayout __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    if (blockIdx.x == 0) {
        step_body<NCH, true, F32, MK, kMaxWideChains>(ka.f, ka.cs, mode, target_arg, gathered, ring_size, wmax, launch);
        __syncthreads();
        if (threadIdx.x == 0) st_agent(&ka.cs.ps->quit, launch + 1ull);
    } else {
        worker_body<NCH, F32, 8, false, kMaxWideChains>(ka.f, ka.cs, launch, (int)blockIdx.x - 1);
    }
}

}  // namespace htm
