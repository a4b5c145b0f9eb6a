// htm_loop_rows.hpp -- what a loop unit (htm_loop_*.hip) makes its rows of the kernel table (htm_host.hpp) from: a row names its
// instantiation once, and its address, its block size and its typed launch all come from that one mention.  k_mcmc comes with this
// header (htm_mcmc.hpp); the loop it runs is the unit's to include: htm_step.hpp, htm_flow.hpp or htm_pipe.hpp, one of them.
#pragma once
#include "htm_host.hpp"
#include "htm_mcmc.hpp"

#pragma GCC visibility push(hidden)

namespace htm {

// The typed launches.  KERNEL is named once, by the row templates below.
template <auto KERNEL>
int launch_mcmc_kernel(const LoopLaunch &l)
{
    hipLaunchKernelGGL(KERNEL, l.grid, l.block, l.smem, l.stream, *l.f, *l.cs, l.mode, l.target, l.gathered, l.ring_size, l.wmax, l.seq);
    return HTM_OK;
}
template <auto KERNEL>
int launch_step_kernel(const LoopLaunch &l)
{
    hipLaunchKernelGGL(KERNEL, l.grid, l.block, l.smem, l.stream, *l.f, *l.cs, l.mode, l.target, l.gathered, l.ring_size, l.wmax);
    return HTM_OK;
}
template <auto KERNEL>
LoopRow mcmc_row_of(bool wide, int nch, bool fp32, int mk, int threads)
{
    return LoopRow{false, wide, nch, fp32, mk, 0, 0, LoopKernel{reinterpret_cast<const void *>(KERNEL), threads, &launch_mcmc_kernel<KERNEL>}};
}
// (k_step takes 64 threads per chain wave, which the caller knows: threads = 0; and no launch count, LoopLaunch::seq.  k_step and
// k_step_wide are the barrier loop's own, htm_step.hpp: the two units that build it name them, step_row and step_wide_row there)
template <auto KERNEL>
LoopRow step_row_of(bool wide, int nch, bool fp32)
{
    return LoopRow{true, wide, nch, fp32, 0, 0, 0, LoopKernel{reinterpret_cast<const void *>(KERNEL), 0, &launch_step_kernel<KERNEL>}};
}
// (k_mcmc is launched with 512 threads; the pipelined master's instantiations with their launch bound, mcmc_threads)
template <int N, bool F, int K> LoopRow mcmc_row() { return mcmc_row_of<k_mcmc<N, F, K>>(false, N, F, K, (K == 5 || K == 6) ? mcmc_threads<N, K>() : 512); }
// (loop 8 with the chain count C and the ring R as literals: taken only for a launch with exactly these, htm_chains_run.hip sized_kernel)
template <int N, bool F, int C, int R> LoopRow sized_row()
{
    return LoopRow{false, false, N, F, 8, C, R, LoopKernel{reinterpret_cast<const void *>(k_mcmc_sized<N, F, C, R>), 512, &launch_mcmc_kernel<k_mcmc_sized<N, F, C, R>>}};
}
template <int N, bool F, int K> LoopRow wide_row() { return mcmc_row_of<k_mcmc_wide<N, F, K>>(true, N, F, K, 512); }

}  // namespace htm

#pragma GCC visibility pop
