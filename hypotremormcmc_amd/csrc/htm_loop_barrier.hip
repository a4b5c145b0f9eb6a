// htm_loop_barrier.hip -- the chain master with barriers (step_body, htm_step.hpp): MK 0, 1, 2 of k_mcmc, and k_step of the two-kernel path.
// Nothing but this family's rows of the kernel table (htm_host.hpp): one line per instantiation, compiled here and nowhere else.
#include "htm_loop_rows.hpp"
#include "htm_step.hpp"

namespace htm {

template <int N, bool F> LoopRow step_row() { return step_row_of<k_step<N, F>>(false, N, F); }

LoopRows loop_rows_barrier()
{
    static const LoopRow rows[] = {
        mcmc_row<1, false, 0>(),
        mcmc_row<2, false, 0>(),
        mcmc_row<0, false, 0>(),
        mcmc_row<1, true, 0>(),
        mcmc_row<2, true, 0>(),
        mcmc_row<1, false, 1>(),
        mcmc_row<2, false, 1>(),
        mcmc_row<0, false, 1>(),
        mcmc_row<1, true, 1>(),
        mcmc_row<2, true, 1>(),
        mcmc_row<1, false, 2>(),
        mcmc_row<2, false, 2>(),
        mcmc_row<0, false, 2>(),
        mcmc_row<1, true, 2>(),
        mcmc_row<2, true, 2>(),
        step_row<1, false>(),
        step_row<2, false>(),
        step_row<0, false>(),
        step_row<1, true>(),
        step_row<2, true>(),
    };
    return {rows, sizeof(rows) / sizeof(rows[0])};
}

}  // namespace htm
