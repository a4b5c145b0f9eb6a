// htm_loop_wide.hip -- the chain master with barriers for 33..64 chains: k_mcmc_wide (MK 0, 1, 2; htm_mcmc.hpp) and k_step_wide (htm_step.hpp).
// Nothing but this family's rows of the kernel table (htm_host.hpp): one line per instantiation, compiled here and nowhere else.
#include "htm_loop_rows.hpp"
#include "htm_step.hpp"

namespace htm {

template <int N, bool F> LoopRow step_wide_row() { return step_row_of<k_step_wide<N, F>>(true, N, F); }

LoopRows loop_rows_wide()
{
    static const LoopRow rows[] = {
        wide_row<1, false, 0>(),
        wide_row<2, false, 0>(),
        wide_row<0, false, 0>(),
        wide_row<1, true, 0>(),
        wide_row<2, true, 0>(),
        wide_row<1, false, 1>(),
        wide_row<2, false, 1>(),
        wide_row<0, false, 1>(),
        wide_row<1, true, 1>(),
        wide_row<2, true, 1>(),
        wide_row<1, false, 2>(),
        wide_row<2, false, 2>(),
        wide_row<0, false, 2>(),
        wide_row<1, true, 2>(),
        wide_row<2, true, 2>(),
        step_wide_row<1, false>(),
        step_wide_row<2, false>(),
        step_wide_row<0, false>(),
        step_wide_row<1, true>(),
        step_wide_row<2, true>(),
    };
    return {rows, sizeof(rows) / sizeof(rows[0])};
}

}  // namespace htm
