// htm_loop_wide.hip -- the chain master with barriers for 33..64 chains: k_mcmc_wide (MK 0, 1, 2) and k_step_wide.
// Nothing but this family's rows of the kernel table (htm_host.hpp): one line per instantiation, compiled here and nowhere else.
#include "htm_loop_rows.hpp"

namespace htm {

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
