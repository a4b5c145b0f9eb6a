// htm_loop_free.hip -- the free-running chain master of a single rank (htm_flow.hpp): MK 3, and MK 8 specialised on what the job fixes
// (and, for eight chains on a ring of 512 positions, on those two sizes: k_mcmc_sized).
// Nothing but this family's rows of the kernel table (htm_host.hpp): one line per instantiation, compiled here and nowhere else.
#include "htm_loop_rows.hpp"
#include "htm_flow.hpp"

namespace htm {

LoopRows loop_rows_free()
{
    static const LoopRow rows[] = {
        mcmc_row<1, false, 3>(),
        mcmc_row<2, false, 3>(),
        mcmc_row<0, false, 3>(),
        mcmc_row<1, true, 3>(),
        mcmc_row<2, true, 3>(),
        mcmc_row<1, false, 8>(),
        mcmc_row<2, false, 8>(),
        mcmc_row<1, true, 8>(),
        mcmc_row<2, true, 8>(),
        sized_row<1, false, 8, 512>(),
        sized_row<2, false, 8, 512>(),
        sized_row<1, true, 8, 512>(),
        sized_row<2, true, 8, 512>(),
    };
    return {rows, sizeof(rows) / sizeof(rows[0])};
}

}  // namespace htm
