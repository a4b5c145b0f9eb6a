// htm_loop_lock.hip -- the free-running chain master (htm_flow.hpp) as a lock-step rank, MK 4, and with several master workgroups, MK 7.
// Nothing but this family's rows of the kernel table (htm_host.hpp): one line per instantiation, compiled here and nowhere else.
#include "htm_loop_rows.hpp"
#include "htm_flow.hpp"

namespace htm {

LoopRows loop_rows_lock()
{
    static const LoopRow rows[] = {
        mcmc_row<1, false, 4>(),
        mcmc_row<2, false, 4>(),
        mcmc_row<0, false, 4>(),
        mcmc_row<1, true, 4>(),
        mcmc_row<2, true, 4>(),
        mcmc_row<1, false, 7>(),
        mcmc_row<2, false, 7>(),
        mcmc_row<1, true, 7>(),
        mcmc_row<2, true, 7>(),
    };
    return {rows, sizeof(rows) / sizeof(rows[0])};
}

}  // namespace htm
