// htm_loop_pipe.hip -- the pipelined chain master (htm_pipe.hpp): MK 5 for a single rank, MK 6 as a lock-step rank.
// Nothing but this family's rows of the kernel table (htm_host.hpp): one line per instantiation, compiled here and nowhere else.
#include "htm_loop_rows.hpp"
#include "htm_pipe.hpp"

namespace htm {

LoopRows loop_rows_pipe()
{
    static const LoopRow rows[] = {
        mcmc_row<1, false, 5>(),
        mcmc_row<2, false, 5>(),
        mcmc_row<1, true, 5>(),
        mcmc_row<2, true, 5>(),
        mcmc_row<1, false, 6>(),
        mcmc_row<2, false, 6>(),
        mcmc_row<1, true, 6>(),
        mcmc_row<2, true, 6>(),
    };
    return {rows, sizeof(rows) / sizeof(rows[0])};
}

}  // namespace htm
