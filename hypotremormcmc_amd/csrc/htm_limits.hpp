// htm_limits.hpp -- the two limits that the host side plans its launches and workspaces under: the work-items of one launch and
// an HTM_x_MB switch of the environment.  Plain C++: nothing of HIP, so that a plan which includes it (htm_locate_plan.hpp) can
// be compiled and checked by itself.  htm_steps_host.hpp brings it to the units that allocate.
#pragma once
#include <cstdlib>

#include "htm_hip.h"

#pragma GCC visibility push(hidden)

namespace htm {

// (htm_host.hpp's declaration, repeated for the headers that stand without it: sets htm_last_error()'s string, returns `code`)
int fail(int code, const char *fmt, ...);

// the dispatch packet holds a launch's grid in work-items as a uint32_t (hsa_kernel_dispatch_packet_t::grid_size_x)
constexpr long kMaxWorkItems = 0xffffffffL;

// HTM_x_MB: a positive number of MiB, `dflt` when the switch is not set
inline int env_mib(const char *name, double dflt, double *mb)
{
    *mb = dflt;
    if (const char *e = getenv(name)) {
        *mb = atof(e);
        if (!(*mb > 0.0)) return fail(HTM_EINVAL, "%s = %s: a positive number of MiB", name, e);
    }
    return HTM_OK;
}

}  // namespace htm

#pragma GCC visibility pop
