// htm_grid.hpp -- the map grid of the analysis programs, stated once: the box that htm_hypo_density bins samples on
// (htm_density.hpp) and that htm_forward_locate tabulates posteriors on (htm_locate.hpp).  For host and device code; no call
// into the HIP runtime, and nothing of HIP included: a plain C++ compiler reads it too (htm_locate_plan.hpp).  The caller's form is
// grid9 = {x0, dx, nx, y0, dy, ny, z0, dz, nz} in doubles (include/htm_hip.h).
#pragma once
#include <cmath>

#include "htm_limits.hpp"      // fail

#ifdef __HIPCC__
#define HTM_GRID_FN __host__ __device__ __forceinline__
#else
#define HTM_GRID_FN inline
#endif

#pragma GCC visibility push(hidden)

namespace htm {

constexpr int kMapMaxCells = 4096;      // cells per axis

// (The initialisers are for the layout of LocGrid, htm_locate.hpp: without them MapGrid is a POD to the C++ ABI, a POD base's
// tail padding stays free, and LocGrid's own members would move from byte 60 of its kernels' argument to byte 64.)
struct MapGrid {
    double x0 = 0.0, dx = 0.0, y0 = 0.0, dy = 0.0, z0 = 0.0, dz = 0.0;
    int nx = 0, ny = 0, nz = 0;
};

// the centre of cell i: one multiplication, then one addition (the library is built with -ffp-contract=off)
HTM_GRID_FN double map_centre(double v0, double dv, int i)
{
    const double t = ((double)i + 0.5) * dv;
    return v0 + t;
}

// what every entry point asks of grid9 before any device call, and the grid itself
inline int map_grid_parse(const double *grid9, MapGrid *g)
{
    int n[3];
    for (int a = 0; a < 3; ++a) {
        const double v0 = grid9[3 * a], dv = grid9[3 * a + 1], cnt = grid9[3 * a + 2];
        if (!std::isfinite(v0) || !std::isfinite(dv) || !(dv > 0.0))
            return fail(HTM_EINVAL, "grid axis %c: origin %g, cell size %g: need a finite origin and a finite cell size > 0", "xyz"[a], v0, dv);
        if (!(cnt >= 1.0 && cnt <= (double)kMapMaxCells) || cnt != std::floor(cnt))
            return fail(HTM_EINVAL, "grid axis %c: %g cells: need an integer in 1..%d", "xyz"[a], cnt, kMapMaxCells);
        n[a] = (int)cnt;
    }
    *g = MapGrid{grid9[0], grid9[1], grid9[3], grid9[4], grid9[6], grid9[7], n[0], n[1], n[2]};
    return HTM_OK;
}

}  // namespace htm

#pragma GCC visibility pop
