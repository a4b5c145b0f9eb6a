// htm_density.hpp -- stacked density maps of recorded hypocentre samples: every sample of every window is binned on a map
// grid (htm_grid.hpp) and counted once in the xy, xz and yz maps (and the volume, where asked for) of its window's layer (rule
// and measurements: DESIGN.md §3.9).  The counts are integers: exact, and the same whatever the order of the adds.
//
// Layout: hypo is [n_mod][ld] row-major, one recorded model per row, window w in columns 3w, 3w+1, 3w+2 (the record of
// hypo.RR.out); layer [n_win] or NULL (every window in layer 0); xy [n_layer][ny][nx], xz [n_layer][nz][nx],
// yz [n_layer][nz][ny], vol [n_layer][nz][ny][nx] or NULL, tally [n_layer][2] = inside, outside.
//
// Both kernels: a wave owns 64 consecutive windows and rows of a slab, which it loads as the ellipsoid kernels do (ell_fetch:
// three coalesced 512-B segments per row, through the wave's LDS tile to lane <-> window).  k_dens_plain: grid = (window
// groups / kDensWG, row slabs), the waves of a workgroup on neighbouring window groups; k_dens_lds: grid = (window groups, row
// slabs), the waves of a workgroup on the same 64 windows and every kDensWG-th piece of kDensU rows, so that a workgroup
// meets as few layers as can be.  A lane keeps, per map, the cell of its last sample and how often it came in a row (a converged chain
// repeats a cell many times) and adds the run when the cell changes.
//
//   k_dens_plain   any grid: the runs go to the maps by 64-bit global atomics.  NAIVE: one global atomic per sample and map,
//                  the yardstick of tools/bench_density.py (HTM_DENSITY_NAIVE=1)
//   k_dens_lds     the three 2-D maps of ONE layer as 32-bit counters in the workgroup's LDS (kDensLdsCells of them); the
//                  runs go there by LDS atomics, and the workgroup adds every counter that is not 0 to the global map once
//                  per layer that its windows belong to (one pass over the slab per such layer: layers made of
//                  neighbouring windows, as time bins are, cost one pass).  The volume does not fit and goes the plain way.
//
// LDS budget: tiles kDensWG x kDensU x 192 doubles = 24 KiB, counters 32 KiB, 56 KiB of a workgroup's static 64 KiB: two
// workgroups (eight waves) per CU within gfx950's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "htm_ellipsoid.hpp"
#include "htm_grid.hpp"

namespace htm {

constexpr int kDensWG = 4;                      // window groups (waves) per workgroup
constexpr int kDensU = 4;                       // rows in flight per thread
constexpr int kDensLdsCells = 8192;             // nx ny + nx nz + ny nz of a grid the LDS path takes
constexpr long kDensMaxSlabRows = 1L << 22;     // rows a workgroup counts between two flushes of its LDS counters
// every lane of a workgroup can put every row of its slab into one 32-bit counter
static_assert(64L * kDensWG * kDensMaxSlabRows <= 0xffffffffL, "a workgroup's 32-bit counter could wrap");

struct DensOut {
    unsigned long long *xy, *xz, *yz, *vol, *tally;
};

// q = (v - v0) / dv, a true division; inside iff 0 <= q < n (NaN and +-inf are outside), then the cell is floor(q)
__device__ __forceinline__ bool dens_bin(double v, double v0, double dv, int n, int *cell)
{
    const double q = (v - v0) / dv;
    const bool in = q >= 0.0 && q < (double)n;
    *cell = in ? (int)floor(q) : 0;
    return in;
}

// a run of equal cells of one lane in one map
struct DensRun {
    int key = -1;
    unsigned n = 0;
};
template <class T>
__device__ __forceinline__ void dens_run_flush(DensRun &r, T *map)
{
    if (r.n) atomicAdd(map + r.key, (T)r.n);
    r.n = 0;
}
template <class T>
__device__ __forceinline__ void dens_run_add(DensRun &r, int key, T *map)
{
    if (key != r.key) {
        dens_run_flush(r, map);
        r.key = key;
    }
    ++r.n;
}

// adds the lanes' (n_in, n_out) to tally [n_layer][2]: one pair of atomics per layer that the wave's lanes belong to
__device__ __forceinline__ void dens_tally(int lane, int L, unsigned n_in, unsigned n_out, unsigned long long *tally)
{
    unsigned long long rem = __ballot(L >= 0);
    while (rem) {
        const int src = __ffsll((long long)rem) - 1;
        const int Ls = __shfl(L, src);
        const bool m = L == Ls;
        unsigned a = m ? n_in : 0u, b = m ? n_out : 0u;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            a += __shfl_xor(a, off);
            b += __shfl_xor(b, off);
        }
        if (lane == src) {
            atomicAdd(tally + 2 * Ls, (unsigned long long)a);
            atomicAdd(tally + 2 * Ls + 1, (unsigned long long)b);
        }
        rem &= ~__ballot(m);
    }
}

// the layer of lane's window, -1 for a window that takes no part
__device__ __forceinline__ int dens_layer(const int *layer, long w, long n_win, int n_layer)
{
    if (w >= n_win) return -1;
    const int L = layer ? layer[w] : 0;
    return L >= 0 && L < n_layer ? L : -1;
}

template <bool NAIVE>
__global__ __launch_bounds__(64 * kDensWG) void k_dens_plain(const double *hypo, long ld, long n_mod, long n_win, long slab_rows,
                                                             const int *layer, int n_layer, MapGrid g, DensOut o)
{
    __shared__ double tiles[kDensWG][kDensU * 192];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long grp = (long)blockIdx.x * kDensWG + wv, w = grp * 64 + lane;
    if (grp * 64 >= n_win) return;
    const int L = dens_layer(layer, w, n_win, n_layer);
    if (!__ballot(L >= 0)) return;
    const long c0 = grp * 192;
    const int n_live = (int)min(192L, 3 * n_win - c0);
    const int lxy = L * g.ny * g.nx, lxz = L * g.nz * g.nx, lyz = L * g.nz * g.ny, lvol = o.vol ? L * g.nz * g.ny * g.nx : 0;
    DensRun rxy, rxz, ryz, rvol;
    unsigned n_in = 0, n_out = 0;
    auto count = [&](const double (&x)[3]) {
        if (L < 0) return;
        int ix, iy, iz;
        const bool inx = dens_bin(x[0], g.x0, g.dx, g.nx, &ix), iny = dens_bin(x[1], g.y0, g.dy, g.ny, &iy), inz = dens_bin(x[2], g.z0, g.dz, g.nz, &iz);
        const bool in = inx && iny && inz;
        if (!in) {
            ++n_out;
            return;
        }
        ++n_in;
        const int kxy = lxy + iy * g.nx + ix, kxz = lxz + iz * g.nx + ix, kyz = lyz + iz * g.ny + iy;
        const int kvol = o.vol ? lvol + (iz * g.ny + iy) * g.nx + ix : 0;
        if (NAIVE) {
            atomicAdd(o.xy + kxy, 1ull);
            atomicAdd(o.xz + kxz, 1ull);
            atomicAdd(o.yz + kyz, 1ull);
            if (o.vol) atomicAdd(o.vol + kvol, 1ull);
        } else {
            dens_run_add(rxy, kxy, o.xy);
            dens_run_add(rxz, kxz, o.xz);
            dens_run_add(ryz, kyz, o.yz);
            if (o.vol) dens_run_add(rvol, kvol, o.vol);
        }
    };
    const long row0 = (long)blockIdx.y * slab_rows, row1 = min(n_mod, row0 + slab_rows);
    double *tile = tiles[wv];
    long r = row0;
    for (; r + kDensU <= row1; r += kDensU) {
        double v[kDensU][3];
        ell_fetch<kDensU>(hypo + c0, ld, r, lane, n_live, tile, v);
#pragma unroll
        for (int u = 0; u < kDensU; ++u) count(v[u]);
    }
    for (; r < row1; ++r) {
        double v[1][3];
        ell_fetch<1>(hypo + c0, ld, r, lane, n_live, tile, v);
        count(v[0]);
    }
    if (!NAIVE) {
        dens_run_flush(rxy, o.xy);
        dens_run_flush(rxz, o.xz);
        dens_run_flush(ryz, o.yz);
        if (o.vol) dens_run_flush(rvol, o.vol);
    }
    dens_tally(lane, L, n_in, n_out, o.tally);
}

// needs nx ny + nx nz + ny nz <= kDensLdsCells and slab_rows <= kDensMaxSlabRows
__global__ __launch_bounds__(64 * kDensWG) void k_dens_lds(const double *hypo, long ld, long n_mod, long n_win, long slab_rows,
                                                           const int *layer, int n_layer, MapGrid g, DensOut o)
{
    __shared__ double tiles[kDensWG][kDensU * 192];
    __shared__ unsigned maps[kDensLdsCells];
    __shared__ int s_next;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long grp = blockIdx.x, w = grp * 64 + lane;
    const int L = dens_layer(layer, w, n_win, n_layer);
    const long c0 = grp * 192;
    const int n_live = (int)min(192L, 3 * n_win - c0);
    const int nxy = g.ny * g.nx, nxz = g.nz * g.nx, nyz = g.nz * g.ny, cells = nxy + nxz + nyz;
    const long nvol = (long)nxy * g.nz;
    unsigned *mxy = maps, *mxz = maps + nxy, *myz = maps + nxy + nxz;
    const long row0 = (long)blockIdx.y * slab_rows, row1 = min(n_mod, row0 + slab_rows);
    double *tile = tiles[wv];
    unsigned n_in = 0, n_out = 0;
    // the layers of the workgroup's windows in ascending order, one pass over the slab for each
    for (int cur = -1;;) {
        if (threadIdx.x == 0) s_next = INT_MAX;
        __syncthreads();
        if (L > cur) atomicMin(&s_next, L);
        __syncthreads();
        cur = s_next;
        if (cur == INT_MAX) break;
        for (int i = threadIdx.x; i < cells; i += 64 * kDensWG) maps[i] = 0u;
        __syncthreads();
        const bool mine = L == cur;
        if (__ballot(mine)) {
            DensRun rxy, rxz, ryz, rvol;
            unsigned long long *vol = o.vol ? o.vol + cur * nvol : nullptr;
            auto count = [&](const double (&x)[3]) {
                if (!mine) return;
                int ix, iy, iz;
                const bool inx = dens_bin(x[0], g.x0, g.dx, g.nx, &ix), iny = dens_bin(x[1], g.y0, g.dy, g.ny, &iy), inz = dens_bin(x[2], g.z0, g.dz, g.nz, &iz);
        const bool in = inx && iny && inz;
                if (!in) {
                    ++n_out;
                    return;
                }
                ++n_in;
                dens_run_add(rxy, iy * g.nx + ix, mxy);
                dens_run_add(rxz, iz * g.nx + ix, mxz);
                dens_run_add(ryz, iz * g.ny + iy, myz);
                if (vol) dens_run_add(rvol, (iz * g.ny + iy) * g.nx + ix, vol);
            };
            const long n_full = (row1 - row0) / kDensU;              // whole pieces of kDensU rows: wave wv takes every kDensWG-th
            for (long c = wv; c < n_full; c += kDensWG) {
                double v[kDensU][3];
                ell_fetch<kDensU>(hypo + c0, ld, row0 + c * kDensU, lane, n_live, tile, v);
#pragma unroll
                for (int u = 0; u < kDensU; ++u) count(v[u]);
            }
            for (long r = row0 + n_full * kDensU; wv == 0 && r < row1; ++r) {
                double v[1][3];
                ell_fetch<1>(hypo + c0, ld, r, lane, n_live, tile, v);
                count(v[0]);
            }
            dens_run_flush(rxy, mxy);
            dens_run_flush(rxz, mxz);
            dens_run_flush(ryz, myz);
            if (vol) dens_run_flush(rvol, vol);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += 64 * kDensWG) {
            const unsigned c = maps[i];
            if (!c) continue;
            unsigned long long *dst = i < nxy ? o.xy + (long)cur * nxy + i
                                      : i < nxy + nxz ? o.xz + (long)cur * nxz + (i - nxy)
                                                      : o.yz + (long)cur * nyz + (i - nxy - nxz);
            atomicAdd(dst, (unsigned long long)c);
        }
        __syncthreads();
    }
    dens_tally(lane, L, n_in, n_out, o.tally);
}

}  // namespace htm
