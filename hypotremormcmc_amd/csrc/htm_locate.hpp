// htm_locate.hpp -- every window's location posterior on a grid under a FIXED structure (vs, qs, station corrections): the
// kernels of htm_forward_locate (htm_locate.hip; rule, choices and measurements: DESIGN.md §3.10).  With the global parameters
// fixed the log-likelihood is a sum of independent per-event terms (each event is demeaned on its own: cls_forward.f90:113-133,
// :199-218, :268-303), so an event's term is a function of its position alone and is tabulated at the cell centres (htm_grid.hpp).
//
// The mapping is the opposite of event_misfit's: a lane owns CELLS, the stations are the serial inner loop in the reference's
// own order 0 .. n_sta - 1, and no sum over stations crosses lanes.
//
//   k_locate_pack     one record per (event of the batch, station): what the evaluation reads of a station, packed so that a
//                     workgroup reads it with uniform SCALAR loads (ld_const), and one record of constants per event
//   k_locate<MODE>    grid = (tiles, events of the batch).  A tile is up to kLocRows whole x-rows of ONE z-layer, at most
//                     kLocTile cells; a thread owns the cells t, t + 256, ... of it, kLocChunk at a time (independent
//                     dependency chains).  The demeaned misfit comes in one pass from the shifted identity (loc_distance,
//                     loc_residuals, LocSums: the station rule of every kernel that evaluates a cell, stated once).
//                     The lanes keep their cells' log posteriors in registers, the workgroup finds the tile's maximum and
//                     its first cell, puts the weights exp(lp - max) in LDS and sums them there in a fixed order: per x-row
//                     (a wave per row, the fixed-tree wave sum) and per ix over the rows.  One partial record per tile.
//   k_locate_combine  one workgroup per event: the event's maximum over its tiles in tile order, every partial rescaled by
//                     exp(max_tile - max_event); marginals, mean, covariance, log evidence.
//   k_locate_pack_draws, k_locate_marginal<MODE>    htm_forward_locate_marginal: the structure marginalised over draws of it,
//                     described where they stand, below k_locate; what follows a cell's log posterior is shared with k_locate
//                     (loc_cell_done, loc_tile_reduce), and k_locate_combine serves both.
//   k_locate_draw_evidence<MODE>, k_locate_draw_combine    htm_forward_locate_draw_evidence: every draw's log evidence per event
//                     and what the draws weigh, described where they stand, below k_locate_marginal
//   k_locate_stack, k_locate_stack_project    htm_forward_locate_stack: the windows' posteriors, one unit of mass each, summed per
//                     layer from the batch's volume, and the three projections; described where they stand, below k_locate_combine
//   k_locate_res_best, k_locate_residuals<MODE>, k_locate_res_combine    htm_forward_locate_residuals: every station's residual, the
//                     offsets that the demeaning takes away and chi2, at the best cell and as means over the window's posterior,
//                     from the batch's volume; described where they stand, at the end.  They share k_locate's station rule
//                     (loc_station_res) and the sums' offset and chi2 (LocSums<1>); the reductions are their own
// No floating-point atomics anywhere: the bits do not depend on timing.  The volume of log posteriors is written only when it
// is asked for, stacked, or read by the residual pass.
//
// A BOX PER EVENT (htm_forward_locate_boxes): k_locate, k_locate_marginal and k_locate_combine evaluate event b of
// the batch on the launch's grid with the origin org[b] in the place of the grid's (loc_grid_of, called at their top; a null
// `org` is the one grid for all).  Cell sizes, counts, tiles, the partial records and every reduction order stay the launch's:
// nothing after "which grid is this event on" changes, so an event's bits are those of a launch on its own grid.  The other
// kernels take no boxes.
//
// Every one of the three evaluation kernels exists twice: F32 = false, all arithmetic fp64, and F32 = true, the single-precision
// forward of htm_forward_locate_set_precision (the rule: loc_station).  The float copies of the structure are
// made ONCE, where the records are packed: the station's corrections in LocSta's last slot (k_locate_pack), 1 / vs and
// pi f / (qs vs) in LocJob (the host), the draws' table as pairs of floats in the place of the pairs of doubles
// (k_locate_pack_draws<float>).  The kernels convert nothing that is uniform.
//
// Partial record of a tile (doubles): [0] the tile's maximum lp (-inf: no included cell; k_locate_combine overwrites it with
// the tile's scale), [1] its first cell's linear index (-1: none), [2] that cell's log-likelihood term, [3] the tile's weight
// sum, then mx[nx] (weight per ix over the tile's rows), S[rows_per_tile] (weight per row), T[rows_per_tile] (weight times x
// per row).
#pragma once
#include <climits>
#include <type_traits>

#include "htm_device.hpp"
#include "htm_locate_plan.hpp"      // the tile's constants, LocSta, LocEv, LocPairT, LocGrid: shared with the host's plan, defined there

namespace htm {

// (the kernels' argument, as this compiler lays it out)
static_assert(sizeof(LocGrid) == 72, "rows, tpl and stride follow nz directly, in MapGrid's tail padding (htm_grid.hpp)");

constexpr int kLocChunk = 4;            // cells of a thread evaluated side by side
static_assert(kLocPerThread % kLocChunk == 0, "whole chunks");
// k_locate_marginal: cells of a thread side by side (the choice and its alternatives: DESIGN.md 3.11)
#ifndef HTM_LOCM_CELLS
#define HTM_LOCM_CELLS 1
#endif
constexpr int kLocmCells = HTM_LOCM_CELLS;
static_assert(kLocmCells >= 1 && kLocPerThread % kLocmCells == 0, "whole chunks");
// the same two choices for the F32 instantiations, whose register budget is another (measured: DESIGN.md 3.13)
#ifndef HTM_LOC_CHUNK32
#define HTM_LOC_CHUNK32 4
#endif
#ifndef HTM_LOCM_CELLS32
#define HTM_LOCM_CELLS32 HTM_LOCM_CELLS
#endif
constexpr int kLocChunk32 = HTM_LOC_CHUNK32;
constexpr int kLocmCells32 = HTM_LOCM_CELLS32;
static_assert(kLocChunk32 >= 1 && kLocPerThread % kLocChunk32 == 0 && kLocmCells32 >= 1 && kLocPerThread % kLocmCells32 == 0, "whole chunks");

struct LocJob {
    const LocSta *sta;      // [nb][S]
    const LocEv *ev;        // [nb]
    const double *prior;    // [nb][nx + ny + nz] log prior per ix, iy, iz, or nullptr: flat
    double *part;           // [nb][nz * tpl][stride]
    double *vol;            // [nb][nz][ny][nx] or nullptr
    const double *org;      // [nb][4] every event's box origin x0, y0, z0 and one unused, or nullptr: the grid's (loc_grid_of)
    int S;
    double rbeta, katt;     // 1 / vs, pi f / (qs vs)
    float rbeta32, katt32;  // the same, rounded to float
};

// a record at a wave-uniform address through the constant address space: scalar loads, as ld_const (the doubles travel in pairs)
typedef double loc_f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ LocSta loc_ld_sta(const LocSta *p)
{
    typedef const loc_f64x2 __attribute__((address_space(4))) *CP;
    const CP q = (CP)(unsigned long long)p;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef const double __attribute__((address_space(4))) *CD;
    typedef const f32x2 __attribute__((address_space(4))) *CF;
    const loc_f64x2 a = q[0], b = q[1], c = q[2], d = q[3];
    // (the last pair is a double and two floats, loaded as what they are: with the floats bit-cast out of a fifth pair's second
    // double, the compiler narrowed the load to the FIRST double's low word -- offset 0x40, not 0x48, in the assembly)
    const double apr = ((CD)q)[8];
    const f32x2 c32 = ((CF)q)[9];
    return LocSta{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1], apr, c32[0], c32[1]};
}
__device__ __forceinline__ LocEv loc_ld_ev(const LocEv *p)
{
    typedef const loc_f64x2 __attribute__((address_space(4))) *CP;
    const CP q = (CP)(unsigned long long)p;
    const loc_f64x2 a = q[0], b = q[1];
    return LocEv{a[0], a[1], b[0], b[1]};
}

// The grid of event b of the batch: the launch's, with the event's own origin where the call has a box per event (org [nb][4] =
// x0, y0, z0 and one unused; nullptr: the launch's grid as it is).  b is block-uniform, so the two pairs come through scalar
// loads, as loc_ld_ev's.  The host's copy writes the array before the launch and no kernel does.
__device__ __forceinline__ LocGrid loc_grid_of(const LocGrid &g, const double *org, int b)
{
    LocGrid ge = g;
    if (org) {      // (uniform)
        typedef const loc_f64x2 __attribute__((address_space(4))) *CP;
        const CP q = (CP)(unsigned long long)(org + 4 * (size_t)b);
        const loc_f64x2 xy = q[0], z = q[1];
        ge.x0 = xy[0]; ge.y0 = xy[1]; ge.z0 = z[0];
    }
    return ge;
}

__device__ __forceinline__ bool loc_included(double lp) { return lp == lp && lp != -__builtin_inf(); }

__global__ __launch_bounds__(256) void k_locate_pack(FwdDev f, int e0, int nb, const double *tc, const double *ac, const double *lct,
                                                     const double *lca, LocSta *sta, LocEv *ev)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)nb * f.S) return;
    const int b = (int)(i / f.S), j = (int)(i - (long)b * f.S);
    const size_t k = (size_t)(e0 + b) * f.S + j;
    LocSta r;
    r.sx = f.sx[j]; r.sy = f.sy[j]; r.sz = f.sz[j]; r.tc = tc[j]; r.ac = ac[j];
    r.tob = f.t_obs[k]; r.tpr = f.t_prec[k]; r.aob = f.a_obs[k]; r.apr = f.a_prec[k];
    r.tc32 = (float)r.tc; r.ac32 = (float)r.ac;
    sta[i] = r;
    if (j == 0) ev[b] = LocEv{f.rpsum_t[e0 + b], f.rpsum_a[e0 + b], lct[e0 + b], lca[e0 + b]};
}

// (value, index) of the larger value, of the lower index among equal values: the same whatever the order of the comparisons
struct LocBest {
    double lp, ell;
    int idx;
};
__device__ __forceinline__ void loc_better(LocBest &a, double lp, double ell, int idx)
{
    const bool take = lp > a.lp || (lp == a.lp && idx < a.idx);
    a.lp = take ? lp : a.lp; a.ell = take ? ell : a.ell; a.idx = take ? idx : a.idx;
}
__device__ __forceinline__ void loc_best_wave(LocBest &a)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) loc_better(a, __shfl_xor(a.lp, off), __shfl_xor(a.ell, off), __shfl_xor(a.idx, off));
}

// the four waves' values, `stride` apart in LDS, in a fixed order: (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double loc_sum4(const double *s, int stride = 1) { return (s[0] + s[stride]) + (s[2 * stride] + s[3 * stride]); }

// sum over the block's 256 threads in a fixed order: the wave sums' tree, then loc_sum4; every thread gets it
__device__ __forceinline__ double loc_block_sum(double v, double *s_red4)
{
    const double w = wave_sum1(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red4[threadIdx.x >> 6] = w;
    __syncthreads();
    return loc_sum4(s_red4);
}

// what a workgroup knows of its tile and event
struct LocTile {
    int tile, b, iz, iy0, rows, ncell;
    long cell0;             // linear index of the tile's first cell
    double zc, pz;
    const double *prior;    // the event's tables, or nullptr
};
__device__ __forceinline__ LocTile loc_tile(const LocGrid &g, const LocJob &jb)
{
    LocTile tl;
    tl.tile = blockIdx.x; tl.b = blockIdx.y;
    tl.iz = tl.tile / g.tpl; tl.iy0 = (tl.tile - tl.iz * g.tpl) * g.rows;
    tl.rows = min(g.rows, g.ny - tl.iy0); tl.ncell = tl.rows * g.nx;
    tl.cell0 = ((long)tl.iz * g.ny + tl.iy0) * g.nx;
    tl.zc = map_centre(g.z0, g.dz, tl.iz);
    tl.prior = jb.prior ? jb.prior + (size_t)tl.b * (g.nx + g.ny + g.nz) : nullptr;
    tl.pz = tl.prior ? tl.prior[g.nx + g.ny + tl.iz] : 0.0;
    return tl;
}

// Cell c of the tile has the log-likelihood term ell and the log prior pxy + pz: its log posterior, NaN for a thread without
// that cell; written to the volume if that is asked for, and offered to the thread's best cell (its cells come in ascending order)
__device__ __forceinline__ double loc_cell_done(const LocGrid &g, const LocJob &jb, const LocTile &tl, int c, double ell, double pxy, LocBest &best)
{
    const double v = tl.prior ? ell + (pxy + tl.pz) : ell;
    const bool live = c < tl.ncell;
    if (live) {
        if (jb.vol) jb.vol[(size_t)tl.b * ((size_t)g.nx * g.ny * g.nz) + (size_t)(tl.cell0 + c)] = v;
        if (loc_included(v)) loc_better(best, v, ell, c);
    }
    return live ? v : __builtin_nan("");
}

// Everything after the cells' log posteriors, for k_locate and k_locate_marginal alike: the tile's maximum and its first cell,
// the weights exp(lp - max) in LDS (s_w [kLocTile]), the row sums, the tile's partial record.  lp_of(k) is the log posterior of
// the thread's k-th cell t + 256 k; it may read s_w[t + 256 k] itself, which only this thread overwrites, after reading it.
template <class LpOf>
__device__ __forceinline__ void loc_tile_reduce(const LocGrid &g, const LocJob &jb, const LocTile &tl, LocBest best, double *s_w, LpOf lp_of)
{
    __shared__ double s_S[kLocRows];
    __shared__ double s_blp[4], s_bell[4];
    __shared__ int s_bidx[4];
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int rows = tl.rows, ncell = tl.ncell;
    // the tile's maximum and its first cell
    loc_best_wave(best);
    if (lane == 0) { s_blp[wv] = best.lp; s_bell[wv] = best.ell; s_bidx[wv] = best.idx; }
    __syncthreads();
    best = LocBest{s_blp[0], s_bell[0], s_bidx[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w) loc_better(best, s_blp[w], s_bell[w], s_bidx[w]);
    double *rec = jb.part + ((size_t)tl.b * ((size_t)g.nz * g.tpl) + tl.tile) * g.stride;
    double *mx = rec + kLocHead, *pS = mx + g.nx, *pT = pS + g.rows;
    const bool none = best.idx == INT_MAX;      // (block-uniform)
    if (t == 0) {
        rec[0] = none ? -__builtin_inf() : best.lp;
        rec[1] = none ? -1.0 : (double)(tl.cell0 + best.idx);
        rec[2] = none ? 0.0 : best.ell;
    }
    if (none) {
        if (t == 0) rec[3] = 0.0;
        for (int i = t; i < g.nx + 2 * g.rows; i += kLocThreads) mx[i] = 0.0;
        return;
    }
    // weights relative to the tile's maximum, into LDS
#pragma unroll
    for (int k = 0; k < kLocPerThread; ++k) {
        const int c = t + kLocThreads * k;
        if (c < ncell) { const double v = lp_of(k); s_w[c] = loc_included(v) ? exp(v - best.lp) : 0.0; }
    }
    __syncthreads();
    // a wave per x-row: the row's weight and weight times x, lane-strided in ascending ix, then the wave sums' fixed tree
    for (int r = wv; r < g.rows; r += 4) {       // (wave-uniform; rows beyond the tile's give zeros)
        double v[2] = {0.0, 0.0};
        if (r < rows)
            for (int ix = lane; ix < g.nx; ix += 64) {
                const double w = s_w[r * g.nx + ix];
                v[0] += w;
                v[1] = __builtin_fma(w, map_centre(g.x0, g.dx, ix), v[1]);
            }
        wave_sum<2>(v);
        if (lane == 0) { s_S[r] = v[0]; pS[r] = v[0]; pT[r] = v[1]; }
    }
    // a thread per ix: the weight over the tile's rows, in ascending row order
    for (int ix = t; ix < g.nx; ix += kLocThreads) {
        double a = 0.0;
        for (int r = 0; r < rows; ++r) a += s_w[r * g.nx + ix];
        mx[ix] = a;
    }
    __syncthreads();
    if (wv == 0) {      // the tile's weight: the rows lane-strided, then the tree
        double a = 0.0;
        for (int r = lane; r < rows; r += 64) a += s_S[r];
        a = wave_sum1(a);
        if (lane == 0) rec[3] = a;
    }
}

// D pairs (LocPairT: htm_locate_plan.hpp) at a wave-uniform address, aligned to the pair, through the constant address space: scalar loads
template <class T, int D>
__device__ __forceinline__ void loc_ld_pairs(const LocPairT<T> *p, T (&a)[D], T (&b)[D])
{
    typedef T vec2 __attribute__((ext_vector_type(2)));
    typedef const vec2 __attribute__((address_space(4))) *CP;
    const CP q = (CP)(unsigned long long)p;
#pragma unroll
    for (int i = 0; i < D; ++i) { const vec2 v = q[i]; a[i] = v[0]; b[i] = v[1]; }
}

// Cell c of a tile of ncell cells whose first x-row is iy0: its centre's x and y and its log prior in x and y from the event's
// tables (nullptr: flat).  A thread without that cell takes cell 0 and drops it
__device__ __forceinline__ void loc_cell_xy(const LocGrid &g, int iy0, int ncell, const double *prior, int c, double &x, double &y, double &pxy)
{
    const int cc = c < ncell ? c : 0;
    const int r = cc / g.nx, ix = cc - r * g.nx;
    x = map_centre(g.x0, g.dx, ix);
    y = map_centre(g.y0, g.dy, iy0 + r);
    pxy = prior ? prior[ix] + prior[g.nx + iy0 + r] : 0.0;
}

// ---- the station rule of all five kernels that evaluate the forward model at a cell ---------------------------------------
// k_locate, k_locate_marginal, k_locate_draw_evidence (loc_station) and the residual pass, k_locate_res_best and
// k_locate_residuals (loc_station_res), are built from the same three statements: loc_distance, loc_residuals, LocSums::add.
//
// The demeaned misfit of a cell comes in one pass from the shifted identity sum p (r - m)^2 = sum p u^2 - (sum p u)^2 / sum p,
// u = r - r_0 (r_0: the first station's residual).  Per data type and per structure (D of them side by side: one for k_locate
// and the residual pass, a block of draws for the other two): the shifts and the running sums, and what falls out of them when
// the stations are through: the offset m = r_0 + s1 / sum p that the demeaning takes away, and chi2 = s2 - s1^2 / sum p
// (1 / sum p per data type: LocEv's rpst, rpsa)
template <int D>
struct LocSums {
    double r0t[D], r0a[D], t1[D], t2[D], a1[D], a2[D];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int q = 0; q < D; ++q) t1[q] = t2[q] = a1[q] = a2[q] = r0t[q] = r0a[q] = 0.0;
    }
    // a station's residual r of precision p into one data type's sums.  first: station 0, which gives the shift by the same
    // operations (its u is r - r, not a constant)
    __device__ __forceinline__ static void add(bool first, double r, double p, double &r0, double &s1, double &s2)
    {
        if (first) r0 = r;
        const double u = r - r0, pu = p * u;
        s1 += pu;
        s2 = __builtin_fma(pu, u, s2);
    }
    __device__ __forceinline__ double mt(const LocEv &ev, int q = 0) const { return r0t[q] + t1[q] * ev.rpst; }
    __device__ __forceinline__ double ma(const LocEv &ev, int q = 0) const { return r0a[q] + a1[q] * ev.rpsa; }
    __device__ __forceinline__ double chi2t(const LocEv &ev, int q = 0) const { return t2[q] - (t1[q] * t1[q]) * ev.rpst; }
    __device__ __forceinline__ double chi2a(const LocEv &ev, int q = 0) const { return a2[q] - (a1[q] * a1[q]) * ev.rpsa; }
};

// F32 = false: all arithmetic fp64.  F32 = true, the single-precision forward (event_misfit<.., F32>'s rule at a cell centre; T is
// float, and the structure comes as its float copies): the three coordinate differences are formed in fp64 and rounded to float;
// d = v_sqrt_f32(fma(dz, dz, fma(dy, dy, dx dx))) and log2 d = v_log_f32(d), once per (cell, station); per structure the travel
// time fma(d, 1 / vs, -tc) and the amplitude fma(-d, pi f / (qs vs), -fma(log2 d, ln 2, ac)) in float -- ln d is folded into the
// structure's own fma, as event_misfit has it, and is never formed by itself --; each synthetic is promoted to double BEFORE the
// observation is subtracted.  Observations, precisions, shifts and sums are fp64 in both forms: everything from `rt` and `ra` on
// is one text.
template <bool F32>
using loc_real = std::conditional_t<F32, float, double>;

// the distance d of the cell (x, y, z) from the station; and, where amplitudes are in use (UA), lg = -ln d (fp64) or log2 d (F32)
template <bool UA, bool F32>
__device__ __forceinline__ void loc_distance(const LocSta &st, double x, double y, double z, loc_real<F32> &d, loc_real<F32> &lg)
{
    lg = 0;
    if constexpr (F32) {
        const float dx = (float)(x - st.sx), dy = (float)(y - st.sy), dz = (float)(z - st.sz);
        d = __builtin_amdgcn_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
        if constexpr (UA) lg = __builtin_amdgcn_logf(d);
    } else {
        const double dx = x - st.sx, dy = y - st.sy, dz = z - st.sz;
        d = htm_sqrt(__builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx)));
        if constexpr (UA) lg = -htm_log(d);
    }
}

// The station's residuals (synthetic minus observation: cls_forward.f90:115-118, :201-204 as event_misfit) at the distance d
// under ONE structure -- 1 / vs, pi f / (qs vs), the station's corrections tc, ac --, each into structure q's sums as it is
// formed: the time sums are added before the amplitude residual is formed.  rt, ra: the residuals themselves (what MODE
// leaves out stays 0).  MODE: 1 travel times only, 2 amplitudes only, 3 both.
template <int MODE, bool F32, int D>
__device__ __forceinline__ void loc_residuals(const LocSta &st, bool first, loc_real<F32> d, loc_real<F32> lg, loc_real<F32> rbeta, loc_real<F32> katt,
                                              loc_real<F32> tc, loc_real<F32> ac, LocSums<D> &sm, int q, double &rt, double &ra)
{
    rt = 0.0; ra = 0.0;
    if constexpr ((MODE & 1) != 0) {
        if constexpr (F32) rt = (double)__builtin_fmaf(d, rbeta, -tc) - st.tob;
        else rt = __builtin_fma(d, rbeta, -tc) - st.tob;
        sm.add(first, rt, st.tpr, sm.r0t[q], sm.t1[q], sm.t2[q]);
    }
    if constexpr ((MODE & 2) != 0) {
        if constexpr (F32) ra = (double)__builtin_fmaf(-d, katt, -__builtin_fmaf(lg, 0.69314718055994531f, ac)) - st.aob;
        else ra = (__builtin_fma(-d, katt, lg) - ac) - st.aob;
        sm.add(first, ra, st.apr, sm.r0a[q], sm.a1[q], sm.a2[q]);
    }
}

// The station st at the cell (x, y, zc) under D structures, into the sums: the distance and its logarithm once, then every
// structure's residuals
template <int MODE, int D, bool F32>
__device__ __forceinline__ void loc_station(const LocSta &st, const loc_real<F32> (&tc)[D], const loc_real<F32> (&ac)[D], bool first, double x, double y,
                                            double zc, const loc_real<F32> (&rbeta)[D], const loc_real<F32> (&katt)[D], LocSums<D> &sm)
{
    loc_real<F32> d, lg;
    loc_distance<(MODE & 2) != 0, F32>(st, x, y, zc, d, lg);
#pragma unroll
    for (int q = 0; q < D; ++q) {
        double rt, ra;
        loc_residuals<MODE, F32>(st, first, d, lg, rbeta[q], katt[q], tc[q], ac[q], sm, q, rt, ra);
    }
}

// The same under the job's one structure as LocJob and the station's record hold it, for the residual pass, which wants the
// residuals themselves too
template <int MODE, bool F32>
__device__ __forceinline__ void loc_station_res(const LocSta &st, const LocJob &jb, bool first, double x, double y, double z, LocSums<1> &sm,
                                                double &rt, double &ra)
{
    loc_real<F32> d, lg;
    loc_distance<(MODE & 2) != 0, F32>(st, x, y, z, d, lg);
    if constexpr (F32) loc_residuals<MODE, F32>(st, first, d, lg, jb.rbeta32, jb.katt32, st.tc32, st.ac32, sm, 0, rt, ra);
    else loc_residuals<MODE, F32>(st, first, d, lg, jb.rbeta, jb.katt, st.tc, st.ac, sm, 0, rt, ra);
}

// the cell's log-likelihood term under structure q from the finished sums
template <int MODE, int D>
__device__ __forceinline__ double loc_term(const LocSums<D> &sm, const LocEv &ev, int q)
{
    double e = 0.0;
    if constexpr ((MODE & 1) != 0) e -= 0.5 * sm.chi2t(ev, q) + ev.ct;
    if constexpr ((MODE & 2) != 0) e -= 0.5 * sm.chi2a(ev, q) + ev.ca;
    return e;
}

template <int MODE, bool F32>
__global__ __launch_bounds__(256) void k_locate(LocGrid launch, LocJob jb)
{
    typedef loc_real<F32> T;
    const LocGrid g = loc_grid_of(launch, jb.org, blockIdx.y);
    constexpr int CHUNK = F32 ? kLocChunk32 : kLocChunk;
    __shared__ double s_w[kLocTile];
    const int t = threadIdx.x;
    const LocTile tl = loc_tile(g, jb);
    const int iy0 = tl.iy0, ncell = tl.ncell;
    const double zc = tl.zc;
    const LocSta *sta = jb.sta + (size_t)tl.b * jb.S;
    const LocEv ev = loc_ld_ev(jb.ev + tl.b);
    const double *prior = tl.prior;
    T rbeta[1], katt[1];
    if constexpr (F32) { rbeta[0] = jb.rbeta32; katt[0] = jb.katt32; }
    else { rbeta[0] = jb.rbeta; katt[0] = jb.katt; }

    double lp[kLocPerThread];
    LocBest best{-__builtin_inf(), 0.0, INT_MAX};
#pragma unroll
    for (int ch = 0; ch < kLocPerThread / CHUNK; ++ch) {
        double x[CHUNK], y[CHUNK], pxy[CHUNK];
        LocSums<1> sm[CHUNK];
        if (ch * CHUNK * kLocThreads >= ncell) {      // (block-uniform: no cell of this chunk exists)
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) lp[ch * CHUNK + k] = __builtin_nan("");
            continue;
        }
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
            loc_cell_xy(g, iy0, ncell, prior, t + kLocThreads * (ch * CHUNK + k), x[k], y[k], pxy[k]);
            sm[k].clear();
        }
        for (int j = 0; j < jb.S; ++j) {
            const LocSta st = loc_ld_sta(sta + j);
            T tc[1], ac[1];
            if constexpr (F32) { tc[0] = st.tc32; ac[0] = st.ac32; }
            else { tc[0] = st.tc; ac[0] = st.ac; }
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) loc_station<MODE, 1, F32>(st, tc, ac, j == 0, x[k], y[k], zc, rbeta, katt, sm[k]);
        }
#pragma unroll
        for (int k = 0; k < CHUNK; ++k)
            lp[ch * CHUNK + k] = loc_cell_done(g, jb, tl, t + kLocThreads * (ch * CHUNK + k), loc_term<MODE>(sm[k], ev, 0), pxy[k], best);
    }
    loc_tile_reduce(g, jb, tl, best, s_w, [&](int k) { return lp[k]; });
}

// ---- the structure marginalised over K draws -----------------------------------------------------------
// The term of a cell becomes log((1 / K) sum_k exp(l_k)), l_k the term k_locate evaluates under draw k's structure.  The
// distance of a (cell, station) and its logarithm do not depend on the structure: a lane forms them ONCE per block of
// kLocDraws draws and then applies every draw's 1 / vs, pi f / (qs vs) and corrections to them: loc_station, which k_locate
// calls with one structure.
//
//   k_locate_pack_draws  the draws' table: {1 / vs_k, pi f / (qs_k vs_k)} per draw and {t_corr_kj, a_corr_kj} per (station,
//                        draw), [station][draw] with the draws padded to whole blocks (the padding repeats the last draw and
//                        is never counted), so that a block's 16-byte pairs are contiguous and read with SCALAR loads
//   k_locate_marginal    k_locate's grid and tiles.  A thread evaluates kLocmCells of its cells side by side; per block of
//                        draws the station loop runs once.  Across the blocks a cell keeps (m, s), s = sum_k exp(l_k - m);
//                        the cells' log posteriors go to the LDS array that holds the weights afterwards (a thread's own
//                        words), so the loop over a thread's cells is a loop, not sixteen copies of the code.
template <class T>          // double, or float: the table of the single-precision forward, every entry rounded to float
struct LocDraws {
    const LocPairT<T> *vq;      // [Kpad] {1 / vs, pi f / (qs vs)}
    const LocPairT<T> *corr;    // [S][Kpad] {t_corr, a_corr}
    int K, Kpad;                // draws; padded to a multiple of kLocDraws
};

template <class T>
__global__ __launch_bounds__(256) void k_locate_pack_draws(int S, int K, int Kpad, const double *tc, const double *ac, const double *rbeta,
                                                           const double *katt, LocPairT<T> *corr, LocPairT<T> *vq)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)(S + 1) * Kpad) return;
    const int j = (int)(i / Kpad), k = min((int)(i - (long)j * Kpad), K - 1);
    if (j == S) vq[i - (long)S * Kpad] = LocPairT<T>{(T)rbeta[k], (T)katt[k]};
    else corr[i] = LocPairT<T>{(T)tc[(size_t)k * S + j], (T)ac[(size_t)k * S + j]};
}

template <int MODE, bool F32>
__global__ __launch_bounds__(256) void k_locate_marginal(LocGrid launch, LocJob jb, LocDraws<loc_real<F32>> dr)
{
    typedef loc_real<F32> T;
    const LocGrid g = loc_grid_of(launch, jb.org, blockIdx.y);
    constexpr int C = F32 ? kLocmCells32 : kLocmCells, D = kLocDraws;
    __shared__ double s_w[kLocTile];
    const int t = threadIdx.x;
    const LocTile tl = loc_tile(g, jb);
    const int ncell = tl.ncell;
    const double zc = tl.zc;
    const LocSta *sta = jb.sta + (size_t)tl.b * jb.S;
    const LocEv ev = loc_ld_ev(jb.ev + tl.b);
    const double *prior = tl.prior;
    const double log_K = htm_log((double)dr.K);

    LocBest best{-__builtin_inf(), 0.0, INT_MAX};
#pragma unroll 1
    for (int ch = 0; ch * C * kLocThreads < ncell; ++ch) {      // (block-uniform)
        double x[C], y[C], pxy[C], m[C], s[C];
        bool bad[C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            loc_cell_xy(g, tl.iy0, ncell, prior, t + kLocThreads * (ch * C + k), x[k], y[k], pxy[k]);
            m[k] = -__builtin_inf(); s[k] = 0.0; bad[k] = false;
        }
#pragma unroll 1
        for (int k0 = 0; k0 < dr.K; k0 += D) {                  // (uniform) a block of draws
            T rbeta[D], katt[D];
            loc_ld_pairs(dr.vq + k0, rbeta, katt);
            LocSums<D> sm[C];
#pragma unroll
            for (int k = 0; k < C; ++k) sm[k].clear();
            // a station's records are loaded once and serve the thread's cells; station 0 has a call of its own, so that the loop
            // over the others carries no selection per draw
            auto station = [&](int j, bool first) {
                const LocSta st = loc_ld_sta(sta + j);
                T tc[D], ac[D];
                loc_ld_pairs(dr.corr + (size_t)j * dr.Kpad + k0, tc, ac);
#pragma unroll
                for (int k = 0; k < C; ++k) loc_station<MODE, D, F32>(st, tc, ac, first, x[k], y[k], zc, rbeta, katt, sm[k]);
            };
            station(0, true);
            for (int j = 1; j < jb.S; ++j) station(j, false);
            // the block's terms, and into (m, s): the padding's draws (k0 + q >= K, uniform) are left out
#pragma unroll
            for (int k = 0; k < C; ++k) {
                double ell[D], mb = -__builtin_inf();
#pragma unroll
                for (int q = 0; q < D; ++q) {
                    const double e = loc_term<MODE>(sm[k], ev, q);
                    const bool in = k0 + q < dr.K;
                    ell[q] = in ? e : -__builtin_inf();
                    bad[k] = bad[k] || (in && e != e);
                    mb = e > mb && in ? e : mb;
                }
                const double mn = mb > m[k] ? mb : m[k], ref = mn == -__builtin_inf() ? 0.0 : mn;
                double acc = s[k] * exp(m[k] - ref);
#pragma unroll
                for (int q = 0; q < D; ++q) acc += exp(ell[q] - ref);
                s[k] = acc; m[k] = mn;
            }
        }
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const int c = t + kLocThreads * (ch * C + k);
            // (K equal draws: s = K exactly and the bracket is exactly 0; K = 1: the term itself)
            double ell = s[k] > 0.0 ? m[k] + (htm_log(s[k]) - log_K) : -__builtin_inf();      // (s = 0: every draw is -inf)
            if (bad[k] || s[k] != s[k]) ell = __builtin_nan("");
            const double v = loc_cell_done(g, jb, tl, c, ell, pxy[k], best);
            if (c < ncell) s_w[c] = v;
        }
    }
    loc_tile_reduce(g, jb, tl, best, s_w, [&](int k) { return s_w[t + kLocThreads * k]; });
}

// ---- the evidence of every draw, and what the draws weigh for a window ----------------------------------
// log_z[k] = log(sum over the included cells of exp(l_k + log prior) dx dy dz): what htm_forward_locate returns in loc[6] under
// draw k.  The reduce is the opposite of k_locate_marginal's, a sum over CELLS for each draw, so the loops are swapped:
//
//   k_locate_draw_evidence  k_locate_marginal's grid, tiles, LocJob (vol unused), LocDraws and table.  A block of kLoceDraws
//                           draws is the OUTER loop (block-uniform), the thread's cells t, t + 256, ... the inner one; per
//                           (cell, station, block) the distance and its logarithm are formed once (loc_station).  A lane
//                           keeps (m_q, s_q), s = sum exp(v - m) over its included cells, per draw of the block; after its cells the pairs are combined across the wave (the largest m by a xor
//                           tree, every lane's s rescaled to it, the wave sums' fixed tree) and across the four waves (LDS,
//                           wave order) into the tile's record part[event][tile][Kpad][2].  The padding's draws are never
//                           written; a tile without an included cell writes (-inf, 0).
//   k_locate_draw_combine   one workgroup per event, a thread per draw: the tiles in ascending order into log_z[k]; then over
//                           the draws, in a fixed order, the largest log_z and its lowest index, S1 = sum exp(log_z - M),
//                           S2 = sum exp(2 (log_z - M)): n_eff = S1^2 / S2, w_max = 1 / S1, log evidence of the mixture
//                           M + (log S1 - log K).
// No floating-point atomics: the bits depend on neither timing nor batching.
#ifndef HTM_LOCE_DRAWS
#define HTM_LOCE_DRAWS HTM_LOCM_DRAWS   // draws per block of k_locate_draw_evidence (measured: DESIGN.md 3.12)
#endif
constexpr int kLoceDraws = HTM_LOCE_DRAWS;
static_assert(kLoceDraws >= 1 && kLocDraws % kLoceDraws == 0, "the table is padded to whole blocks of kLocDraws draws");

// (m, s) += (mo, so), s = sum exp(v - m): the same bits whichever side is which (equal maxima: a plain sum)
__device__ __forceinline__ void loc_ms_merge(double &m, double &s, double mo, double so)
{
    const bool mine = m >= mo;
    const double hi = mine ? m : mo, lo = mine ? mo : m, s_hi = mine ? s : so, s_lo = mine ? so : s;
    const double e = lo == -__builtin_inf() ? 0.0 : exp(lo - hi);      // (both -inf: nothing on either side)
    m = hi; s = __builtin_fma(s_lo, e, s_hi);
}

template <int MODE, bool F32>
__global__ __launch_bounds__(256) void k_locate_draw_evidence(LocGrid g, LocJob jb, LocDraws<loc_real<F32>> dr)
{
    typedef loc_real<F32> T;
    constexpr int D = kLoceDraws;
    __shared__ double s_m[4][D], s_s[4][D];
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const LocTile tl = loc_tile(g, jb);
    const int ncell = tl.ncell;
    const double zc = tl.zc;
    const LocSta *sta = jb.sta + (size_t)tl.b * jb.S;
    const LocEv ev = loc_ld_ev(jb.ev + tl.b);
    const double *prior = tl.prior;
    double *rec = jb.part + ((size_t)tl.b * ((size_t)g.nz * g.tpl) + tl.tile) * ((size_t)dr.Kpad * 2);

#pragma unroll 1
    for (int k0 = 0; k0 < dr.K; k0 += D) {                      // (uniform) a block of draws
        T rbeta[D], katt[D];
        double m[D], s[D];
        loc_ld_pairs(dr.vq + k0, rbeta, katt);
#pragma unroll
        for (int q = 0; q < D; ++q) { m[q] = -__builtin_inf(); s[q] = 0.0; }
#pragma unroll 1
        for (int c0 = 0; c0 < ncell; c0 += kLocThreads) {       // (block-uniform) the thread's cells
            const int c = c0 + t;
            double x, y, pxy;
            loc_cell_xy(g, tl.iy0, ncell, prior, c, x, y, pxy);
            LocSums<D> sm;
            sm.clear();
            auto station = [&](int j, bool first) {             // (as in k_locate_marginal)
                const LocSta st = loc_ld_sta(sta + j);
                T tc[D], ac[D];
                loc_ld_pairs(dr.corr + (size_t)j * dr.Kpad + k0, tc, ac);
                loc_station<MODE, D, F32>(st, tc, ac, first, x, y, zc, rbeta, katt, sm);
            };
            station(0, true);
            for (int j = 1; j < jb.S; ++j) station(j, false);
#pragma unroll
            for (int q = 0; q < D; ++q) {
                const double ell = loc_term<MODE>(sm, ev, q);
                const double v = prior ? ell + (pxy + tl.pz) : ell;         // (loc_cell_done's log posterior)
                if (c < ncell && loc_included(v)) {             // one exponential per (cell, draw)
                    const bool up = v > m[q];
                    const double e = exp(up ? m[q] - v : v - m[q]);
                    s[q] = up ? __builtin_fma(s[q], e, 1.0) : s[q] + e;
                    m[q] = up ? v : m[q];
                }
            }
        }
        // the block's D pairs.  Across the wave: the largest m (a xor tree of comparisons), every lane's s rescaled to it -- one
        // exponential per draw -- and the wave sums' fixed tree; then the four waves in their order
#pragma unroll
        for (int q = 0; q < D; ++q) {
            double mw = m[q];
#pragma unroll
            for (int off = 32; off; off >>= 1) { const double o = __shfl_xor(mw, off); mw = o > mw ? o : mw; }
            s[q] = m[q] == -__builtin_inf() ? 0.0 : s[q] * exp(m[q] - mw);      // (a lane without an included cell: s = 0)
            m[q] = mw;
        }
        wave_sum<D>(s);
        __syncthreads();                                       // (the block before has been read)
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < D; ++q) { s_m[wv][q] = m[q]; s_s[wv][q] = s[q]; }
        }
        __syncthreads();
        if (t < D && k0 + t < dr.K) {                           // (the padding's draws are never written)
            double mm = s_m[0][t], ss = s_s[0][t];
            for (int w = 1; w < 4; ++w) loc_ms_merge(mm, ss, s_m[w][t], s_s[w][t]);
            rec[2 * (size_t)(k0 + t)] = mm; rec[2 * (size_t)(k0 + t) + 1] = ss;
        }
    }
}

// One workgroup of 256 threads per event of the batch.  part [nb][n_tiles][Kpad][2], log_z [nb][K], summary [nb][4] = n_eff,
// w_max, k_max, log evidence of the mixture.
__global__ __launch_bounds__(256) void k_locate_draw_combine(int n_tiles, int K, int Kpad, const double *part, double log_cell, double *log_z,
                                                             double *summary)
{
    __shared__ double s_red4[4];
    __shared__ double s_blp[4];
    __shared__ int s_bidx[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.x;
    const double *P = part + (size_t)b * n_tiles * ((size_t)Kpad * 2);
    double *Z = log_z + (size_t)b * K;
    // a thread per draw, the tiles in ascending order: neighbouring threads read neighbouring pairs
    LocBest best{-__builtin_inf(), 0.0, INT_MAX};
    for (int k = t; k < K; k += 256) {
        double m = -__builtin_inf(), s = 0.0;
        for (int i = 0; i < n_tiles; ++i) { const double mt = P[((size_t)i * Kpad + k) * 2]; m = mt > m ? mt : m; }
        if (m != -__builtin_inf())
            for (int i = 0; i < n_tiles; ++i) {
                const double *r = P + ((size_t)i * Kpad + k) * 2;
                s = __builtin_fma(r[1], exp(r[0] - m), s);      // (an empty tile: 0 exp(-inf))
            }
        const double z = m != -__builtin_inf() ? (m + htm_log(s)) + log_cell : -__builtin_inf();
        Z[k] = z;
        loc_better(best, z, 0.0, k);
    }
    // the largest log_z and its lowest index
    loc_best_wave(best);
    if (lane == 0) { s_blp[wv] = best.lp; s_bidx[wv] = best.idx; }
    __syncthreads();
    best = LocBest{s_blp[0], 0.0, s_bidx[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w) loc_better(best, s_blp[w], 0.0, s_bidx[w]);
    const double M = best.lp;
    if (M == -__builtin_inf()) {        // (block-uniform) no included cell under any draw
        if (t < 4) summary[(size_t)b * 4 + t] = t == 2 ? -1.0 : __builtin_nan("");
        return;
    }
    // the weights relative to the heaviest draw: every thread its own draws in ascending order (it wrote them), then the fixed tree
    double a1 = 0.0, a2 = 0.0;
    for (int k = t; k < K; k += 256) { const double d = Z[k] - M; a1 += exp(d); a2 += exp(2.0 * d); }      // (exp(-inf) = 0)
    const double S1 = loc_block_sum(a1, s_red4), S2 = loc_block_sum(a2, s_red4);
    if (t == 0) {
        double *R = summary + (size_t)b * 4;
        R[0] = S1 * S1 / S2; R[1] = 1.0 / S1; R[2] = (double)best.idx; R[3] = M + (htm_log(S1) - htm_log((double)K));
    }
}

// One workgroup of 256 threads per event of the batch.  loc [nb][16], marg [nb][nx + ny + nz] (always there: the moments are
// taken from the marginals).
// wsum [nb] or nullptr: the event's weight sum W (0 for an event without an included cell), for k_locate_stack.
// org [nb][4] or nullptr: the events' box origins, as LocJob's.
__global__ __launch_bounds__(256) void k_locate_combine(LocGrid launch, double *part, double log_cell, double *loc, double *marg, double *wsum,
                                                        const double *org)
{
    const LocGrid g = loc_grid_of(launch, org, blockIdx.x);
    __shared__ double s_red4[4];
    __shared__ double s_blp[4], s_bell[4], s_bidx[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.x;
    const int n_tiles = g.nz * g.tpl, nm = g.nx + g.ny + g.nz;
    double *P = part + (size_t)b * n_tiles * g.stride;
    double *L = loc + (size_t)b * 16, *M = marg + (size_t)b * nm;
    const double nan = __builtin_nan("");

    // the event's maximum and its first cell: the tiles are in ascending order of their cells' indices
    double blp = -__builtin_inf(), bell = 0.0, bidx = -1.0;
    auto better = [&](double lp, double ell, double idx) {
        const bool take = idx >= 0.0 && (lp > blp || bidx < 0.0 || (lp == blp && idx < bidx));
        blp = take ? lp : blp; bell = take ? ell : bell; bidx = take ? idx : bidx;
    };
    for (int k = t; k < n_tiles; k += 256) { const double *r = P + (size_t)k * g.stride; better(r[0], r[2], r[1]); }
#pragma unroll
    for (int off = 32; off; off >>= 1) better(__shfl_xor(blp, off), __shfl_xor(bell, off), __shfl_xor(bidx, off));
    if (lane == 0) { s_blp[wv] = blp; s_bell[wv] = bell; s_bidx[wv] = bidx; }
    __syncthreads();
    blp = s_blp[0]; bell = s_bell[0]; bidx = s_bidx[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) better(s_blp[w], s_bell[w], s_bidx[w]);
    if (bidx < 0.0) {       // (block-uniform) no included cell
        if (t == 0 && wsum) wsum[b] = 0.0;
        if (t < 16) L[t] = t == 0 ? -1.0 : nan;
        for (int i = t; i < nm; i += 256) M[i] = nan;
        return;
    }
    // every tile's scale exp(max_tile - max_event) takes the place of its maximum (an empty tile: exp(-inf) = 0)
    for (int k = t; k < n_tiles; k += 256) { double *r = P + (size_t)k * g.stride; r[0] = exp(r[0] - blp); }
    __syncthreads();
    // the weight sum: tiles thread-strided in ascending order, then the fixed tree
    double acc = 0.0;
    for (int k = t; k < n_tiles; k += 256) { const double *r = P + (size_t)k * g.stride; acc = __builtin_fma(r[0], r[3], acc); }
    const double W = loc_block_sum(acc, s_red4);
    // the marginals, every entry by one thread in tile order, divided by the weight sum
    for (int ix = t; ix < g.nx; ix += 256) {
        double a = 0.0;
        for (int k = 0; k < n_tiles; ++k) { const double *r = P + (size_t)k * g.stride; a = __builtin_fma(r[0], r[kLocHead + ix], a); }
        M[ix] = a / W;
    }
    for (int iy = t; iy < g.ny; iy += 256) {
        const int tl = iy / g.rows, rr = iy - tl * g.rows;
        double a = 0.0;
        for (int iz = 0; iz < g.nz; ++iz) { const double *r = P + (size_t)(iz * g.tpl + tl) * g.stride; a = __builtin_fma(r[0], r[kLocHead + g.nx + rr], a); }
        M[g.nx + iy] = a / W;
    }
    for (int iz = t; iz < g.nz; iz += 256) {
        double a = 0.0;
        for (int tl = 0; tl < g.tpl; ++tl) { const double *r = P + (size_t)(iz * g.tpl + tl) * g.stride; a = __builtin_fma(r[0], r[3], a); }
        M[g.nx + g.ny + iz] = a / W;
    }
    __syncthreads();
    // mean and variances from the marginals: the mean as the best cell's centre plus the mean offset from it (a posterior that
    // sits in one cell of an axis has that centre for its mean, exactly), the variances about the mean
    const long cb = (long)bidx;
    const int bz = (int)(cb / ((long)g.nx * g.ny)), by = (int)((cb - (long)bz * g.nx * g.ny) / g.nx), bx = (int)(cb - ((long)bz * g.ny + by) * g.nx);
    const double v0[3] = {g.x0, g.y0, g.z0}, dv[3] = {g.dx, g.dy, g.dz};
    const int n[3] = {g.nx, g.ny, g.nz}, off[3] = {0, g.nx, g.nx + g.ny}, bi[3] = {bx, by, bz};
    double mean[3], var[3], bc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        bc[a] = map_centre(v0[a], dv[a], bi[a]);
        double s = 0.0;
        for (int i = t; i < n[a]; i += 256) s = __builtin_fma(M[off[a] + i], map_centre(v0[a], dv[a], i) - bc[a], s);
        mean[a] = bc[a] + loc_block_sum(s, s_red4);
        s = 0.0;
        for (int i = t; i < n[a]; i += 256) { const double d = map_centre(v0[a], dv[a], i) - mean[a]; s = __builtin_fma(M[off[a] + i] * d, d, s); }
        var[a] = loc_block_sum(s, s_red4);
    }
    // the mixed moments about the mean from the rows' sums: tiles thread-strided, a tile's rows in order
    double cxy = 0.0, cxz = 0.0, cyz = 0.0;
    for (int k = t; k < n_tiles; k += 256) {
        const double *r = P + (size_t)k * g.stride, *pS = r + kLocHead + g.nx, *pT = pS + g.rows;
        const int iz = k / g.tpl, iy0 = (k - iz * g.tpl) * g.rows, rows = min(g.rows, g.ny - iy0);
        double A = 0.0, B = 0.0, C = 0.0;
        for (int rr = 0; rr < rows; ++rr) {
            const double ex = pT[rr] - mean[0] * pS[rr], ey = map_centre(g.y0, g.dy, iy0 + rr) - mean[1];
            A += ex; B = __builtin_fma(ey, ex, B); C = __builtin_fma(ey, pS[rr], C);
        }
        const double ez = map_centre(g.z0, g.dz, iz) - mean[2];
        cxy = __builtin_fma(r[0], B, cxy); cxz = __builtin_fma(r[0] * ez, A, cxz); cyz = __builtin_fma(r[0] * ez, C, cyz);
    }
    cxy = loc_block_sum(cxy, s_red4) / W; cxz = loc_block_sum(cxz, s_red4) / W; cyz = loc_block_sum(cyz, s_red4) / W;
    if (t == 0) {
        L[0] = bidx; L[1] = bc[0]; L[2] = bc[1]; L[3] = bc[2];
        L[4] = blp; L[5] = bell; L[6] = (blp + htm_log(W)) + log_cell;
        L[7] = mean[0]; L[8] = mean[1]; L[9] = mean[2];
        L[10] = var[0]; L[11] = cxy; L[12] = cxz; L[13] = var[1]; L[14] = cyz; L[15] = var[2];
        if (wsum) wsum[b] = W;
    }
}

// ---- the stacked density of the windows' posteriors (the rule: include/htm_hip.h) ------------------------
// A window e of layer L with an included cell puts the mass exp(lp_e(c) - lp_best,e) * (1 / W_e) into cell c of stack[L]: one
// unit of mass per window.  The batch's log posteriors are read from the volume that k_locate / k_locate_marginal wrote, lp_best
// from the batch's loc records, W from k_locate_combine's wsum.
//
//   k_locate_stack          after a batch's k_locate_combine.  A thread owns a CELL, the batch's windows are the serial loop in
//                           event order: for a fixed window consecutive threads read consecutive lp.  What is uniform per window
//                           -- its layer, whether it takes part, lp_best, W -- comes through scalar loads.  kLocStkAhead
//                           windows' lp are requested before the first of them is added: the loads are independent, only the
//                           adds are ordered.  The thread keeps the running total of the current layer in a register; when the
//                           layer changes, and at the end, it writes it to stack[L][c], which only it owns, and on entering a
//                           layer it reads that layer's total first: a cell's total goes through memory unchanged from batch to
//                           batch, so its additions are the same however the windows are batched.  Thread 0 of block 0 counts
//                           the windows: tally[L][0] those that add their unit, tally[L][1] those without an included cell.
//   k_locate_stack_project  after the last batch: xy (sum over iz), xz (over iy), yz (over ix) of the finished stack.  xy and xz:
//                           a thread per map cell, the summed axis in ascending order, neighbouring threads neighbouring ix;
//                           yz: a wave per map cell, its x-row lane-strided in ascending ix, then the wave sums' fixed tree.
//                           Grid-stride loops: every map cell has one owner and an order that depends on the grid alone.
// No floating-point atomics.  All index arithmetic is in size_t or long: batch x cells passes 2^31.
constexpr int kLocStkAhead = 8;         // windows whose lp are in flight ahead of the accumulate

// one value at a wave-uniform address through the constant address space: a scalar load
template <class T>
__device__ __forceinline__ T loc_ld_uniform(const T *p)
{
    typedef const T __attribute__((address_space(4))) *CP;
    return *(CP)(unsigned long long)p;
}

// vol [nb][cells], loc [nb][16], wsum [nb]: the batch's; layer [n_events] or nullptr (every window in layer 0), e0 the batch's
// first event; stack [n_layer][cells], tally [n_layer][2]
__global__ __launch_bounds__(256) void k_locate_stack(long cells, int nb, int e0, const double *vol, const double *loc, const double *wsum,
                                                      const int *layer, int n_layer, double *stack, double *tally)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = c < cells;
    const size_t cc = live ? (size_t)c : 0;      // (a thread beyond the grid reads cell 0 and writes nothing)
    // the window's layer, or -1: it takes no part (uniform)
    auto layer_of = [&](int b) {
        const int L = layer ? loc_ld_uniform(layer + e0 + b) : 0;
        return L >= 0 && L < n_layer ? L : -1;
    };
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int b = 0; b < nb; ++b) {
            const int L = layer_of(b);
            if (L >= 0) tally[2 * (size_t)L + (loc[16 * (size_t)b] < 0.0 ? 1 : 0)] += 1.0;
        }
    int cur = -1;
    double acc = 0.0;
    for (int b0 = 0; b0 < nb; b0 += kLocStkAhead) {
        // the requests of the block's windows, unconditional so that they are counted: beyond the batch's end the last window
        // is read again and dropped
        double v[kLocStkAhead], idx[kLocStkAhead], best[kLocStkAhead], w[kLocStkAhead];
        int lay[kLocStkAhead];
#pragma unroll
        for (int q = 0; q < kLocStkAhead; ++q) {
            const int b = min(b0 + q, nb - 1);
            v[q] = vol[(size_t)b * (size_t)cells + cc];
            lay[q] = layer_of(b);
            idx[q] = loc_ld_uniform(loc + 16 * (size_t)b); best[q] = loc_ld_uniform(loc + 16 * (size_t)b + 4); w[q] = loc_ld_uniform(wsum + b);
        }
#pragma unroll
        for (int q = 0; q < kLocStkAhead; ++q) {
            if (b0 + q >= nb) break;                                     // (uniform)
            const int L = lay[q];
            if (L < 0 || idx[q] < 0.0) continue;                         // (uniform) it takes no part, or has no included cell
            if (L != cur) {
                if (cur >= 0 && live) stack[(size_t)cur * (size_t)cells + cc] = acc;
                cur = L;
                acc = live ? stack[(size_t)L * (size_t)cells + cc] : 0.0;
            }
            const double rw = 1.0 / w[q];                                // (uniform: once per window)
            acc += loc_included(v[q]) ? exp(v[q] - best[q]) * rw : 0.0;
        }
    }
    if (cur >= 0 && live) stack[(size_t)cur * (size_t)cells + cc] = acc;
}

__global__ __launch_bounds__(256) void k_locate_stack_project(LocGrid g, int n_layer, const double *stack, double *xy, double *xz, double *yz)
{
    const size_t nx = g.nx, ny = g.ny, nz = g.nz, cells = nx * ny * nz, nl = n_layer;
    const size_t n_thr = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t i = t0; i < nl * ny * nx; i += n_thr) {                  // xy [layer][iy][ix]: iz ascending
        const size_t L = i / (nx * ny);
        const double *p = stack + L * cells + (i - L * nx * ny);
        double a = 0.0;
        for (size_t iz = 0; iz < nz; ++iz) a += p[iz * nx * ny];
        xy[i] = a;
    }
    for (size_t i = t0; i < nl * nz * nx; i += n_thr) {                  // xz [layer][iz][ix]: iy ascending
        const size_t L = i / (nx * nz), r = i - L * nx * nz, iz = r / nx;
        const double *p = stack + L * cells + iz * nx * ny + (r - iz * nx);
        double a = 0.0;
        for (size_t iy = 0; iy < ny; ++iy) a += p[iy * nx];
        xz[i] = a;
    }
    const size_t lane = threadIdx.x & 63;
    for (size_t i = t0 >> 6; i < nl * nz * ny; i += n_thr >> 6) {        // yz [layer][iz][iy] (wave-uniform): the x-row i of the stack
        const double *p = stack + i * nx;
        double a = 0.0;
        for (size_t ix = lane; ix < nx; ix += 64) a += p[ix];
        a = wave_sum1(a);
        if (lane == 0) yz[i] = a;
    }
}

// ---- the stations' residuals, the source terms and the fit of every window (the rule: include/htm_hip.h) --
// What the forward model demeans away and what is left of a station after it, at the best cell and as means over the window's
// posterior: with r_j(c) station j's residual (synthetic minus observation) at cell c and p_j its precision, the offset
// m(c) = sum_j p_j r_j(c) / sum_j p_j, the residual rho_j(c) = m(c) - r_j(c) and chi2(c) = sum_j p_j rho_j(c)^2; the weights
// w(c) = exp(lp(c) - lp_best) of the included cells, W their sum.  A posterior mean is taken about the best cell, mean(q) =
// q(best) + sum_c w(c) (q(c) - q(best)) / W, so everything a cell adds is a DIFFERENCE from the best cell's value, which the best
// cell itself and a posterior of one cell give as exact zeros.  The batch's log posteriors are read from the volume that k_locate
// wrote, lp_best and the best index from its loc records, W from k_locate_combine's wsum: after a batch's k_locate_combine.
//
//   k_locate_res_best     one wave per event, the stations in their order (uniform: scalar loads, every lane the same numbers):
//                         r_j(best) per station and data type, then m(best) and chi2(best) from the shifted sums, by the very
//                         operations that k_locate_residuals applies to a cell (loc_station_res: k_locate's station rule)
//   k_locate_residuals    grid = (blocks of kLocResBlock cells, events of the batch); cells by linear index, a thread owns the
//                         cells t, t + 256, ... of its block, kLocResCells side by side.  ONE station loop per cell (uniform,
//                         the outer loop): per station the lanes' sum_k w (r_j - r_j(best)) goes through the wave sums' fixed
//                         tree and lane 0 puts it into LDS; after kLocResSta stations, and at the end, the four waves' values
//                         are added in wave order and written to the block's partial record -- a barrier per kLocResSta
//                         stations, none per station.  When the loop ends the cell's m and chi2 fall out of the shifted sums;
//                         the event's own sums (kLocResEv) close the record.  An excluded cell, and a thread beyond the grid's
//                         end (which reads cell 0), contribute by SELECTION, never by 0 * value: their residuals may be NaN or
//                         infinite.
//   k_locate_res_combine  one workgroup per event: a thread per station adds the partial records in ascending block order; res
//                         and fit.  An event without an included cell, and a data type that is not in use, give NaN.
// No floating-point atomics; no cap on n_sta.  All index arithmetic is in size_t or long.
struct LocRes {
    const double *loc, *wsum;       // [nb][16], [nb]: k_locate_combine's
    double *base;                   // [nb][2 S + kLocResBase]
    double *part;                   // [nb][n_blk][2 S + kLocResEv]
    double *res, *fit;              // [nb][S][4], [nb][10]
    long cells;
    int n_blk;
};

// the centre of the cell of linear index c
__device__ __forceinline__ void loc_res_centre(const LocGrid &g, long c, double &x, double &y, double &z)
{
    const long nxy = (long)g.nx * g.ny;
    const int iz = (int)(c / nxy), iy = (int)((c - (long)iz * nxy) / g.nx), ix = (int)(c - (long)iz * nxy - (long)iy * g.nx);
    x = map_centre(g.x0, g.dx, ix); y = map_centre(g.y0, g.dy, iy); z = map_centre(g.z0, g.dz, iz);
}

template <int MODE, bool F32>
__global__ __launch_bounds__(64) void k_locate_res_best(LocGrid g, LocJob jb, LocRes rs)
{
    const int b = blockIdx.x, S = jb.S;
    const double idx = loc_ld_uniform(rs.loc + 16 * (size_t)b);
    if (idx < 0.0) return;                                  // (uniform) no included cell: k_locate_res_combine writes the NaN
    const LocSta *sta = jb.sta + (size_t)b * S;
    const LocEv ev = loc_ld_ev(jb.ev + b);
    double *base = rs.base + (size_t)b * (2 * (size_t)S + kLocResBase);
    double x, y, z;
    loc_res_centre(g, (long)idx, x, y, z);
    LocSums<1> sm;
    sm.clear();
    for (int j = 0; j < S; ++j) {
        const LocSta st = loc_ld_sta(sta + j);
        double rt, ra;
        loc_station_res<MODE, F32>(st, jb, j == 0, x, y, z, sm, rt, ra);
        if (threadIdx.x == 0) { base[2 * (size_t)j] = rt; base[2 * (size_t)j + 1] = ra; }
    }
    if (threadIdx.x == 0) {
        double *q = base + 2 * (size_t)S;
        q[0] = sm.mt(ev); q[1] = sm.chi2t(ev); q[2] = sm.ma(ev); q[3] = sm.chi2a(ev);
    }
}

template <int MODE, bool F32>
__global__ __launch_bounds__(256) void k_locate_residuals(LocGrid g, LocJob jb, LocRes rs)
{
    constexpr bool UT = (MODE & 1) != 0, UA = (MODE & 2) != 0;
    constexpr int C = kLocResCells;
    __shared__ double s_sta[4][kLocResSta][2];
    __shared__ double s_ev[4][kLocResEv];
    const int t = threadIdx.x, lane = t & 63, b = blockIdx.y, S = jb.S;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const double idx = loc_ld_uniform(rs.loc + 16 * (size_t)b);
    if (idx < 0.0) return;                                  // (uniform) no included cell: nothing of this event's records is read
    const double lp_best = loc_ld_uniform(rs.loc + 16 * (size_t)b + 4);
    const LocSta *sta = jb.sta + (size_t)b * S;
    const LocEv ev = loc_ld_ev(jb.ev + b);
    const size_t reclen = 2 * (size_t)S + kLocResEv;
    const double *base = rs.base + (size_t)b * (2 * (size_t)S + kLocResBase);
    double *rec = rs.part + ((size_t)b * rs.n_blk + blockIdx.x) * reclen;
    const double *vol = jb.vol + (size_t)b * (size_t)rs.cells;

    double x[C], y[C], z[C], w[C];
    bool inc[C];
    LocSums<1> sm[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const long c = (long)blockIdx.x * kLocResBlock + kLocThreads * k + t;
        const bool live = c < rs.cells;
        const long cc = live ? c : 0;                       // (a thread beyond the end reads cell 0 and adds nothing)
        const double v = vol[(size_t)cc];
        inc[k] = live && loc_included(v);
        w[k] = inc[k] ? exp(v - lp_best) : 0.0;
        loc_res_centre(g, cc, x[k], y[k], z[k]);
        sm[k].clear();
    }
    for (int j0 = 0; j0 < S; j0 += kLocResSta) {            // (uniform) a block of stations
        const int nj = min(kLocResSta, S - j0);
        for (int jj = 0; jj < nj; ++jj) {
            const int j = j0 + jj;
            const LocSta st = loc_ld_sta(sta + j);
            const loc_f64x2 rb = *(const loc_f64x2 __attribute__((address_space(4))) *)(unsigned long long)(base + 2 * (size_t)j);
            double v[2] = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < C; ++k) {
                double rt, ra;
                loc_station_res<MODE, F32>(st, jb, j == 0, x[k], y[k], z[k], sm[k], rt, ra);
                if constexpr (UT) v[0] += inc[k] ? w[k] * (rt - rb[0]) : 0.0;
                if constexpr (UA) v[1] += inc[k] ? w[k] * (ra - rb[1]) : 0.0;
            }
            wave_sum<2>(v);
            if (lane == 0) { s_sta[wv][jj][0] = v[0]; s_sta[wv][jj][1] = v[1]; }
        }
        __syncthreads();
        if (t < 2 * nj) {
            const int jj = t >> 1, d = t & 1;
            rec[2 * (size_t)j0 + t] = loc_sum4(&s_sta[0][jj][d], 2 * kLocResSta);
        }
        __syncthreads();                                    // (read before the next block of stations overwrites it)
    }
    // the cells' offsets and chi2 against the best cell's, and the event's sums
    const double *q = base + 2 * (size_t)S;
    const double mtb = loc_ld_uniform(q), ctb = loc_ld_uniform(q + 1), mab = loc_ld_uniform(q + 2), cab = loc_ld_uniform(q + 3);
    double e[kLocResEv];
#pragma unroll
    for (int i = 0; i < kLocResEv; ++i) e[i] = 0.0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        if constexpr (UT) {
            const double u = sm[k].mt(ev) - mtb, wu = w[k] * u;
            e[0] += inc[k] ? wu : 0.0; e[1] += inc[k] ? wu * u : 0.0; e[2] += inc[k] ? w[k] * (sm[k].chi2t(ev) - ctb) : 0.0;
        }
        if constexpr (UA) {
            const double u = sm[k].ma(ev) - mab, wu = w[k] * u;
            e[3] += inc[k] ? wu : 0.0; e[4] += inc[k] ? wu * u : 0.0; e[5] += inc[k] ? w[k] * (sm[k].chi2a(ev) - cab) : 0.0;
        }
    }
    wave_sum<kLocResEv>(e);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kLocResEv; ++i) s_ev[wv][i] = e[i];
    }
    __syncthreads();
    if (t < kLocResEv) rec[2 * (size_t)S + t] = loc_sum4(&s_ev[0][t], kLocResEv);
}

// use_t, use_a: the data types of the handle
__global__ __launch_bounds__(256) void k_locate_res_combine(LocRes rs, int S, int use_t, int use_a)
{
    __shared__ double s_ev[kLocResEv];
    const int t = threadIdx.x, b = blockIdx.x;
    const double nan = __builtin_nan("");
    double *R = rs.res + (size_t)b * 4 * (size_t)S, *F = rs.fit + (size_t)b * 10;
    if (rs.loc[16 * (size_t)b] < 0.0) {                     // (block-uniform) no included cell
        for (size_t i = t; i < 4 * (size_t)S; i += 256) R[i] = nan;
        if (t < 10) F[t] = nan;
        return;
    }
    const size_t reclen = 2 * (size_t)S + kLocResEv;
    const double *P = rs.part + (size_t)b * rs.n_blk * reclen;
    const double *base = rs.base + (size_t)b * (2 * (size_t)S + kLocResBase), *q = base + 2 * (size_t)S;
    const double W = rs.wsum[b];
    if (t < kLocResEv) {
        double a = 0.0;
        for (int i = 0; i < rs.n_blk; ++i) a += P[(size_t)i * reclen + 2 * (size_t)S + t];
        s_ev[t] = a;
    }
    __syncthreads();
    const int use[2] = {use_t, use_a};
    for (int j = t; j < S; j += 256)
        for (int d = 0; d < 2; ++d) {
            double best = nan, mean = nan;
            if (use[d]) {
                double a = 0.0;
                for (int i = 0; i < rs.n_blk; ++i) a += P[(size_t)i * reclen + 2 * (size_t)j + d];
                best = q[2 * d] - base[2 * (size_t)j + d];
                mean = best + (s_ev[3 * d] - a) / W;
            }
            R[4 * (size_t)j + 2 * d] = best; R[4 * (size_t)j + 2 * d + 1] = mean;
        }
    if (t < 2) {
        const int d = t;
        double f[5] = {nan, nan, nan, nan, nan};
        if (use[d]) {
            const double m1 = s_ev[3 * d] / W, var = s_ev[3 * d + 1] / W - m1 * m1;
            f[0] = q[2 * d]; f[1] = q[2 * d] + m1; f[2] = var > 0.0 ? htm_sqrt(var) : 0.0;      // (floored at 0)
            f[3] = q[2 * d + 1]; f[4] = q[2 * d + 1] + s_ev[3 * d + 2] / W;
        }
        for (int i = 0; i < 5; ++i) F[5 * d + i] = f[i];
    }
}

}  // namespace htm
