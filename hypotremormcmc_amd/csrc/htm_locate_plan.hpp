// htm_locate_plan.hpp -- the batch plan of the locate entry points (htm_locate.hip), worked out by plain functions without a
// device: the tiles of the grid, the length of every device array of a call, the bytes they take under HTM_LOCATE_MB and the
// events per batch.  htm_forward_locate_plan (include/htm_hip.h, which states the formula) asks it for any shape on a machine
// without a GPU; tests/test_locate_plan.py pins it there.  Plain C++17, nothing of HIP: the constants and records that both the
// plan and the kernels (htm_locate.hpp) need are defined here, once.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>

#include "htm_grid.hpp"
#include "htm_limits.hpp"

#pragma GCC visibility push(hidden)

namespace htm {

constexpr int kLocThreads = 256;
constexpr int kLocPerThread = 16;       // cells of a tile per thread
constexpr int kLocTile = kLocThreads * kLocPerThread;
constexpr int kLocRows = 256;           // x-rows per tile at the most
constexpr int kLocHead = 4;
static_assert(kLocTile >= kMapMaxCells, "a tile holds at least one whole x-row");
// k_locate_marginal: draws per block (the choice and its alternatives: DESIGN.md 3.11)
#ifndef HTM_LOCM_DRAWS
#define HTM_LOCM_DRAWS 8
#endif
constexpr int kLocDraws = HTM_LOCM_DRAWS;
constexpr int kLocMaxDraws = 4096;      // draws per call (include/htm_hip.h)
static_assert(kLocDraws >= 1 && kLocMaxDraws % kLocDraws == 0, "whole blocks of draws");
// k_locate_residuals: cells of a thread side by side, the cells of a workgroup (one partial record each), the stations whose
// sums cross the four waves together, and the event's own sums at a record's end
constexpr int kLocResCells = 4;
constexpr int kLocResBlock = kLocThreads * kLocResCells;
constexpr int kLocResSta = 64;
constexpr int kLocResEv = 6;            // per data type: sum w u, sum w u^2 (u = m - m(best)), sum w (chi2 - chi2(best))
constexpr int kLocResBase = 4;          // per data type: m(best), chi2(best), behind the stations' residuals at the best cell

// what the evaluation reads of one station for one event; 80 bytes, read with scalar loads.  tc32, ac32: tc and ac rounded to
// float, for the single-precision forward
struct __attribute__((aligned(16))) LocSta {
    double sx, sy, sz, tc, ac, tob, tpr, aob, apr;
    float tc32, ac32;
};
static_assert(sizeof(LocSta) == 80, "nine doubles and two floats: the record kept its size");
// per event: 1 / sum of precisions (time, amplitude) and sum_j (log_2pi_half + log stdv_j) (time, amplitude)
struct __attribute__((aligned(16))) LocEv {
    double rpst, rpsa, ct, ca;
};
// a pair of T: doubles, or the floats of the single-precision forward (the draws' table)
template <class T>
struct __attribute__((aligned(2 * sizeof(T)))) LocPairT {
    T a, b;
};
typedef LocPairT<double> LocPair;

struct LocGrid : MapGrid {
    int rows;        // x-rows per tile
    int tpl;         // tiles per z-layer
    int stride;      // doubles per partial record
};

// ---- what a call wants --------------------------------------------------------------------------------------------
enum { kLocFixed = 0, kLocMarginal = 1, kLocEvidence = 2 };      // HTM_LOCATE_FIXED .. of include/htm_hip.h
struct LocRequest {
    int n_sta, n_events;
    int job;            // kLocFixed: one structure; kLocMarginal: the mixture over the draws; kLocEvidence: every draw's evidence
    int n_draws;        // 0 under a fixed structure
    bool volume;        // every event's volume of log posteriors is asked for (a stack keeps one on the device whether or not)
    bool prior;         // prior tables are given (false: flat)
    int n_layer;        // layers of the stack; 0: no stack
    bool layer;         // the stack has a layer per window
    bool fp32;          // the single-precision forward: the draws' table holds pairs of floats
    bool residuals;     // htm_forward_locate_residuals: the stations' residuals and the fit (kLocFixed only, without a stack)
    bool boxes;         // htm_forward_locate_boxes: a box origin per event (kLocFixed and kLocMarginal, without a stack or residuals)
};

// ---- what the run needs -------------------------------------------------------------------------------------------
// The length, in elements, of every device array of a call; 0: the call has no such array.  The workspace allocates from these
// and the byte totals below are sums over these, so a length is written down once.
struct LocLengths {
    // per event of a batch
    size_t sta, ev;                  // LocSta, LocEv
    size_t part;                     // the tiles' partial records, or a pair per tile and draw of the padded table
    size_t logz, sum;                // the draws' evidences and their summary
    size_t loc, marg, prior, vol;
    size_t w;                        // the event's weight sum, for the stack
    size_t org;                      // the event's box origin x0, y0, z0 and one unused: two aligned pairs of doubles; boxes only
    // once per call
    size_t dtc, dac, rk;             // the draws as they come, and their 1 / vs and pi f / (qs vs): the pack kernel's input
    size_t corr, vq;                 // the draws' table, pairs
    size_t stack, xy, xz, yz, tally;
    size_t layer;                    // ints
    // per event of a batch, of a call with residuals
    size_t rbase;                    // the stations' residuals at the best cell, {t, a} each, then m and chi2 there
    size_t rpart;                    // the partial records of the residual pass: per block of cells [n_sta][2] and the event's sums
    size_t res, fit;
};
enum { kLocByEvents, kLocByTiles, kLocByPack, kLocByBudget, kLocLimits };
struct LocPlan {
    LocGrid g;
    long cells, n_tiles, nm, map_cells;      // nm: the marginals' length nx + ny + nz; map_cells: nx ny + nx nz + ny nz
    long n_rblk;                             // blocks of kLocResBlock cells: the residual pass's workgroups per event
    int K, Kpad;                             // draws; padded to whole blocks of kLocDraws
    LocLengths len;
    double per_event, table, fixed;          // bytes: per event of a batch; the draws' table and its input; the stack's part
    long limit[kLocLimits];                  // what each rule allows a batch (locate_budget)
    long nb;                                 // events per batch
};

// The grid and its tiles.  Refuses a bad grid and more than 2^31 - 1 cells.
inline int locate_tiles(const double *grid9, LocPlan *p)
{
    *p = LocPlan{};
    LocGrid &g = p->g;
    if (int rc = map_grid_parse(grid9, &g)) return rc;
    p->cells = (long)g.nx * g.ny * g.nz;
    if (p->cells > (long)INT_MAX) return fail(HTM_EINVAL, "%d x %d x %d cells: more than 2^31 - 1", g.nx, g.ny, g.nz);
    // tiles: whole x-rows of one z-layer, at most kLocRows of them and kLocTile cells
    g.rows = std::max(1, std::min(std::min(g.ny, kLocRows), kLocTile / g.nx));
    g.tpl = (g.ny + g.rows - 1) / g.rows;
    g.stride = kLocHead + g.nx + 2 * g.rows;
    // (a tile that is not a layer's last holds more than 2048 cells or 256 rows of at most 16: at most 2^31 / 256 + 4096 tiles, 2^31 work-items per event)
    p->n_tiles = (long)g.nz * g.tpl;
    p->nm = (long)g.nx + g.ny + g.nz;
    p->map_cells = (long)g.nx * g.ny + (long)g.nx * g.nz + (long)g.ny * g.nz;
    p->n_rblk = (p->cells + kLocResBlock - 1) / kLocResBlock;
    return HTM_OK;
}

// The lengths, the bytes and the batch of request `rq` on the grid that locate_tiles put into *p, under `mb` MiB.  Refuses, in
// this order: mb not positive (env_mib says so first where mb is HTM_LOCATE_MB's); the draws' table and one event above mb;
// a stack of more than 2^31 - 1 doubles; the stack, the table and one event above mb.
inline int locate_budget(const LocRequest &rq, double mb, LocPlan *p)
{
    if (!(mb > 0.0)) return fail(HTM_EINVAL, "HTM_LOCATE_MB = %g: a positive number of MiB", mb);
    const LocGrid &g = p->g;
    const bool draws = rq.job != kLocFixed, evid = rq.job == kLocEvidence, stk = rq.n_layer > 0;
    const size_t S = (size_t)rq.n_sta, cells = (size_t)p->cells, n_tiles = (size_t)p->n_tiles, nm = (size_t)p->nm;
    const int K = p->K = draws ? rq.n_draws : 0;
    const int Kpad = p->Kpad = (K + kLocDraws - 1) / kLocDraws * kLocDraws;

    LocLengths &n = p->len = LocLengths{};
    n.sta = S; n.ev = 1;
    if (evid) { n.part = n_tiles * Kpad * 2; n.logz = (size_t)K; n.sum = 4; }
    else { n.part = n_tiles * g.stride; n.loc = 16; n.marg = nm; }
    if (rq.prior) n.prior = nm;
    if (rq.volume || stk || rq.residuals) n.vol = cells;
    if (stk || rq.residuals) n.w = 1;
    if (rq.boxes) n.org = 4;
    if (rq.residuals) {
        n.rbase = 2 * S + kLocResBase; n.rpart = (size_t)p->n_rblk * (2 * S + kLocResEv);
        n.res = 4 * S; n.fit = 10;
    }
    if (draws) { n.dtc = n.dac = (size_t)K * S; n.rk = 2 * (size_t)K; n.corr = S * Kpad; n.vq = (size_t)Kpad; }

    // (the prior's tables are counted whether or not the call has a prior: a flat-prior call is planned as if it allocated them.
    // Every other term is an array of the call: the stack's + 1 of include/htm_hip.h is w, which a stacked call allocates; with
    // boxes, + 8 * 4 bytes: the event's origin)
    p->per_event = sizeof(double) * (double)(n.part + n.logz + n.sum + n.loc + n.marg + nm + n.vol + n.w + n.org + n.rbase + n.rpart + n.res + n.fit) +
                   sizeof(LocSta) * (double)n.sta +
                   sizeof(LocEv) * (double)n.ev;
    // the draws' table and the draws as they come are part of the workspace, once per call
    const size_t pair = rq.fp32 ? sizeof(LocPairT<float>) : sizeof(LocPairT<double>);
    p->table = pair * (double)(n.corr + n.vq) + sizeof(double) * (double)(n.dtc + n.dac + n.rk);
    if (draws && p->table + p->per_event > mb * 1048576.0)
        return fail(HTM_EINVAL, "HTM_LOCATE_MB = %g: the table of %d draws (%.0f bytes) and one event (%.0f bytes) do not fit", mb, K, p->table, p->per_event);
    // the stack: every layer's volume, its three maps and its tally, and the windows' layers, once per call
    p->fixed = 0.0;
    if (stk) {
        const double n_out = (double)rq.n_layer * ((double)p->cells + (double)p->map_cells + 2.0);
        if (n_out > (double)INT_MAX)
            return fail(HTM_EINVAL, "%d layers of %ld + %ld cells and a tally: more than 2^31 - 1 doubles", rq.n_layer, p->cells, p->map_cells);
        const size_t nl = (size_t)rq.n_layer;
        n.stack = nl * cells; n.xy = nl * g.nx * g.ny; n.xz = nl * g.nx * g.nz; n.yz = nl * g.ny * g.nz; n.tally = nl * 2;
        if (rq.layer) n.layer = (size_t)rq.n_events;
        p->fixed = sizeof(double) * (double)(n.stack + n.xy + n.xz + n.yz + n.tally) + sizeof(int) * (double)n.layer;
        if (p->fixed + p->table + p->per_event > mb * 1048576.0)
            return fail(HTM_EINVAL, "HTM_LOCATE_MB = %g: the stack of %d layers (%.0f bytes)%s and one event (%.0f bytes) do not fit", mb, rq.n_layer, p->fixed,
                        draws ? ", the table of the draws" : "", p->per_event);
    }
    // events per batch; one at the least, whatever the budget (only a call with a table or a stack is refused for it)
    p->limit[kLocByEvents] = 65535L;                                                  // a launch's grid: y <= 65535
    p->limit[kLocByTiles] = kMaxWorkItems / (p->n_tiles * kLocThreads);               // the evaluation: (tiles, events) blocks of kLocThreads
    if (rq.residuals)                                                                 // the residual pass: (blocks of cells, events), whichever are more
        p->limit[kLocByTiles] = kMaxWorkItems / (std::max(p->n_tiles, p->n_rblk) * kLocThreads);
    p->limit[kLocByPack] = (kMaxWorkItems - 256) / rq.n_sta;                          // k_locate_pack: a thread per (event, station), whole blocks of 256
    p->limit[kLocByBudget] = (long)std::min((mb * 1048576.0 - p->table - p->fixed) / p->per_event, 65535.0);      // the workspace under mb MiB
    p->nb = (long)rq.n_events;
    for (long l : p->limit) p->nb = std::min(p->nb, l);
    p->nb = std::max(p->nb, 1L);
    return HTM_OK;
}

// both, for a caller that has nothing of its own to check between them
inline int locate_plan(const LocRequest &rq, const double *grid9, double mb, LocPlan *p)
{
    if (int rc = locate_tiles(grid9, p)) return rc;
    return locate_budget(rq, mb, p);
}

}  // namespace htm

#pragma GCC visibility pop
