// htm_worker.hpp -- worker_body: the full-evaluation workers of a k_mcmc launch (blocks behind the master's, htm_mcmc.hpp), whichever
// loop the master runs.  The hand-off with the master: htm_handoff.hpp.
#pragma once
#include "htm_handoff.hpp"

namespace htm {

// Worker block of a k_mcmc launch: waits for work orders of its own launch and evaluates its event tile of
// every model in the order (same arithmetic as k_full: wave <-> event, lane <-> station).  Block w, wave v
// take events (w*8 + v) + k * 8 * W.  The immutable inputs of its first event (observation rows, station
// coordinates) are loaded once per launch and stay in registers.  Hand-off in both directions by tagged
// granules (data is the flag); chain state is read with agent-scope loads after the job word has been seen
// (the master drained its stores before publishing it).  Leaves when the master has finished (PSync::quit)
// or after a bounded wait.
// NWV = waves per worker block (8: the master's block shape).  PIPE: the launch's master is the pipelined one (htm_pipe.hpp), whose
// orders name a second left-out event and want the left-out events' sums reported on their own -- compiled only into those
// launches: in the workers' event loop it costs the others 13 % at 10 000 x 128 x 16 fp64 (profiles/r04_h_worker_pipe_ab.txt).
template <int NCH, bool F32, int NWV = 8, bool PIPE = false, int CAP = kMaxChains>
__device__ __forceinline__ void worker_body(FwRef f_, CsRef cs_, unsigned long long launch, int w)
{
    CsRef cs = rebase(cs_);
    FwRef f = rebase(f_);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *s_red = reinterpret_cast<double *>(smem);          // [NWV <= 16]
    unsigned *s_tag = reinterpret_cast<unsigned *>(smem + 128);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = cs.n_workers;
    const int nc = cs.n_chains;
    const int ev0 = w * NWV + wave;

    constexpr int N = NCH > 0 ? NCH : 1;
    StaRegs<N> st;
    ObsRegs<N, F32> ob0;
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int j = lane + 64 * c;
            const bool valid = j < f.S;
            st.sx[c] = valid ? f.sx[j] : 0.0; st.sy[c] = valid ? f.sy[j] : 0.0; st.sz[c] = valid ? f.sz[j] : 0.0;
            st.tc[c] = 0.0; st.ac[c] = 0.0;
        }
        if (ev0 < f.E) load_obs_regs<NCH, F32>(ob0, f, ev0, lane);
    }

    int *s_chain = reinterpret_cast<int *>(smem + 136);
    // wave 0: lane 8k + g holds granule g of chain (8 j + k)'s slot; lane 8k remembers the last tag served
    constexpr int kGroups = (CAP + 7) / 8;
    unsigned last_tag[kGroups];
#pragma unroll
    for (int j = 0; j < kGroups; ++j) last_tag[j] = 0;
    // An order whose named commit does not show within kDeferTicks is put aside -- its tag stays in last_tag, so the polls
    // skip it -- and becomes eligible again kDeferTicks later (if the slot still holds it): a wait that the master's
    // signals should have ended (void_slot) must never keep the worker from the other chains' orders.
    constexpr unsigned long long kDeferTicks = 2000ull;       // 20 us of the 100 MHz clock; legitimate waits are a few us
    // (kept in LDS, wave 0 only: scalar registers are what this kernel is short of)
    int *s_defer_chain = reinterpret_cast<int *>(smem + 192);
    unsigned long long *s_defer_until = reinterpret_cast<unsigned long long *>(smem + 200);
    if (threadIdx.x == 0) { *s_defer_chain = -1; *s_defer_until = 0ull; }
    // [0] type | idx << 3, [1] x_new high, [2] x_new low, [3] committed element or ~0, [4] its value high, [5] low,
    // [6] element (+1) whose value, as seen by this evaluation, is to be reported (two-ahead orders), 0 = none
    unsigned *s_job = reinterpret_cast<unsigned *>(smem + 160);
    const unsigned long long *slots = cs.slots + (size_t)(w % cs.slot_rep) * cs.slot_stride;
    const int npoll = cs.npoll;
    for (;;) {
        if (wave == 0) {
            unsigned tag = 0;
            int chain = -1;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
            // one poll = the slots of all chains (one load per 8 chains) + the quit word; npoll polls in flight
            constexpr int kPolls = 3;
            unsigned long long x[kPolls][kGroups], qw[kPolls];
            auto issue = [&](int b) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < kGroups; ++j) {
                    x[b][j] = 0ull;
                    if (8 * j < nc && 8 * j + (lane >> 3) < nc) x[b][j] = ld_agent(slots + (size_t)(8 * j) * kGranPerSlot + lane);
                }
                qw[b] = lane == 63 ? ld_agent(&cs.ps->quit) : 0ull;
            };
            // returns 1: an order was taken (tag, chain, s_job set), -1: the master has quit, 0: nothing yet
            auto check = [&](int b) __attribute__((always_inline)) -> int {
#pragma unroll
                for (int j = 0; j < kGroups; ++j) {
                    if (8 * j >= nc) continue;
                    const unsigned t = (unsigned)(x[b][j] >> 32), pay = (unsigned)x[b][j];
                    const unsigned tq = (unsigned)__builtin_amdgcn_update_dpp(0, (int)t, 0x00, 0xF, 0xF, false);    // quad_perm [0,0,0,0]
                    const unsigned t4 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)t, 0x114, 0xF, 0xF, false);   // row_shr:4
                    bool ok = t == tq && t != 0u && 8 * j + (lane >> 3) < nc;
                    if ((lane & 7) == 4) ok = ok && t == t4;                 // second quad agrees with the first
                    if ((lane & 7) == 0) ok = ok && pay == (unsigned)launch && t != last_tag[j];
                    unsigned long long m = __ballot(ok);
                    m &= m >> 1; m &= m >> 2; m &= m >> 4; m &= 0x0101010101010101ull;
                    if (m) {
                        const int l0 = __ffsll((long long)m) - 1;           // lane of granule 0 of the chosen chain
                        chain = 8 * j + (l0 >> 3);
                        tag = (unsigned)__builtin_amdgcn_readlane((int)t, l0);
                        if (lane == l0) last_tag[j] = tag;
                        unsigned pv[7];
#pragma unroll
                        for (int q = 0; q < 7; ++q) pv[q] = (unsigned)__builtin_amdgcn_readlane((int)pay, l0 + 1 + q);
                        if (lane == 0) {
#pragma unroll
                            for (int q = 0; q < 7; ++q) s_job[q] = pv[q];
                        }
                        return 1;
                    }
                }
                const unsigned qlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)qw[b], 63);
                const unsigned qhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(qw[b] >> 32), 63);
                return ((((unsigned long long)qhi << 32) | qlo) > launch) ? -1 : 0;
            };
#pragma unroll
            for (int b = 0; b < kPolls; ++b) if (b < npoll) issue(b);
            auto rearm = [&](int dc) __attribute__((always_inline)) {       // the order put aside may be taken again
#pragma unroll
                for (int j = 0; j < kGroups; ++j)
                    if (j == (dc >> 3) && lane == 8 * (dc & 7)) last_tag[j] = 0;
                if (lane == 0) *s_defer_chain = -1;
            };
            for (bool spin = true; spin;) {
                {
                    const int dc = *s_defer_chain;
                    if (__builtin_expect(dc >= 0, 0)) { if (__builtin_amdgcn_s_memrealtime() > *s_defer_until) rearm(dc); }
                }
#pragma unroll
                for (int b = 0; b < kPolls; ++b) {
                    if (b >= npoll) continue;
#ifdef HTM_STAMPS
                    if (cs.stamps && w == 0 && lane == 0) cs.stamps[27] += 1;      // polls of worker 0
#endif
                    int r = spin ? check(b) : 0;
                    if (r == 1 && s_job[3] != 0xffffffffu) {
                        // The order was sent ahead of the chain's latest commit: wait until that store is what memory returns
                        // (the other waves read the chain's state only after this wave has seen it).  If the master takes the
                        // order back meanwhile -- the chain repeated a pass and rewrote the element, so the value never shows --
                        // it says so by rewriting the slot (void_slot, or a newer order): the order is dropped and the worker
                        // keeps polling.  A wait that lasts longer than any commit takes to land puts the order ASIDE for a while
                        // (kDeferTicks): it is neither dropped nor answered on the clock's say-so, the worker merely serves the other
                        // chains' orders meanwhile and looks again later.  The further bounds are fail-stops (master gone, 30 s).
                        const unsigned long long want = ((unsigned long long)s_job[4] << 32) | s_job[5];
                        const unsigned long long tw0 = __builtin_amdgcn_s_memrealtime();
                        for (unsigned spins = 0;; ++spins) {
                            if ((unsigned long long)__double_as_longlong(ld_agent(cs.xall + s_job[3])) == want) break;
                            const unsigned now_tag = (unsigned)(ld_agent(slots + (size_t)chain * kGranPerSlot) >> 32);
                            if (now_tag != tag) {
#ifdef HTM_STAMPS
                                if (lane == 0 && w == 0 && cs.stamps) {
                                    cs.stamps[112] += 1; cs.stamps[113] = chain; cs.stamps[114] = tag; cs.stamps[115] = s_job[3]; cs.stamps[116] = want;
                                    cs.stamps[117] = (unsigned long long)__double_as_longlong(ld_agent(cs.xall + s_job[3])); cs.stamps[118] = s_job[0]; cs.stamps[119] = now_tag;
                                }
#endif
                                r = 0; tag = 0; chain = -1;      // taken back: keep polling
                                break;
                            }
                            if ((spins & 7u) == 7u && __builtin_amdgcn_s_memrealtime() - tw0 > kDeferTicks) {
                                // not now: back to the polls, this order aside (it stays in last_tag until it is re-armed)
                                if (w == 0 && lane == 0) cs.diag[24] += 1;          // (reported with error -8)
                                { const int dc = *s_defer_chain; if (dc >= 0) rearm(dc); }
                                if (lane == 0) { *s_defer_chain = chain; *s_defer_until = __builtin_amdgcn_s_memrealtime() + kDeferTicks; }
                                r = 0; tag = 0; chain = -1;
                                break;
                            }
                            if ((spins & 63u) == 63u) {          // fail-stops only
                                if (w == 0 && lane == 0 && cs.diag[16] == 0 && __builtin_amdgcn_s_memrealtime() - t0 > 100000000ull) {
                                    // a second in this wait: leave a note for the host's error message (once)
                                    unsigned long long *dg = cs.diag;
                                    dg[17] = chain; dg[18] = tag; dg[19] = s_job[3]; dg[20] = want;
                                    dg[21] = (unsigned long long)__double_as_longlong(ld_agent(cs.xall + s_job[3])); dg[22] = s_job[0]; dg[23] = s_job[6];
                                    dg[16] = 1;
                                }
                                if (ld_agent(&cs.ps->quit) > launch) { r = -1; tag = 0; chain = -1; break; }
                                if (__builtin_amdgcn_s_memrealtime() - t0 > 3000000000ull) { r = -1; tag = 0; chain = -1; break; }
                            }
                            __builtin_amdgcn_s_sleep(1);
                        }
                    }
                    if (r != 0) spin = false;
                    if (spin) issue(b);
                }
                if (spin && __builtin_amdgcn_s_memrealtime() - t0 > 3000000000ull) spin = false;   // never spin forever (30 s)
            }
            if (lane == 0) { *s_tag = tag; *s_chain = chain; }
        }
        __syncthreads();
        const unsigned tag = *s_tag;
        const int m = *s_chain;
        if (tag == 0) return;
#ifdef HTM_STAMPS
        const bool wstamp = cs.stamps && w == 0 && tid == 0;
        if (wstamp) cs.stamps[21] += __builtin_amdgcn_s_memrealtime();
#endif
        {
            // (bit 31 of the order word: an order of the pipelined master, htm_pipe.hpp -- no commit is named, and the word after
            // it names a SECOND event the workers leave out)
            const bool pipe_order = PIPE && (s_job[0] >> 31) != 0u;
            const int type = (int)(s_job[0] & 7u), idx = (int)((s_job[0] & 0x7fffffffu) >> 3);
            const double ov_val = __longlong_as_double((long long)(((unsigned long long)s_job[1] << 32) | s_job[2]));
            // vs and qs of the evaluated model: chain state unless they are the proposal (same round of loads as
            // the corrections and the event coordinates below)
            const GroupOff go = group_offsets(cs);
            const double beta_c = ld_agent(cs.xall + m), q_c = ld_agent(cs.xall + go.qs + m);
            const double beta = type == 1 ? ov_val : beta_c, q = type == 3 ? ov_val : q_c;
            // (once per order, not once per event: cls_forward.f90:118, :204 divide per station; event_misfit multiplies)
            const double rbeta_j = 1.0 / beta, katt_j = (kPi * kFreq) / (q * beta);
            int ov_kind = 0, ov_idx = -1, ov_evt = -1, ov_cmp = 0;
            const int r_off = (int)s_job[6] - 1 - (go.hy + m * go.nh);
            const int r_evt = s_job[6] ? r_off / 3 : -1;       // two-ahead orders: the event left to the chain's own wave
            const int r_off2 = (int)s_job[4] - 1 - (go.hy + m * go.nh);
            const int r_evt2 = (pipe_order && s_job[4]) ? r_off2 / 3 : -1;
            // An order of the pipelined master: the wave that holds a left-out event evaluates it at BOTH candidate positions --
            // where the state has it, and with the component that the hypocentre step in between proposes (its value comes in
            // tagged granules beside the order) -- under this order's parameters, and reports the two sums on their own: the
            // master adds the one that step's decision selects (htm_pipe.hpp).
            unsigned long long lgv0 = 0, lgv1 = 0, lgv2 = 0, lgv3 = 0;
            if (pipe_order && (r_evt >= 0 || r_evt2 >= 0)) {
                const unsigned long long *lgi = cs.lo_gran + (size_t)m * 16;
                lgv0 = ld_agent(lgi); lgv1 = ld_agent(lgi + 1); lgv2 = ld_agent(lgi + 2); lgv3 = ld_agent(lgi + 3);
            }
            auto leftout = [&](const auto &ob_, double x, double y, double z, int e, const auto &st_, double rb_, double ka_) __attribute__((always_inline)) {
                if constexpr (NCH > 0) {
                    const int k = (e == r_evt) ? 0 : 1;
                    const int cmpk = k == 0 ? r_off - 3 * r_evt : r_off2 - 3 * r_evt2;
                    unsigned long long *lg = cs.lo_gran + (size_t)m * 16;
                    unsigned long long a = k == 0 ? lgv0 : lgv2, b = k == 0 ? lgv1 : lgv3;      // (requested with the order's state loads)
                    for (unsigned spins = 0; spins < (1u << 22); ++spins) {
                        if ((unsigned)(a >> 32) == tag && (unsigned)(b >> 32) == tag) break;
                        __builtin_amdgcn_s_sleep(1);
                        a = ld_agent(lg + 2 * k); b = ld_agent(lg + 2 * k + 1);
                    }
                    if ((unsigned)(a >> 32) != tag || (unsigned)(b >> 32) != tag) return;      // (never seen: the master's collector reports the unanswered order)
                    const double xn = gran_f64(a, b);
                    const double px[2] = {x, cmpk == 0 ? xn : x};
                    const double py[2] = {y, cmpk == 1 ? xn : y};
                    const double pz[2] = {z, cmpk == 2 ? xn : z};
                    double o2[2];
                    event_misfit<(NCH > 0 ? NCH : 1), 2, F32, true>(f, ob_, lane, st_, px, py, pz, rb_, ka_, o2);
                    wave_sum<2>(o2);
                    if (lane == 0) { st_gran_f64(lg + 8 + 4 * k, tag, o2[0]); st_gran_f64(lg + 8 + 4 * k + 2, tag, o2[1]); }
                }
            };
            if (type == 2 || type == 4) { ov_kind = type; ov_idx = idx; }
            else if (type >= 5) { ov_evt = idx / 3; ov_cmp = idx - 3 * ov_evt; }
            const double *hyp = cs.xall + go.hy + (size_t)m * go.nh;
            const double *tc = cs.xall + go.tc + (size_t)m * cs.S, *ac = cs.xall + go.ac + (size_t)m * cs.S;
            double lane_acc = 0.0;
            if constexpr (NCH > 0) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {                 // chain state: agent-scope loads
                    const int j = lane + 64 * c;
                    const bool valid = j < f.S;
                    st.tc[c] = valid ? ld_agent(tc + j) : 0.0;
                    st.ac[c] = valid ? ld_agent(ac + j) : 0.0;
                    if (valid && ov_idx == j) { if (ov_kind == 2) st.tc[c] = ov_val; if (ov_kind == 4) st.ac[c] = ov_val; }
                }
                if constexpr (!F32) {
                    // Events ev0, ev0 + 8W, ...: the first one's observation rows are resident (ob0); every further event's
                    // rows and coordinates are requested BEFORE the current event is evaluated (software pipeline, one
                    // event of look-ahead).  fp64: an event's arithmetic covers the next one's loads, the deeper form below
                    // measured -1 % at 1 000 and 10 000 events x 64 stations, and two stations per lane do not fit the 256
                    // registers of a wave with three buffers.
                    const bool full_rows64 = f.S == 64 * NCH && f.use_time != 0 && f.use_amp != 0;      // (loads without selects or branches)
                    ObsRegs<NCH, F32> ob_cur = ob0, ob_nxt = ob0;
                    double cx = 0.0, cy = 0.0, cz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
                    if (ev0 < f.E) { cx = ld_agent(hyp + 3 * ev0); cy = ld_agent(hyp + 3 * ev0 + 1); cz = ld_agent(hyp + 3 * ev0 + 2); }
                    for (int ev = ev0; ev < f.E; ev += NWV * W) {
                        const int evn = ev + NWV * W;
                        if (evn < f.E) {
                            if (full_rows64) load_obs_regs_nobranch<NCH, F32, HTM_NT_WORKERS != 0, HTM_VRPS_WORKERS != 0, true>(ob_nxt, f, evn, lane);
                            else load_obs_regs<NCH, F32, HTM_NT_WORKERS != 0, HTM_VRPS_WORKERS != 0>(ob_nxt, f, evn, lane);
                            nx = ld_agent(hyp + 3 * evn); ny = ld_agent(hyp + 3 * evn + 1); nz = ld_agent(hyp + 3 * evn + 2);
                        }
                        double ex = cx, ey = cy, ez = cz;      // (the proposed component of a first-iteration order: a rare branch)
                        if (__builtin_expect(ev == ov_evt, 0)) { ex = ov_cmp == 0 ? ov_val : cx; ey = ov_cmp == 1 ? ov_val : cy; ez = ov_cmp == 2 ? ov_val : cz; }
                        const double px[1] = {ex};
                        const double py[1] = {ey};
                        const double pz[1] = {ez};
                        double out[1];
                        if (__builtin_expect(pipe_order && (ev == r_evt || ev == r_evt2), 0)) leftout(ob_cur, cx, cy, cz, ev, st, rbeta_j, katt_j);
                        else {
                            event_misfit<NCH, 1, F32, true>(f, ob_cur, lane, st, px, py, pz, rbeta_j, katt_j, out);
                            // two-ahead order: the event of the step in between is left to the chain's own wave (it may be mid-commit)
                            lane_acc += (ev == r_evt) ? 0.0 : out[0];
                        }
                        ob_cur = ob_nxt; cx = nx; cy = ny; cz = nz;
                    }
                } else {
                    // Events ev0, ev0 + 8W, ...: the first one's observation rows are resident (ob0).  Three register buffers in
                    // rotation: the rows and coordinates of the event TWO places ahead are requested before the current event is
                    // evaluated, with a fixed number of loads per request (load_obs_regs_nobranch), so that at E >> 8W two
                    // events' loads fly under the arithmetic of a third: the fp32 forward's arithmetic is too short to cover an
                    // event's loads (configs[4] shape: 837 -> 902 k steps/s).  The last <= 4 events of a wave take the plain path.
                    const int s8 = NWV * W;
                    ObsRegs<NCH, F32> b0 = ob0, b1 = ob0, b2 = ob0;
                    double x0 = 0.0, y0 = 0.0, z0 = 0.0, x1 = 0.0, y1 = 0.0, z1 = 0.0, x2 = 0.0, y2 = 0.0, z2 = 0.0;
                    // (every lane has a station in both chunks and both data types are used: the loads need no selects)
                    const bool full_rows = (f.S & 63) == 0 && f.S == 64 * NCH && f.use_time != 0 && f.use_amp != 0;
                    auto fetch = [&](ObsRegs<NCH, F32> &b, double &x, double &y, double &z, int e) __attribute__((always_inline)) {
                        if (full_rows) load_obs_regs_nobranch<NCH, F32, HTM_NT_WORKERS != 0, HTM_VRPS_WORKERS != 0, true>(b, f, e, lane);
                        else load_obs_regs_nobranch<NCH, F32, HTM_NT_WORKERS != 0, HTM_VRPS_WORKERS != 0>(b, f, e, lane);
                        x = ld_agent(hyp + 3 * e); y = ld_agent(hyp + 3 * e + 1); z = ld_agent(hyp + 3 * e + 2);
                    };
                    auto eval = [&](const ObsRegs<NCH, F32> &b, double x, double y, double z, int e) __attribute__((always_inline)) {
                        // (the proposed hypocentre component of an order of the first iteration: a rare branch, not three selects per event)
                        double ex = x, ey = y, ez = z;
                        if (__builtin_expect(e == ov_evt, 0)) { ex = ov_cmp == 0 ? ov_val : x; ey = ov_cmp == 1 ? ov_val : y; ez = ov_cmp == 2 ? ov_val : z; }
                        const double px[1] = {ex};
                        const double py[1] = {ey};
                        const double pz[1] = {ez};
                        double out[1];
                        if (__builtin_expect(pipe_order && (e == r_evt || e == r_evt2), 0)) leftout(b, x, y, z, e, st, rbeta_j, katt_j);
                        else {
                            event_misfit<NCH, 1, F32, true>(f, b, lane, st, px, py, pz, rbeta_j, katt_j, out);
                            // two-ahead order: the event of the step in between is left to the chain's own wave (it may be mid-commit)
                            lane_acc += (e == r_evt) ? 0.0 : out[0];
                        }
                    };
                    int ev = ev0;
                    if (ev < f.E) {
                        x0 = ld_agent(hyp + 3 * ev); y0 = ld_agent(hyp + 3 * ev + 1); z0 = ld_agent(hyp + 3 * ev + 2);
                        if (ev + s8 < f.E) fetch(b1, x1, y1, z1, ev + s8);
                    }
                    while (ev + 4 * s8 < f.E) {            // b0 <- event ev, b1 <- ev + s8 on entry and again after the trip
                        fetch(b2, x2, y2, z2, ev + 2 * s8); eval(b0, x0, y0, z0, ev);
                        fetch(b0, x0, y0, z0, ev + 3 * s8); eval(b1, x1, y1, z1, ev + s8);
                        fetch(b1, x1, y1, z1, ev + 4 * s8); eval(b2, x2, y2, z2, ev + 2 * s8);
                        ev += 3 * s8;
                    }
                    if (ev < f.E) { if (ev + 2 * s8 < f.E) fetch(b2, x2, y2, z2, ev + 2 * s8); eval(b0, x0, y0, z0, ev); }
                    if (ev + s8 < f.E) { if (ev + 3 * s8 < f.E) fetch(b0, x0, y0, z0, ev + 3 * s8); eval(b1, x1, y1, z1, ev + s8); }
                    if (ev + 2 * s8 < f.E) eval(b2, x2, y2, z2, ev + 2 * s8);
                    if (ev + 3 * s8 < f.E) eval(b0, x0, y0, z0, ev + 3 * s8);
                }
            } else {
                // generic station count: corrections are read through plain loads after an agent acquire
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                for (int ev = ev0; ev < f.E; ev += NWV * W) {
                    const bool ov = ev == ov_evt;
                    const double hx = ld_agent(hyp + 3 * ev), hy = ld_agent(hyp + 3 * ev + 1), hz = ld_agent(hyp + 3 * ev + 2);
                    const double px[1] = {(ov && ov_cmp == 0) ? ov_val : hx};
                    const double py[1] = {(ov && ov_cmp == 1) ? ov_val : hy};
                    const double pz[1] = {(ov && ov_cmp == 2) ? ov_val : hz};
                    double out[1];
                    event_misfit_generic<1>(f, ev, lane, f.sx, f.sy, f.sz, tc, ac, ov_kind, ov_idx, ov_val, px, py, pz,
                                            beta, q, out);
                    lane_acc += out[0];
                }
            }
            const double tot = wave_sum1(lane_acc);
#ifdef HTM_STAMPS
            if (wstamp) cs.stamps[22] += __builtin_amdgcn_s_memrealtime();
#endif
            if (lane == 0) s_red[wave] = tot;
            __syncthreads();
#ifdef HTM_STAMPS
            if (wstamp) cs.stamps[23] += __builtin_amdgcn_s_memrealtime();
#endif
            if (tid == 0) {
                double tot8 = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) + ((s_red[4] + s_red[5]) + (s_red[6] + s_red[7]));
                if constexpr (NWV == 12) tot8 = tot8 + ((s_red[8] + s_red[9]) + (s_red[10] + s_red[11]));
                st_gran_f64(cs.pgran + ((size_t)m * cs.n_wg + w) * cs.pgran_stride, tag, tot8);
            }
            __syncthreads();
        }
    }
}

}  // namespace htm
