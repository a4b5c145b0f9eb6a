// htm_chains_kernels.hpp -- the small non-template kernels around the chain loops: the producers of the random stream
// (types and device helpers: htm_stream.hpp), the set-up of a launch with several master workgroups (htm_flow.hpp: MbShared and
// its MW_* words are defined there) and the probe of the peer-mapped inboxes (htm_handoff.hpp).  A non-template kernel defined in a header gives every unit that includes it
// a host stub and a copy of the device code of its own, so exactly ONE unit includes this file: htm_chains_run.hip.
#pragma once
#include "htm_flow.hpp"

namespace htm {

// ---- htm_stream.hpp: the producers ------------------------------------------------------------------------------------
// grid = ceil(n / 4096) workgroups of ONE wave; n a multiple of 64.  gen_in: state after the last produced draw
// (read by every wave); gen_out: the state after this call's last draw (a different buffer: no race with the readers).
__global__ __launch_bounds__(64) void k_rawgen(StreamDev sd, long long start, int n, const u32x4 *jump,
                                               const uint32_t *gen_in, uint32_t *gen_out)
{
    __shared__ uint32_t tile[64 * 65];
    const int lane = threadIdx.x;
    const int n_seg = n >> 6;
    const int g = blockIdx.x * 64 + lane;                 // this lane's segment
    uint32_t s[4] = {gen_in[0], gen_in[1], gen_in[2], gen_in[3]};
    // bits 6.. of g are uniform over the wave (scalar branch), bits 0..5 differ by lane (predicated)
    for (int b = 6; b < kJumpLevels; ++b)
        if ((blockIdx.x >> (b - 6)) & 1) jump_apply(s, jump + (size_t)b * 128);
    for (int b = 0; b < 6; ++b) {
        uint32_t t[4] = {s[0], s[1], s[2], s[3]};
        jump_apply(t, jump + (size_t)b * 128);
        if ((lane >> b) & 1) { s[0] = t[0]; s[1] = t[1]; s[2] = t[2]; s[3] = t[3]; }
    }
    uint32_t x = s[0], y = s[1], z = s[2], w = s[3];
#pragma unroll
    for (int k = 0; k < 64; ++k) tile[lane * 65 + k] = xs128_next(x, y, z, w);
    if (g == n_seg - 1) { gen_out[0] = x; gen_out[1] = y; gen_out[2] = z; gen_out[3] = w; }
    __syncthreads();
    const int seg0 = blockIdx.x * 64;
    for (int k = 0; k < 64 && seg0 + k < n_seg; ++k)
        sd.raw[(start + (long long)(seg0 + k) * 64 + lane) & sd.mask] = tile[k * 65 + lane];
}

// the same stream drawn serially by one lane (htm_selftest compares the two)
__global__ void k_rawgen_serial(uint32_t *out, int n, const uint32_t *gen_in, uint32_t *gen_out)
{
    uint32_t x = gen_in[0], y = gen_in[1], z = gen_in[2], w = gen_in[3];
    for (int k = 0; k < n; ++k) out[k] = xs128_next(x, y, z, w);
    gen_out[0] = x; gen_out[1] = y; gen_out[2] = z; gen_out[3] = w;
}

__global__ __launch_bounds__(256) void k_stream_tr(StreamDev sd, long long start, long long end)
{
    const long long p = start + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    const uint32_t r0 = sd.raw[p & sd.mask], r1 = sd.raw[(p + 1) & sd.mask];
    const double u = u_of(r0);
    sd.U[p & sd.mask] = u;
    sd.LOGU[p & sd.mask] = log(u);
    sd.G[p & sd.mask] = g_of(r0, r1);
}

// cls_mcmc.f90:134-165: a_select, then (id,) (icmp,) then the two draws of rand_g, then the judge's rand_u
__global__ __launch_bounds__(256) void k_stream_rec(StreamDev sd, long long start, long long end, double th1,
                                                    double th2, double th3, double th4, int S, int E,
                                                    int n_procs, int n_chains)
{
    const long long p = start + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    const long long M = sd.mask;
    const double a = sd.U[p & M], u1 = sd.U[(p + 1) & M], u2 = sd.U[(p + 2) & M];
    int type, idx, evt = -999, goff;
    if (a < th1) { type = 1; idx = 0; goff = 1; }
    else if (a < th2) { type = 2; idx = (int)(u1 * S); goff = 2; }
    else if (a < th3) { type = 3; idx = 0; goff = 1; }
    else if (a < th4) { type = 4; idx = (int)(u1 * S); goff = 2; }
    else {
        const int id = (int)(u1 * E) + 1;
        const int icmp = (int)(u2 * 3);
        idx = 3 * id - icmp - 1; type = 5 + icmp; evt = id; goff = 3;
    }
    const long long gpos = p + goff, jpos = gpos + 2;
    sd.dec[p & M] = make_int4(type, idx, evt, goff + 3);     // draws if prior_ok: ..., g(2), r
    sd.pg[p & M] = sd.G[gpos & M];
    sd.pr[p & M] = sd.U[jpos & M];
    sd.plogr[p & M] = sd.LOGU[jpos & M];
    // select_pair (cls_parallel.f90:226-230) if it started at p: i1, then i2 redrawn until it differs
    int i1 = -1, i2 = -1, used = -1;
    if (n_procs * n_chains > 1) {
        i1 = (int)(a * n_procs * n_chains);
        for (int k = 1; k <= 12; ++k) {
            i2 = (int)(sd.U[(p + k) & M] * n_procs * n_chains);
            if (i2 != i1) { used = k + 1; break; }
        }
    }
    sd.sw[p & M] = make_int4(i1, i2, used, 0);
}

__global__ __launch_bounds__(256) void k_stream_hop(StreamDev sd, long long start, long long end)
{
    const long long p = start + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    long long h = p;
#pragma unroll
    for (int k = 0; k < kHops; ++k) {
        h += sd.dec[h & sd.mask].w;
        sd.hop[(p & sd.mask) * kHops + k] = (int)(h - p);      // stored relative to p
    }
}

__global__ void k_publish(long long *dst, long long v) { *dst = v; }

// ---- htm_flow.hpp ------------------------------------------------------------------------------------------------------
// before a launch with several master workgroups (one wave): MbShared as the first step finds it
__global__ __launch_bounds__(64) void k_mb_init(ChainsDev cs, int target_arg)
{
    MbShared *g = cs.mb;
    const int lane = threadIdx.x;
    unsigned long long *w = reinterpret_cast<unsigned long long *>(g);
    for (int k = lane; k < (int)(sizeof(MbShared) / sizeof(unsigned long long)); k += 64) w[k] = 0ull;
    __syncthreads();
    for (int c = lane; c < kMaxChains; c += 64) g->prog[c] = (unsigned long long)(unsigned)c;          // key(i0, c), epoch 0, prior ok
    if (lane == 0) {
        const Ctrl c = *cs.ctrl;
        g->word[MW_LAST] = (unsigned long long)(unsigned)(target_arg >= 0 ? target_arg : c.iter_target);
        g->word[MW_NLIK] = (unsigned long long)(unsigned)c.n_lik; g->word[MW_NSMP] = (unsigned long long)(unsigned)c.n_smp;
        g->word[7] = c.jobs_total;
    }
}

// ---- htm_handoff.hpp ---------------------------------------------------------------------------------------------------
// Probe of the peer-mapped inboxes (htm_chains_xchg_probe): one wave writes a token record into every rank's inbox and
// waits (bounded, `ticks` of the 100 MHz clock) until the tokens of all ranks have arrived in its own -- the same
// stores, loads and scopes exchange_post / exchange_finish use, so a mapping whose writes are not visible to a polling kernel is
// found at set-up, not inside a run.  Token tags have the top bit set: no iteration number ever matches them.
__global__ __launch_bounds__(64) void k_xchg_probe(ChainsDev cs, unsigned token, unsigned long long ticks, int *result)
{
    const int lane = threadIdx.x, np = cs.n_procs, G = cs.xg;
    const unsigned tag = 0x80000000u | token;
    if (lane < 2)
        for (int q = 0; q < np; ++q)
            st_sys(ld_const(cs.outbox + q) + (size_t)(0 * np + cs.rank) * G + lane, ((unsigned long long)tag << 32) | (unsigned)cs.rank);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool ok = false;
    for (;;) {
        bool mine = true;
        for (int r = lane >> 1; r < np; r += 32) {
            const unsigned long long v = ld_sys(cs.inbox + (size_t)r * G + (lane & 1));
            mine = mine && (unsigned)(v >> 32) == tag && (unsigned)v == (unsigned)r;
        }
        if (__all(mine)) { ok = true; break; }
        if (__builtin_amdgcn_s_memrealtime() - t0 > ticks) break;
        __builtin_amdgcn_s_sleep(8);
    }
    if (lane == 0) *result = ok ? 1 : 0;
}

}  // namespace htm
