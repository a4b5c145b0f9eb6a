// htm_stream.hpp -- producers of the rank's random stream (run on a side stream, ahead of k_step).
//
// mod_random (reference src/mod_random.f90) is one serial xorshift128 stream per rank, consumed in an order
// that depends on chain state only through HOW MANY draws each chain step takes.  The values themselves,
// and everything derived from a value at a given stream position, are independent of the chains.  So the
// stream is produced ahead of time:
//   k_rawgen       the recurrence itself, in parallel: xorshift128 is GF(2)-linear, so every lane jumps to the start
//                  of its own 64-draw segment with precomputed powers of the transition matrix
//   k_stream_tr    per position: rand_u, log(rand_u), the Box-Muller value that starts there
//   k_stream_rec   per position: the chain step that would START there, decoded (proposal type, element,
//                  event, draws consumed) with its Gaussian and its Metropolis draw
//   k_stream_hop   per position: where the 1st..8th following chain step starts (optimistic)
// k_step only copies a window of these rings into LDS and follows them.
#pragma once
#include "htm_device.hpp"

namespace htm {

constexpr int kHops = 8;          // hop tables cover 1..8 chain steps (k_step has at most 8 chain waves)
constexpr int kRecLag = 16;       // a record at p reads transforms up to p+5, a swap plan up to p+13
constexpr int kHopLag = 6 * kHops;

// ---- the recurrence itself, in parallel by jump-ahead ---------------------------------------------------------
// xorshift128 (mod_random.f90:63-71) is linear over GF(2): one step is state' = T * state for a fixed 128 x 128 bit
// matrix T (state = x | y << 32 | z << 64 | w << 96).  The host precomputes J[b] = T^(64 * 2^b) (htm_jump_table),
// stored as 128 columns of 4 words.  Segment g of 64 draws starts from  T^(64 g) * s0 = prod_{bits b of g} J[b] * s0,
// so every LANE can start its own segment: a wave produces 64 segments = 4 096 consecutive draws, transposes them
// through LDS and writes them with coalesced 256-B stores.  Bit-identical to the serial stream by construction.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // one matrix column
constexpr int kJumpLevels = 20;       // segments per call < 2^20 (ring capacity <= 2^24 positions)

__device__ __forceinline__ void jump_apply(uint32_t (&s)[4], const u32x4 *J)
{
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int wd = 0; wd < 4; ++wd) {
        const uint32_t v = s[wd];
#pragma unroll 8
        for (int bit = 0; bit < 32; ++bit) {
            const u32x4 col = ld_const(J + wd * 32 + bit);           // wave-uniform: scalar load
            const uint32_t m = 0u - ((v >> bit) & 1u);
            a0 ^= col.x & m; a1 ^= col.y & m; a2 ^= col.z & m; a3 ^= col.w & m;
        }
    }
    s[0] = a0; s[1] = a1; s[2] = a2; s[3] = a3;
}

// The kernels themselves are defined in htm_chains_kernels.hpp, which one unit includes.  These two are launched from the
// self-test's unit as well:
// grid = ceil(n / 4096) workgroups of ONE wave; n a multiple of 64.  gen_in: state after the last produced draw
// (read by every wave); gen_out: the state after this call's last draw (a different buffer: no race with the readers).
__global__ void k_rawgen(StreamDev sd, long long start, int n, const u32x4 *jump, const uint32_t *gen_in, uint32_t *gen_out);
// the same stream drawn serially by one lane (htm_selftest compares the two)
__global__ void k_rawgen_serial(uint32_t *out, int n, const uint32_t *gen_in, uint32_t *gen_out);


}  // namespace htm
