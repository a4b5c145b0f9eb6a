// htm_forward_kernels.hpp -- the non-template kernels of the forward unit: k_sum_partials and k_syn (see htm_kernels.hpp) and the
// self-test kernels.  A non-template kernel defined in a header gives every unit that includes it a host stub and a copy of
// the device code of its own, so exactly ONE unit includes this file: htm_forward.hip.
#pragma once
#include "htm_kernels.hpp"
#include "htm_handoff.hpp"

namespace htm {

// L[m] = -(sum of partials) - const_sum, fixed summation order (lane-strided, then the DPP tree)
__global__ __launch_bounds__(64) void k_sum_partials(const double *partial, int n_wg, double const_sum,
                                                     double *L)
{
    const int m = blockIdx.x, lane = threadIdx.x;
    double acc = 0.0;
    for (int k = lane; k < n_wg; k += 64) acc += partial[(size_t)m * n_wg + k];
    const double tot = wave_sum1(acc);
    if (lane == 0) L[m] = -tot - const_sum;
}

// ---------------------------------------------------------------------------------------------------
// calc_travel_time / calc_amp (+ _single): writes the demeaned synthetics.  wave <-> event.
// which: 0 = travel time, 1 = amplitude.  ev_only >= 0 restricts to one event and writes out[0..S).
__global__ __launch_bounds__(256) void k_syn(FwdDev f, const double *hypo, const double *corr, double beta,
                                             double q, int which, int ev_only, double *out)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int ev = blockIdx.x * 4 + wave;
    if (ev_only >= 0) { if (ev != 0) return; ev = ev_only; }
    if (ev >= f.E) return;
    const double x = hypo[3 * ev], y = hypo[3 * ev + 1], z = hypo[3 * ev + 2];
    const double *obs = which == 0 ? f.t_obs : f.a_obs;
    const double *prec = which == 0 ? f.t_prec : f.a_prec;
    const double psum = which == 0 ? f.psum_t[ev] : f.psum_a[ev];
    const size_t base = (size_t)ev * f.S;
    const double qbeta = q * beta;
    double acc = 0.0;
    for (int j = lane; j < f.S; j += 64) {
        const double dx = x - f.sx[j], dy = y - f.sy[j], dz = z - f.sz[j];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        const double s = which == 0 ? d / beta - corr[j] : -(d * kPi * kFreq / qbeta) - htm_log(d) - corr[j];
        acc += prec[base + j] * (s - obs[base + j]);
    }
    const double mean = wave_sum1(acc) / psum;
    double *o = ev_only >= 0 ? out : out + base;
    for (int j = lane; j < f.S; j += 64) {
        const double dx = x - f.sx[j], dy = y - f.sy[j], dz = z - f.sz[j];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        const double s = which == 0 ? d / beta - corr[j] : -(d * kPi * kFreq / qbeta) - htm_log(d) - corr[j];
        o[j] = s - mean;
    }
}

// ---------------------------------------------------------------------------------------------------
// self-test: DPP wave_sum against a serial loop of the same tree order; device RNG against host values
// ---------------------------------------------------------------------------------------------------
// htm_selftest_math: the forward model's own logarithm / square root (htm_device.hpp) on n arbitrary arguments
__global__ void k_mathtest(int which, const double *x, double *y, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (which == 4) {            // the matrix-pipe wave sum: every lane's result for its wave's 64 values (n a multiple of 64)
        if (i < n) y[i] = wave_sum_mfma(x[i]);
        return;
    }
    if (which == 5 || which == 6) {     // four sums per wave at once (5, wave_sum<4>) and one by one (6): x = four blocks of n / 4 values
        const int q = n / 4;
        if (i < q) {
            double v[4] = {x[i], x[q + i], x[2 * q + i], x[3 * q + i]};
            if (which == 5) wave_sum<4>(v);
            else { for (int k = 0; k < 4; ++k) v[k] = wave_sum1(v[k]); }
            for (int k = 0; k < 4; ++k) y[k * q + i] = v[k];
        }
        return;
    }
    if (which == 7) {            // htm_log with its constants in registers (LogRegs), against mode 0 bit for bit
        const LogRegs lg = log_regs();
        if (i < n) y[i] = htm_log(x[i], lg);
        return;
    }
    if (which == 8 || which == 9) {     // the transposed sum with the lane classes in registers (SumRegs): four values at once (8), two
        const SumRegs sm = sum_regs();  // pairs (9); against mode 6.  x = four blocks of n / 4 values, n / 4 a multiple of 64: whole waves
        const int q = n / 4;
        if (i < q) {
            double v[4] = {x[i], x[q + i], x[2 * q + i], x[3 * q + i]};
            if (which == 8) wave_sum_transposed<4>(v, sm);
            else {
                double a[2] = {v[0], v[1]}, b[2] = {v[2], v[3]};
                wave_sum_transposed<2>(a, sm); wave_sum_transposed<2>(b, sm);
                v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
            }
            for (int k = 0; k < 4; ++k) y[k * q + i] = v[k];
        }
        return;
    }
    if (i < n) y[i] = which == 0 ? htm_log(x[i]) : which == 1 ? htm_sqrt(x[i]) : which == 2 ? sqrt(x[i]) : log(x[i]);   // 3: the device library's log (Rayleigh prior ratio, htm_step.hpp)
}

__global__ void k_selftest(const double *in, double *out_dpp, double *out_ref, uint32_t *rng_out,
                           double *rng_d)
{
    const int lane = threadIdx.x;
    {   // DPP inclusive scan vs a serial prefix sum (draw counts are 3..6, use a wider spread)
        const int v = 3 + ((lane * 7 + 1) % 5);
        const int sc = wave_incl_scan(v);
        int ref = 0;
        for (int i = 0; i <= lane; ++i) ref += 3 + ((i * 7 + 1) % 5);
        const unsigned long long bad = __ballot(sc != ref);
        if (lane == 0) rng_d[9] = bad ? 1.0 : 0.0;
    }
    double v[2] = {in[lane], in[64 + lane]};
    wave_sum<2>(v);
    if (lane == 0) {
        out_dpp[0] = v[0]; out_dpp[1] = v[1];
        for (int s = 0; s < 2; ++s) {   // same association as wave_sum's
            double t[64];
            for (int i = 0; i < 64; ++i) t[i] = in[64 * s + i];
            if (HTM_MFMA_SUM != 0) {     // the matrix instruction adds its four products in order of k, from zero
                double S[16], G[4];
                for (int i = 0; i < 16; ++i) S[i] = ((t[i] + t[i + 16]) + t[i + 32]) + t[i + 48];
                for (int g = 0; g < 4; ++g) G[g] = (S[g] + S[g + 4]) + (S[g + 8] + S[g + 12]);
                out_ref[s] = ((G[0] + G[1]) + G[2]) + G[3];
                continue;
            }
            double q[16];
            for (int i = 0; i < 16; ++i) q[i] = (t[4 * i] + t[4 * i + 1]) + (t[4 * i + 2] + t[4 * i + 3]);
            double r[4];
            for (int i = 0; i < 4; ++i) r[i] = (q[4 * i] + q[4 * i + 1]) + (q[4 * i + 2] + q[4 * i + 3]);
            out_ref[s] = (r[3] + r[2]) + (r[1] + r[0]);
        }
        uint32_t x = 0x4b88a366u, y = 0x1b11733cu, z = 0x097044b6u, w = 0x00676ea2u;  // rank-0 seed state
        for (int i = 0; i < 8; ++i) { rng_out[i] = xs128_next(x, y, z, w); rng_d[i] = u_of(rng_out[i]); }
        rng_d[8] = g_of(rng_out[0], rng_out[1]);
    }
}

}  // namespace htm
