// htm_fft.hpp -- batched fp64 complex FFT for step 1 (htm_convert.hpp), unnormalised in both directions:
//     X[k] = sum_j x[j] exp(sign 2 pi i j k / n),   sign = -1 forward, +1 backward.
//
// Lengths whose only prime factors are 2, 3, 5 and 7 run as Stockham autosort passes, one launch per pass and one
// thread per butterfly (inputs read n/R apart, outputs written ns apart: both coalesced across neighbouring
// butterflies).  Every other length goes through Bluestein's chirp-z form with a power-of-two inner transform.
// The twiddle and chirp tables are built on the host in long double (k^2 mod 2n in 64-bit integers for the chirp),
// so their accuracy depends neither on the device libm nor on the size of the argument.  See DESIGN.md §3.5.
#pragma once
#include <hip/hip_runtime.h>

namespace htm {

constexpr long kFftMaxN = 1L << 24;     // longest transform
constexpr int kFftThreads = 256;

__device__ __forceinline__ double2 c_mul(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 c_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 c_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 c_conj(double2 a) { return make_double2(a.x, -a.y); }

// cos and sin of 2 pi m / R, m = 0 .. R-1, for the odd radices (decimal expansions to 20 digits)
template <int R> struct FftRoots;
template <> struct FftRoots<3> {
    static constexpr double c[3] = {1.0, -0.5, -0.5};
    static constexpr double s[3] = {0.0, 0.86602540378443864676, -0.86602540378443864676};
};
template <> struct FftRoots<5> {
    static constexpr double c[5] = {1.0, 0.30901699437494742410, -0.80901699437494742410, -0.80901699437494742410,
                                    0.30901699437494742410};
    static constexpr double s[5] = {0.0, 0.95105651629515357212, 0.58778525229247312917, -0.58778525229247312917,
                                    -0.95105651629515357212};
};
template <> struct FftRoots<7> {
    static constexpr double c[7] = {1.0, 0.62348980185873353053, -0.22252093395631440429, -0.90096886790241912624,
                                    -0.90096886790241912624, -0.22252093395631440429, 0.62348980185873353053};
    static constexpr double s[7] = {0.0, 0.78183148246802980871, 0.97492791218182360702, 0.43388373911755812048,
                                    -0.43388373911755812048, -0.97492791218182360702, -0.78183148246802980871};
};

// in-register DFT of R points: v[q] <- sum_r v[r] exp(sign 2 pi i q r / R)
template <int R>
__device__ __forceinline__ void fft_small(double2 *v, int sign)
{
    if constexpr (R == 2) {
        const double2 a = v[0], b = v[1];
        v[0] = c_add(a, b); v[1] = c_sub(a, b);
    } else if constexpr (R == 4) {
        const double2 a = c_add(v[0], v[2]), b = c_sub(v[0], v[2]), c = c_add(v[1], v[3]), e = c_sub(v[1], v[3]);
        const double2 d = make_double2(-sign * e.y, sign * e.x);       // (v1 - v3) * (sign i)
        v[0] = c_add(a, c); v[2] = c_sub(a, c); v[1] = c_add(b, d); v[3] = c_sub(b, d);
    } else {
        double2 o[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            double2 acc = v[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const int m = (q * r) % R;
                const double2 w = make_double2(FftRoots<R>::c[m], sign * FftRoots<R>::s[m]);
                acc = c_add(acc, c_mul(v[r], w));
            }
            o[q] = acc;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) v[q] = o[q];
    }
}

// one Stockham pass of radix R over `total` = rows * n / R butterflies.  ns = product of the radices before this
// pass; tw[k (R-1) + r - 1] = exp(-2 pi i r k / (ns R)), k < ns (the forward roots; conjugated for sign = +1).
template <int R>
__global__ __launch_bounds__(kFftThreads) void k_fft_pass(const double2 *in, long ld_in, double2 *out, long ld_out,
                                                         int n, int ns, const double2 *tw, int sign, long total)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int nb = n / R;
    const long row = g / nb;
    const int j = (int)(g - row * nb);
    const double2 *src = in + row * ld_in;
    double2 *dst = out + row * ld_out;
    const int k = j % ns;
    double2 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = src[j + r * nb];
    if (ns > 1) {
#pragma unroll
        for (int r = 1; r < R; ++r) {
            double2 w = tw[(long)k * (R - 1) + r - 1];
            if (sign > 0) w.y = -w.y;
            v[r] = c_mul(v[r], w);
        }
    }
    fft_small<R>(v, sign);
    const int base = (j / ns) * ns * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) dst[base + r * ns] = v[r];
}

// rows of n values: out[row][k] = in[row][k]
__global__ __launch_bounds__(kFftThreads) void k_fft_copy(const double2 *in, long ld_in, double2 *out, long ld_out,
                                                         long n, long total)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long row = g / n, k = g - row * n;
    out[row * ld_out + k] = in[row * ld_in + k];
}

// Bluestein, forward form (the backward transform is conj(forward(conj x))): a[row][j] = x[j] w[j] for j < n,
// 0 for n <= j < m, with the chirp w[j] = exp(-pi i (j^2 mod 2n) / n)
__global__ __launch_bounds__(kFftThreads) void k_blue_pre(const double2 *in, long ld_in, double2 *a, long n, long m,
                                                         const double2 *chirp, int conj_in, long total)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long row = g / m, j = g - row * m;
    double2 v = make_double2(0.0, 0.0);
    if (j < n) {
        v = in[row * ld_in + j];
        if (conj_in) v.y = -v.y;
        v = c_mul(v, chirp[j]);
    }
    a[g] = v;
}

// a[row][k] *= B[k], B = the inner forward transform of the conjugate chirp divided by m
__global__ __launch_bounds__(kFftThreads) void k_blue_mul(double2 *a, long m, const double2 *b, long total)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    a[g] = c_mul(a[g], b[g % m]);
}

// out[row][k] = w[k] conv[row][k], k < n (conjugated for the backward transform)
__global__ __launch_bounds__(kFftThreads) void k_blue_post(const double2 *a, long m, double2 *out, long ld_out, long n,
                                                          const double2 *chirp, int conj_out, long total)
{
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long row = g / n, k = g - row * n;
    double2 v = c_mul(chirp[k], a[row * m + k]);
    if (conj_out) v.y = -v.y;
    out[row * ld_out + k] = v;
}

}  // namespace htm
