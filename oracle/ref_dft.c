/* ref_dft.c -- TEST INFRASTRUCTURE ONLY.  A stand-in for the four FFTW 3 calls the reference's steps 2 and 3 make
 * (declared for Fortran in oracle/fftw3.f03), so that their unmodified sources compile and run without FFTW.
 *
 * Direct DFTs with FFTW's semantics, summed and twiddled in long double, rounded to double once per output:
 *   r2c: X[k] = sum_m x[m] exp(-2 pi i k m / n) for k = 0 .. n/2 (n/2 + 1 outputs);
 *   c2r: y[m] = sum_k X[k] exp(+2 pi i k m / n) over the Hermitian extension of the n/2 + 1 inputs, unnormalised;
 *        the imaginary parts of bin 0 and (n even) bin n/2 are ignored, the input is not overwritten.
 * The values agree with FFTW's to rounding only, not bit for bit.  O(n^2): meant for the oracle's short windows.
 * Plans are never destroyed (the reference never destroys them). */
#include <complex.h>
#include <math.h>
#include <stdlib.h>

typedef struct {
    int n;
    long double *c, *s;         /* cos / sin of 2 pi j / n, j = 0 .. n-1 */
} ref_plan;

static ref_plan *make_plan(int n)
{
    if (n < 1) return NULL;
    ref_plan *p = malloc(sizeof *p);
    if (!p) return NULL;
    p->n = n;
    p->c = malloc((size_t)n * sizeof(long double));
    p->s = malloc((size_t)n * sizeof(long double));
    if (!p->c || !p->s) { free(p->c); free(p->s); free(p); return NULL; }
    const long double two_pi = 2.0L * acosl(-1.0L);
    for (int j = 0; j < n; ++j) {
        p->c[j] = cosl(two_pi * (long double)j / (long double)n);
        p->s[j] = sinl(two_pi * (long double)j / (long double)n);
    }
    return p;
}

void *fftw_plan_dft_r2c_1d(int n, double *in, double complex *out, int flags)
{
    (void)in; (void)out; (void)flags;
    return make_plan(n);
}

void *fftw_plan_dft_c2r_1d(int n, double complex *in, double *out, int flags)
{
    (void)in; (void)out; (void)flags;
    return make_plan(n);
}

void fftw_execute_dft_r2c(const void *plan, double *in, double complex *out)
{
    const ref_plan *p = plan;
    const int n = p->n;
    for (int k = 0; k <= n / 2; ++k) {
        long double re = 0.0L, im = 0.0L;
        for (int m = 0; m < n; ++m) {
            const int j = (int)(((long)k * m) % n);
            re += (long double)in[m] * p->c[j];
            im -= (long double)in[m] * p->s[j];
        }
        double *o = (double *)&out[k];       /* C99: a complex is an array of its two parts */
        o[0] = (double)re;
        o[1] = (double)im;
    }
}

void fftw_execute_dft_c2r(const void *plan, double complex *in, double *out)
{
    const ref_plan *p = plan;
    const int n = p->n;
    const int top = (n - 1) / 2;        /* bins 1 .. top appear twice in the Hermitian extension */
    for (int m = 0; m < n; ++m) {
        long double acc = (long double)creal(in[0]);
        if (n % 2 == 0) acc += (m % 2 ? -1.0L : 1.0L) * (long double)creal(in[n / 2]);
        for (int k = 1; k <= top; ++k) {
            const int j = (int)(((long)k * m) % n);
            acc += 2.0L * ((long double)creal(in[k]) * p->c[j] - (long double)cimag(in[k]) * p->s[j]);
        }
        out[m] = (double)acc;
    }
}
