/* Host build of the rules of stimulus decoding (theano_pyglm_amd/csrc/pglm_decode.h) for the CPU tests and as the mirror of the
 * k_dec_* kernels:
 *   decode_eval     c, S (nT, N), basis (Rt, B), theta (N, P), u (Tu, D) -> F[3], grad (Tu, D) or null and, where v is given, hv;
 *                   work: Rt D N + 3 nT N + 2 nT D doubles;
 *   decode_points   the ll term, the residual and the curvature of every element at x = c + K * (L u): term, r, cc (nT, N);
 *                   work: Rt D N + nT D doubles;
 *   decode_interp / decode_interp_t / decode_conv / decode_corr   L, L^T, K * and K^T on their own (the adjoint identities).
 * With DECODE_HOST_MAIN: a program that reads problems from a file and runs decode_eval on each (the sanitizer run). */
#include "../../theano_pyglm_amd/csrc/pglm_decode.h"

static void filters(const double* basis, int Rt, int B, int D, const double* theta, int P, int N, double* K)
{
    for (int tau = 0; tau < Rt; ++tau)
        for (int d = 0; d < D; ++d)
            for (int n = 0; n < N; ++n) K[((long long)tau * D + d) * N + n] = pgl_dec_filter_at(basis, B, theta, P, tau, d, n);
}

void decode_eval(long long nT, int N, int nlin, double dt, const double* c, const double* S, const double* basis, int Rt, int B, int D,
                 const double* theta, int P, const double* u, long long Tu, int q, double mu, double sigma, double rho,
                 const double* v, double* F, double* grad, double* hv, double* work)
{
    const PglDecPrior prior = {mu, sigma, rho};
    double* K = work;
    double* r = K + (long long)Rt * D * N;
    double* cc = r + nT * N;
    double* y = cc + nT * N;
    double* s = y + nT * N;
    double* gs = s + nT * D;
    filters(basis, Rt, B, D, theta, P, N, K);
    pgl_dec_eval_host(nT, N, nlin, dt, c, S, K, Rt, D, u, Tu, q, &prior, F, grad, r, cc, s, gs);
    if (v) pgl_dec_hvp_host(nT, N, cc, K, Rt, D, v, Tu, q, &prior, hv, s, y, gs);
}

void decode_points(long long nT, int N, int nlin, double dt, const double* c, const double* S, const double* basis, int Rt, int B, int D,
                   const double* theta, int P, const double* u, long long Tu, int q, double* term, double* r, double* cc,
                   double* work)
{
    double* K = work;
    double* s = K + (long long)Rt * D * N;
    filters(basis, Rt, B, D, theta, P, N, K);
    for (long long t = 0; t < nT; ++t)
        for (int d = 0; d < D; ++d) s[t * D + d] = pgl_dec_interp_at(u, Tu, D, q, t, d);
    for (long long t = 0; t < nT; ++t)
        for (int n = 0; n < N; ++n)
            pgl_dec_point(c[t * N + n] + pgl_dec_conv_at(K, Rt, D, N, s, t, n), S[t * N + n], nlin, dt, &term[t * N + n], &r[t * N + n],
                          &cc[t * N + n]);
}

void decode_interp(const double* u, long long Tu, int D, int q, long long nT, double* s)
{
    for (long long t = 0; t < nT; ++t)
        for (int d = 0; d < D; ++d) s[t * D + d] = pgl_dec_interp_at(u, Tu, D, q, t, d);
}

void decode_interp_t(const double* g, long long nT, int D, int q, long long Tu, double* out)
{
    for (long long i = 0; i < Tu; ++i)
        for (int d = 0; d < D; ++d) out[i * D + d] = pgl_dec_interp_t_at(g, nT, D, q, Tu, i, d);
}

void decode_conv(const double* K, int Rt, int D, int N, const double* s, long long nT, double* I)
{
    for (long long t = 0; t < nT; ++t)
        for (int n = 0; n < N; ++n) I[t * N + n] = pgl_dec_conv_at(K, Rt, D, N, s, t, n);
}

void decode_corr(const double* K, int Rt, int D, int N, const double* y, long long nT, double* gs)
{
    for (long long t = 0; t < nT; ++t)
        for (int d = 0; d < D; ++d) gs[t * D + d] = pgl_dec_corr_at(K, Rt, D, N, y, nT, t, d);
}

#ifdef DECODE_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

/* File: per problem a header line "nT N nlin dt Rt B D P Tu q mu sigma rho" and then the arrays c, S, basis, theta, u, v as text
 * doubles.  Prints F, the largest |grad| and the largest |hv| of every problem. */
static double* read_doubles(FILE* f, long long n)
{
    double* a = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
    for (long long i = 0; i < n; ++i)
        if (fscanf(f, "%lf", &a[i]) != 1) { fprintf(stderr, "short file\n"); exit(2); }
    return a;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: decode_host_main FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    long long nT, Tu;
    int N, nlin, Rt, B, D, P, q, count = 0;
    double dt, mu, sigma, rho;
    while (fscanf(f, "%lld %d %d %lf %d %d %d %d %lld %d %lf %lf %lf", &nT, &N, &nlin, &dt, &Rt, &B, &D, &P, &Tu, &q, &mu, &sigma,
                  &rho) == 13) {
        double* c = read_doubles(f, nT * N);
        double* S = read_doubles(f, nT * N);
        double* basis = read_doubles(f, (long long)Rt * B);
        double* theta = read_doubles(f, (long long)N * P);
        double* u = read_doubles(f, Tu * D);
        double* v = read_doubles(f, Tu * D);
        double* grad = (double*)malloc((size_t)(Tu * D) * sizeof(double));
        double* hv = (double*)malloc((size_t)(Tu * D) * sizeof(double));
        double* work = (double*)malloc((size_t)((long long)Rt * D * N + 3 * nT * N + 2 * nT * D) * sizeof(double));
        double F[PGL_DEC_NF], gmax = 0.0, hmax = 0.0;
        decode_eval(nT, N, nlin, dt, c, S, basis, Rt, B, D, theta, P, u, Tu, q, mu, sigma, rho, v, F, grad, hv, work);
        for (long long i = 0; i < Tu * D; ++i) {
            gmax = fmax(gmax, fabs(grad[i]));
            hmax = fmax(hmax, fabs(hv[i]));
        }
        printf("problem %d: F = %.17g  ll = %.17g  lp = %.17g  max|grad| = %.6g  max|hv| = %.6g\n", count++, F[0], F[1], F[2], gmax, hmax);
        free(c); free(S); free(basis); free(theta); free(u); free(v); free(grad); free(hv); free(work);
    }
    fclose(f);
    return count > 0 ? 0 : 1;
}
#endif
