// The Wald statistic of ONE coupling group of one neuron from the lower factor W of its Laplace covariance, W W^T = A^-1
// (inference/laplace.py: laplace_from_factor).  The per-pair Granger-causality test of point-process GLMs (Kim, Putrino,
// Ghosh & Brown 2011) in its Wald form: under H0: w_g = 0 the statistic is approximately chi-square with B degrees of freedom.
// In the style of pglm_psis.h and pglm_acf.h: the rule in plain C, pgl_wald_group the whole rule of one group with the lanes
// of a wave played serially -- the host mirror (tests/csrc/wald_host.c).  k_wald_groups (pglm_wald.hip.h, one wave per
// group) owns the parallel form of the two sums over the columns and calls pgl_wald_finish for the B x B algebra.
//
// Inputs of row m, group g: W (lower triangular, leading dimension ld, only the entries j <= i are read), the theta row, the
// offset o = first + g B of the group's B weights w = theta[o .. o + B), a contrast c of B doubles.
//
// The rule:
//  1. S = W_g W_g^T (B x B), the group's block of the covariance:  S[a][b] = sum_{k = 0}^{o + min(a, b)} W[o+a][k] W[o+b][k].
//     Order of the sum (part of the rule): column k belongs to lane k mod PGL_WALD_LANES (64); a lane adds its products in
//     ascending k from 0.0; the 64 lane sums are combined by the binary tree  p[l] += p[l + h], h = 32, 16, .. 1.  A lane
//     without a column holds 0.0.
//  2. lin = sum_a c[a] w[a] and var = sum_a c[a] (sum_b S[a][b] c[b]), each sum ascending from 0.0.
//  3. S = L L^T, unpivoted, row by row:  s = S[a][b] - sum_{k < b} L[a][k] L[b][k] (k ascending, one subtraction per term);
//     L[a][b] = s / L[b][b] (b < a), L[a][a] = sqrt(s).  A pivot s that is not finite or <= 0 ends the group: info = a + 1,
//     T = lin = var = NaN, y = NaN.
//  4. y = S^-1 w:  z[a] = (w[a] - sum_{k < a} L[a][k] z[k]) / L[a][a], a ascending;
//                  y[a] = (z[a] - sum_{k > a} L[k][a] y[k]) / L[a][a], a descending, k ascending.
//  5. T = sum_a w[a] y[a], ascending from 0.0.
//  6. on request u = W_g^T y, the direction of the restricted Newton step (theta - W u has the group at zero under the
//     quadratic approximation):  u[k] = sum_{a : k <= o + a} W[o+a][k] y[a], a ascending from 0.0, for k < o + B; u[k] = 0
//     for o + B <= k < P.
// Every product and every sum is rounded on its own: the functions below are compiled with FP contraction off, as
// pglm_acf.h's.  The order depends on (o, B) alone: a group gives the same bits alone or among others, on any grid, run
// after run, and the device, this file under gcc and the numpy statement inference/connectivity.py: wald_groups agree bit
// for bit on the same input.
//
// Output: PGL_WALD_NOUT doubles per group: T, lin, var, info (as a double).
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_WALD_H
#define PGLM_WALD_H

#include "pglm_hmc.h"

#define PGL_WALD_MAX_B 16
#define PGL_WALD_NOUT 4
#define PGL_WALD_LANES 64

#if defined(__clang__)
#define PGL_WALD_FN PGL_HMC_FN
#define PGL_WALD_NOCONTRACT _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define PGL_WALD_FN __attribute__((optimize("fp-contract=off"))) PGL_HMC_FN
#define PGL_WALD_NOCONTRACT
#else
#define PGL_WALD_FN PGL_HMC_FN
#define PGL_WALD_NOCONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define PGL_WALD_SQRT(x) __dsqrt_rn(x)
#else
#define PGL_WALD_SQRT(x) sqrt(x)
#endif

// one step of a sum: s + a b in two roundings
PGL_WALD_FN double pgl_wald_madd(double s, double a, double b)
{
    PGL_WALD_NOCONTRACT
    const double t = a * b;
    return s + t;
}

// Steps 2 .. 5 on the lower triangle of S (S[a * B + b], b <= a; it becomes L in place), w (B), c (B): out (4) and y (B).
// Returns the group's info.
PGL_WALD_FN int pgl_wald_finish(double* S, const double* w, const double* c, int B, double* out, double* y)
{
    PGL_WALD_NOCONTRACT
    const double nan = __builtin_nan("");
    double lin = 0.0, var = 0.0;
    for (int a = 0; a < B; ++a) {
        const double t = c[a] * w[a];
        lin = lin + t;
        double r = 0.0;
        for (int b = 0; b < B; ++b) {
            const double q = (b <= a ? S[a * B + b] : S[b * B + a]) * c[b];
            r = r + q;
        }
        const double v = c[a] * r;
        var = var + v;
    }
    int info = 0;
    for (int a = 0; a < B && !info; ++a) {
        for (int b = 0; b <= a; ++b) {
            double s = S[a * B + b];
            for (int k = 0; k < b; ++k) {
                const double t = S[a * B + k] * S[b * B + k];
                s = s - t;
            }
            if (b < a) {
                S[a * B + b] = s / S[b * B + b];
            } else if (!pgl_hmc_finite(s) || !(s > 0.0)) {
                info = a + 1;
            } else {
                S[a * B + a] = PGL_WALD_SQRT(s);
            }
        }
    }
    if (info) {
        for (int a = 0; a < B; ++a) y[a] = nan;
        out[0] = nan;
        out[1] = nan;
        out[2] = nan;
        out[3] = (double)info;
        return info;
    }
    for (int a = 0; a < B; ++a) {
        double s = w[a];
        for (int k = 0; k < a; ++k) {
            const double t = S[a * B + k] * y[k];
            s = s - t;
        }
        y[a] = s / S[a * B + a];
    }
    for (int a = B - 1; a >= 0; --a) {
        double s = y[a];
        for (int k = a + 1; k < B; ++k) {
            const double t = S[k * B + a] * y[k];
            s = s - t;
        }
        y[a] = s / S[a * B + a];
    }
    double T = 0.0;
    for (int a = 0; a < B; ++a) {
        const double t = w[a] * y[a];
        T = T + t;
    }
    out[0] = T;
    out[1] = lin;
    out[2] = var;
    out[3] = 0.0;
    return 0;
}

// u[k] of step 6 for one column k < P
PGL_WALD_FN double pgl_wald_u(const double* W, long long ld, long long o, int B, const double* y, long long k)
{
    PGL_WALD_NOCONTRACT
    double s = 0.0;
    for (int a = 0; a < B; ++a)
        if (k <= o + a) {
            const double t = W[(o + a) * ld + k] * y[a];
            s = s + t;
        }
    return s;
}

// The whole rule of one group with the lanes played serially: out (4), and u (P) where u is not null.  Returns info.
PGL_WALD_FN int pgl_wald_group(const double* W, long long P, long long ld, const double* theta, long long o, int B, const double* c,
                               double* out, double* u)
{
    PGL_WALD_NOCONTRACT
    double S[PGL_WALD_MAX_B * PGL_WALD_MAX_B], y[PGL_WALD_MAX_B], p[PGL_WALD_LANES];
    for (int a = 0; a < B; ++a)
        for (int b = 0; b <= a; ++b) {
            const double* ra = W + (o + a) * ld;
            const double* rb = W + (o + b) * ld;
            for (int l = 0; l < PGL_WALD_LANES; ++l) p[l] = 0.0;
            for (long long k = 0; k <= o + b; ++k) p[k % PGL_WALD_LANES] = pgl_wald_madd(p[k % PGL_WALD_LANES], ra[k], rb[k]);
            for (int h = PGL_WALD_LANES / 2; h > 0; h >>= 1)
                for (int l = 0; l < h; ++l) p[l] = p[l] + p[l + h];
            S[a * B + b] = p[0];
        }
    const int info = pgl_wald_finish(S, theta + o, c, B, out, y);
    if (u)
        for (long long k = 0; k < P; ++k) u[k] = k < o + B ? pgl_wald_u(W, ld, o, B, y, k) : 0.0;
    return info;
}

#endif
