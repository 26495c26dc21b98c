// Lock-step HMC with a dense mass matrix: what pglm_hmc.h lacks for it, per element.  Everything else -- the random
// numbers, the target and its NaN rules, the decision and the step-size rule -- is pglm_hmc.h, unchanged.
//
// The inverse mass matrix of a row is Sigma = W W^T, W (P, P) lower triangular, row-major.  The chain runs in the
// whitened momentum r = W^T p (p ~ N(0, Sigma^-1) makes r standard normal), which needs W alone and no solve:
//   kinetic       K = 1/2 p^T Sigma p = 1/2 sum_j r_j^2;
//   transition t  r_j = z_j, the draws of pglm_hmc.h (the SAME numbers as the diagonal chain);  H0 = U(q0) + K(r);
//                 r -= eps/2 W^T grad U(q0);  n_leapfrog times:  q += eps W r;  r -= eps W^T grad U(q)  (eps/2 the last
//                 time);  H1 = U(q) + K(r);  pgl_hmc_decide.
// That is Neal's algorithm with M^-1 = Sigma: q' = Sigma p and p' = -grad U, written for r.  With W = diag(sqrt(minv))
// it is the diagonal chain of pglm_hmc.h in exact arithmetic (r_j = sqrt(minv_j) p_j).
// The state block is that of pglm_hmc.h; its p array holds r.
//
// The two products are sums over part of a row or of a column of W; the caller chooses how the terms are dealt out (the
// device: one lane or one wave per stride, pglm_hmc_dense.hip.h; the host mirror: all in index order) and adds the partial
// sums in an order of its own.  Only j <= i is ever read: the strict upper triangle of W may hold anything.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_HMC_DENSE_H
#define PGLM_HMC_DENSE_H

#include "pglm_hmc.h"

// part of (W x)_i = sum_{j <= i} W[i, j] x_j:  the terms j = j0, j0 + stride, ... in that order
PGL_HMC_FN double pgl_hmcd_row_dot(const double* W, int P, int i, const double* x, int j0, int stride)
{
    const double* w = W + (long long)i * P;
    double a = 0.0;
#pragma unroll 4
    for (int j = j0; j <= i; j += stride) a += w[j] * x[j];
    return a;
}
// part of (W^T x)_j = sum_{i >= j} W[i, j] x_i:  the terms i = i0, i0 + stride, ... with i >= j, in that order
PGL_HMC_FN double pgl_hmcd_col_dot(const double* W, int P, int j, const double* x, int i0, int stride)
{
    double a = 0.0;
#pragma unroll 4
    for (int i = i0; i < P; i += stride)
        if (i >= j) a += W[(long long)i * P + j] * x[i];
    return a;
}
PGL_HMC_FN double pgl_hmcd_kinetic_elem(double r) { return r * r; }                          // K = 1/2 sum of these
// kick and drift from the finished products a = (W^T grad U)_j and b = (W r)_j
PGL_HMC_FN double pgl_hmcd_kick(double r, double scale, double step, double a) { return pgl_hmc_kick(r, scale, step, a); }
PGL_HMC_FN double pgl_hmcd_drift(double q, double step, double b) { return pgl_hmc_drift(q, step, 1.0, b); }

#endif
