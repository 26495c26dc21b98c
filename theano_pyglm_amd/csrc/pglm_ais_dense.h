// Annealed importance sampling with a dense, tempered mass matrix: what pglm_ais.h and pglm_hmc_dense.h lack for it, per
// element.  Everything else -- the ladder, the weights, the kept parts ll0 / lp0 / gll, the random numbers, the decision
// and the step-size rule -- is pglm_ais.h over pglm_hmc.h; the whitened momentum and the two triangular products are
// pglm_hmc_dense.h.  Nothing of either is restated here.
//
// The transition at temperature beta with the inverse mass matrix Sigma = W W^T (W (P, P) lower triangular, shared by the
// particles of a neuron), in the whitened momentum r = W^T p:
//   r_j = z_j, the draws of the diagonal AIS row (same key, same seed per particle);  H0 = U_beta + 1/2 sum_j r_j^2
//   (pgl_hmcd_kinetic_elem, pgl_hmc_begin);  r -= eps/2 W^T grad U_beta (pgl_hmcd_col_dot, pgl_hmcd_kick);  n_leapfrog
//   times { q += eps W r (pgl_hmcd_row_dot, pgl_hmcd_drift);  r -= eps W^T grad U_beta(q), eps/2 the last time };
//   H1 = U_beta(q) + 1/2 sum_j r_j^2;  pgl_ais_decide (adapt != 0: the step-size rule).
// The state block is pglm_ais.h's; its p array holds r.  With W = diag(sqrt(minv)) this is the diagonal AIS row in exact
// arithmetic.
//
// The tempered mass.  The priors are Gaussian, so the prior precision Lambda is a known diagonal; with G = minus the
// Hessian of ll at a fitted point, the Gaussian approximation of the target prior x L^beta has precision
//   A_beta = beta G + Lambda,
// positive definite for every beta >= 0 where ll is concave, and the prior exactly at beta = 0.  W_beta is the lower factor
// of A_beta^-1.  A mass that depends on beta but not on the particle's state keeps every transition valid for its target.
// A row whose A_beta does not factor runs on W = diag(pgl_aisd_fallback(diag A_beta)), the 'laplace' rule.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_AIS_DENSE_H
#define PGLM_AIS_DENSE_H

#include "pglm_ais.h"
#include "pglm_hmc_dense.h"

// entry c of the diagonal of Lambda for the row [bias, w_stim (Dstim), w_ir]
PGL_HMC_FN double pgl_aisd_prior_precision(int c, int Dstim, double sg_b, double stim_sigma, double sigma)
{
    const double sd = pgl_ais_prior_sd(c, Dstim, sg_b, stim_sigma, sigma);
    return 1.0 / (sd * sd);
}
// entry (i, j) of A_beta from G[i, j]; lam = Lambda_ii on the diagonal, 0 off it
PGL_HMC_FN double pgl_aisd_tempered(double beta, double g, double lam) { return beta * g + lam; }
// diagonal entry of the fallback factor from a = (A_beta)_ii: 1 / sqrt(max(a, floor)), a non-finite a counting as floor
PGL_HMC_FN double pgl_aisd_fallback(double a, double floor)
{
    if (!pgl_hmc_finite(a) || !(a > floor)) a = floor;
    return 1.0 / sqrt(a);
}

#endif
