// Annealed importance sampling (Neal 2001, "Annealed importance sampling") on one row -- one particle of one neuron's
// parameter vector -- as a reverse-communication state machine on top of pglm_hmc.h: the random numbers, prior terms, NaN
// rules, leapfrog dynamics and step-size rule are that header's; this one adds the tempered target, the exact prior
// draw, the weight and what a row keeps so that a change of temperature needs no evaluation.  The caller (the k_ais_*
// row kernels of pglm_ais.hip.h, one workgroup per row; tests/csrc/ais_host.c on the host) owns the vectors, computes
// the reductions and supplies ll and its gradient.
//
//   rows          R = K M: K particles of the M neurons n_lo .. n_lo + M - 1, particle-major: row r = k M + i is particle
//                 particle0 + k of neuron n_lo + i, so block k of an (R, P) array is the (M, P) block of one pgl_ll_grad_dev.
//   ladder        0 = beta_0 < beta_1 < ... < beta_J = 1.
//   target        U_beta(q) = -(beta ll(q) + log prior(q)),  grad U_beta = -(beta grad ll + grad log prior), with the
//                 rules of pglm_hmc.h (pgl_hmc_energy, pgl_hmc_grad_elem: a non-finite sum gives U = +inf, a non-finite
//                 gradient entry becomes 0).  Gaussian priors only (kind 0): bias N(mu_b, sg_b), stimulus weights
//                 N(0, stim_sigma), impulse weights N(mu, sigma) -- the start is an exact draw from the NORMALISED prior.
//   per row       1. q_j = m_j + s_j z_j (pgl_ais_draw), z_j the normals of transition number 0; evaluate; log w = 0.
//                 2. for j = 1 .. J:  log w += (beta_j - beta_{j-1}) ll0, ll0 = ll at the CURRENT point, i.e. the point
//                    sampled under beta_{j-1} (a non-finite ll0 gives log w = -inf for good: the particle is dead);
//                    then the target becomes U_{beta_j} (and, frozen mode, the row's step that temperature's table entry);
//                 3. for j < J: n_steps HMC transitions (Neal 2011 fig. 2 exactly as pglm_hmc.h) that leave
//                    prior x L^beta_j invariant.  No move follows the last weight.
//                 This is Neal's order.  (The reference, pyglm/inference/parallel_ais.py, moves under beta_j first and
//                 then weighs f_j / f_{j-1} at the MOVED point, which is not Neal's estimator and is biased.)
//   kept per row  ll0, lp0 (log prior, constants dropped as the host priors drop them) and gll = grad ll at the current
//                 point, separately: U0 = pgl_hmc_energy(beta ll0, lp0) and g are recomputed from them at every
//                 temperature change.
//   random numbers  pglm_hmc.h's, with a seed per particle: s = pgl_ais_particle_seed(seed, particle); transition number 0
//                 is the prior draw, the moves are numbered from 1 across the whole ladder (documented in
//                 include/pyglm_hip.h).  Keyed by the NEURON and PARTICLE indices, not the row of the call.
//   step size     adapting mode: pgl_hmc_decide's rule after every transition.  Frozen mode: never changed by a decision,
//                 set from a table at every temperature change -- AIS weights need transition kernels fixed in advance.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_AIS_H
#define PGLM_AIS_H

#include "pglm_hmc.h"

// The state of R rows of P parameters is ONE block of doubles: PGL_AIS_NVEC (R, P) arrays -- q, p, q0, g (= grad U_beta at
// the current point), gll (= grad ll there), gu (= grad U_beta along the running trajectory) -- then PGL_AIS_NSCAL (R)
// arrays, field-major, the fields of PglAis in order.
#define PGL_AIS_NVEC 6
#define PGL_AIS_NSCAL 15
#define PGL_AIS_ADAPT_ALWAYS 0x7fffffff

typedef struct {
    PglHmc h;                   // U0 = U_beta at the current point; seed_lo / seed_hi: the PARTICLE's seed; t from 1
    double ll0, lp0;            // log likelihood and log prior at the current point
    double beta;                // the temperature of the target
    double logw;                // log weight
    double particle;            // particle index of the row: particle0 + row / M
} PglAis;

// seed of one particle's stream; particle = -1 is a stream of its own too (the driver's pilot)
PGL_HMC_FN pgl_hmc_u64 pgl_ais_particle_seed(pgl_hmc_u64 seed, long long particle)
{
    return pgl_hmc_mix(seed + PGL_HMC_G * (pgl_hmc_u64)(particle + 1));
}

// mean and sd of component c of the row [bias, w_stim (Dstim), w_ir] under the Gaussian priors
PGL_HMC_FN double pgl_ais_prior_mean(int c, int Dstim, double mu_b, double mu) { return c == 0 ? mu_b : (c <= Dstim ? 0.0 : mu); }
PGL_HMC_FN double pgl_ais_prior_sd(int c, int Dstim, double sg_b, double stim_sigma, double sigma)
{
    return c == 0 ? sg_b : (c <= Dstim ? stim_sigma : sigma);
}
PGL_HMC_FN double pgl_ais_draw(double mean, double sd, double z) { return mean + sd * z; }

// the tempered target from the kept parts
PGL_HMC_FN double pgl_ais_energy(double beta, double ll, double lp) { return pgl_hmc_energy(beta * ll, lp); }
PGL_HMC_FN double pgl_ais_scaled(double beta, double gll) { return beta * gll; }   // then pgl_hmc_grad_elem / _prior_group

// start of a row, after the prior draw
PGL_HMC_FN void pgl_ais_init(PglAis* s, double step0, int neuron, long long particle, pgl_hmc_u64 seed)
{
    pgl_hmc_init(&s->h, 0.0, step0, neuron, pgl_ais_particle_seed(seed, particle));
    s->h.t = 1.0;                                             // (transition number 0 was the prior draw)
    s->ll0 = 0.0; s->lp0 = 0.0; s->beta = 0.0; s->logw = 0.0;
    s->particle = (double)particle;
}
// the evaluation at the current point (the start; an accepted move)
PGL_HMC_FN void pgl_ais_keep(PglAis* s, double ll, double lp) { s->ll0 = ll; s->lp0 = lp; }
// temperature change: the weight of the current point, then the new target
PGL_HMC_FN void pgl_ais_temper(PglAis* s, double beta_new)
{
    if (!pgl_hmc_finite(s->ll0) || s->logw == -(double)INFINITY) s->logw = -(double)INFINITY;
    else s->logw += (beta_new - s->beta) * s->ll0;
    s->beta = beta_new;
    s->h.U0 = pgl_ais_energy(beta_new, s->ll0, s->lp0);
}
// end of a transition: pgl_hmc_decide (adapt != 0: the step-size rule, every time; 0: frozen); on accept the new point's
// ll and log prior are kept
PGL_HMC_FN int pgl_ais_decide(PglAis* s, double ll1, double lp1, double ksum, double u, int adapt)
{
    const int acc = pgl_hmc_decide(&s->h, pgl_ais_energy(s->beta, ll1, lp1), ksum, u, adapt ? PGL_AIS_ADAPT_ALWAYS : 0);
    if (acc) pgl_ais_keep(s, ll1, lp1);
    return acc;
}

#endif
