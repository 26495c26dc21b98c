// Hamiltonian Monte Carlo on one row (one neuron's parameter vector) as a reverse-communication state machine: the random
// numbers, the scalar decisions and the per-element updates of the algorithm, no loops over the row and no callbacks --
// the caller (the k_hmc_* row kernels of pglm_hmc.hip.h, one workgroup per neuron; tests/csrc/hmc_host.c on the host) owns
// the vectors, computes the reductions and supplies ll and its gradient.  All rows take the same number of leapfrog
// steps, so M chains advance in lock step: one ll+grad launch per leapfrog step (inference/batched_hmc.py).
//
// The algorithm is Neal (2011), "MCMC using Hamiltonian dynamics", fig. 2, exactly as inference/hmc.py: hmc / hmc_lockstep
// state it, with a diagonal mass matrix:
//   target        U(q) = -(ll(q) + log prior(q)), the priors of pgl_bfgs_objective_dev (bias.py:33, bkgd.py:76,
//                 priors.py:139 / 202);  rules of hmc_lockstep's callers (gibbs.py: _neg_lp_grad): a non-finite ll + log
//                 prior gives U = +inf, a NaN or infinite entry of the gradient of ll + log prior becomes 0;
//   kinetic       K(p) = 1/2 sum_j p_j^2 minv_j  (minv: the diagonal of the inverse mass matrix; absent = 1);
//   transition t  p_j = z_j / sqrt(minv_j), z_j standard normal;  H0 = U(q0) + K(p);  p -= eps/2 grad U(q0);
//                 n_leapfrog times:  q += eps minv o p;  p -= eps grad U(q)  (eps/2 after the last drift);
//                 H1 = U(q) + K(p);  accept iff H1 is finite and log u < H0 - H1, u uniform;
//                 on accept U and grad U of the new point are kept (hmc_lockstep's UG_curr), on reject q = q0.
//   step size     one per row.  While t < n_warmup, after the decision (adapt_step_size of inference/hmc.py):
//                 factor = 1.02 if avg_accept > 0.9 else 0.98 (avg_accept BEFORE this transition),
//                 avg_accept = 0.95 avg_accept + (1 - 0.95) accepted,  eps = clip(eps * factor, 1e-3, 1).
//                 From t = n_warmup on eps is frozen: the kept chain is a Markov chain with a fixed kernel.
//                 (The reference -- gibbs.py:306-316 and the Hmc*Update classes here -- shares ONE step size among all
//                 neurons, fed by their decisions in neuron order, and never stops adapting.)
//   random numbers  stateless, pgl_hmc_normal / pgl_hmc_accept_uniform below: a function of (seed, neuron index n,
//                 transition t, component j) alone -- the NEURON index, not the row of the call, so a chain over a range of
//                 neurons equals the matching rows of a chain over all of them.
// Every sum over a row (K, the log prior) is the caller's, in a fixed order.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_HMC_H
#define PGLM_HMC_H

#include "pglm_linesearch.h"
#if !defined(__HIPCC__)
#include <math.h>
#endif

#define PGL_HMC_FN PGL_LS_FN

#define PGL_HMC_TGT_ACCEPT 0.9
#define PGL_HMC_TIME_CONST 0.95
#define PGL_HMC_MIN_STEP 1e-3
#define PGL_HMC_MAX_STEP 1.0
#define PGL_HMC_AVG0 0.9        // avg_accept at the start of a chain (the Hmc*Update classes' start)

// The state of M rows of P parameters is ONE block of doubles: PGL_HMC_NVEC (M, P) arrays -- q, p, q0, g (= grad U at the
// last accepted point) -- then PGL_HMC_NSCAL (M) arrays, field-major, the fields of PglHmc in order.
#define PGL_HMC_NVEC 4
#define PGL_HMC_NSCAL 10

typedef struct {
    double U0, H0;              // U at the last accepted point, total energy at the start of the running transition
    double step, avg_accept;    // step size, moving average of the accept indicator
    double n_accept;            // accepted transitions among those with t >= n_warmup
    double t;                   // completed transitions
    double acc;                 // decision of the last transition (1 accepted)
    double neuron;              // neuron index of the row: n_lo + row
    double seed_lo, seed_hi;    // the two 32-bit halves of the seed
} PglHmc;

typedef unsigned long long pgl_hmc_u64;

PGL_HMC_FN int pgl_hmc_finite(double x) { return x - x == 0.0; }

// ---- random numbers (documented in include/pyglm_hip.h) ----
#define PGL_HMC_G 0x9e3779b97f4a7c15ULL
PGL_HMC_FN pgl_hmc_u64 pgl_hmc_mix(pgl_hmc_u64 z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
PGL_HMC_FN pgl_hmc_u64 pgl_hmc_key(pgl_hmc_u64 seed, pgl_hmc_u64 n, pgl_hmc_u64 t)
{
    return pgl_hmc_mix(pgl_hmc_mix(pgl_hmc_mix(seed + PGL_HMC_G) + PGL_HMC_G * (n + 1)) + PGL_HMC_G * (t + 1));
}
PGL_HMC_FN double pgl_hmc_uniform(pgl_hmc_u64 key, pgl_hmc_u64 k)      // in (0, 1]
{
    const pgl_hmc_u64 z = pgl_hmc_mix(key + PGL_HMC_G * (k + 1));
    return ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
PGL_HMC_FN double pgl_hmc_accept_uniform(pgl_hmc_u64 key) { return pgl_hmc_uniform(key, 0); }
PGL_HMC_FN double pgl_hmc_normal(pgl_hmc_u64 key, pgl_hmc_u64 j)       // Box-Muller on the uniforms 2 j + 1, 2 j + 2
{
    const double u1 = pgl_hmc_uniform(key, 2 * j + 1), u2 = pgl_hmc_uniform(key, 2 * j + 2);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
PGL_HMC_FN pgl_hmc_u64 pgl_hmc_seed(const PglHmc* s)
{
    return ((pgl_hmc_u64)s->seed_hi << 32) | (pgl_hmc_u64)s->seed_lo;
}
PGL_HMC_FN pgl_hmc_u64 pgl_hmc_row_key(const PglHmc* s)
{
    return pgl_hmc_key(pgl_hmc_seed(s), (pgl_hmc_u64)s->neuron, (pgl_hmc_u64)s->t);
}

// ---- target ----
// U from ll and the summed log prior; one entry of grad U from the entries of grad ll and grad log prior
PGL_HMC_FN double pgl_hmc_energy(double ll, double lprior)
{
    const double lp = ll + lprior;
    return pgl_hmc_finite(lp) ? -lp : (double)INFINITY;
}
PGL_HMC_FN double pgl_hmc_grad_elem(double gll, double gprior)
{
    const double g = gll + gprior;
    return pgl_hmc_finite(g) ? -g : 0.0;
}

// ---- target: priors, term by term (the caller sums the returned log densities in a fixed order) ----
// Each returns the term's log density (up to the constants the host priors drop too) and its derivative through *dlp.
PGL_HMC_FN double pgl_hmc_prior_bias(double b, double mu_b, double sg_b, double* dlp)         // bias.py:33
{
    const double d = b - mu_b;
    *dlp = -d / (sg_b * sg_b);
    return -0.5 / (sg_b * sg_b) * d * d;
}
PGL_HMC_FN double pgl_hmc_prior_stim(double w, double stim_sigma, double* dlp)                // bkgd.py:76
{
    const double is2 = 1.0 / (stim_sigma * stim_sigma);
    *dlp = -w * is2;
    return -0.5 * is2 * w * w;
}
// one presynaptic group w[0..B) of the impulse weights: kind 0 Gaussian (priors.py:139), 1 group lasso (priors.py:202;
// a zero group gives 0/0 = NaN derivatives like the host prior, which the gradient rule then turns into 0).  Returns
// the group's log density; g[0..B) holds the group's entries of grad ll on entry and of grad U on return.
PGL_HMC_FN double pgl_hmc_prior_group(int kind, const double* w, int B, double mu, double sigma, double lam, double* g)
{
    double lp = 0.0;
    if (kind == 1) {
        double ss = 0.0;
        for (int b = 0; b < B; ++b) {
            const double z = (w[b] - mu) / sigma;
            ss += z * z;
        }
        const double nrm = sqrt(ss);
        lp = -lam * nrm;
        for (int b = 0; b < B; ++b) g[b] = pgl_hmc_grad_elem(g[b], -lam * ((w[b] - mu) / sigma) / nrm / sigma);
    } else {
        const double is2 = 1.0 / (sigma * sigma);
        for (int b = 0; b < B; ++b) {
            const double d = w[b] - mu;
            lp += -0.5 * is2 * d * d;
            g[b] = pgl_hmc_grad_elem(g[b], -d * is2);
        }
    }
    return lp;
}
// ---- dynamics, per element ----
PGL_HMC_FN double pgl_hmc_momentum(double z, double minv) { return z / sqrt(minv); }
PGL_HMC_FN double pgl_hmc_kinetic_elem(double p, double minv) { return p * p * minv; }      // K = 1/2 sum of these
PGL_HMC_FN double pgl_hmc_kick(double p, double scale, double step, double g) { return p - scale * step * g; }
PGL_HMC_FN double pgl_hmc_drift(double q, double step, double minv, double p) { return q + step * (minv * p); }

// ---- the scalar state ----
PGL_HMC_FN void pgl_hmc_init(PglHmc* s, double U0, double step0, int neuron, pgl_hmc_u64 seed)
{
    s->U0 = U0; s->H0 = U0;
    s->step = step0; s->avg_accept = PGL_HMC_AVG0;
    s->n_accept = 0.0; s->t = 0.0; s->acc = 0.0;
    s->neuron = (double)neuron;
    s->seed_lo = (double)(seed & 0xffffffffULL); s->seed_hi = (double)(seed >> 32);
}
// start of a transition: ksum = sum_j p_j^2 minv_j of the fresh momentum
PGL_HMC_FN void pgl_hmc_begin(PglHmc* s, double ksum) { s->H0 = s->U0 + 0.5 * ksum; }
// end of a transition: U1 at the end of the trajectory, ksum of the final momentum, u the accept uniform.  Returns the
// decision; on accept the caller keeps the point and its gradient, else restores q0.  Then the step-size rule while
// t < n_warmup, and t += 1.
PGL_HMC_FN int pgl_hmc_decide(PglHmc* s, double U1, double ksum, double u, int n_warmup)
{
    const double H1 = U1 + 0.5 * ksum;
    const int acc = pgl_hmc_finite(H1) && log(u) < s->H0 - H1;
    if (acc) s->U0 = U1;
    s->acc = (double)acc;
    if (s->t < (double)n_warmup) {
        const double factor = s->avg_accept > PGL_HMC_TGT_ACCEPT ? 1.02 : 0.98;
        s->avg_accept = PGL_HMC_TIME_CONST * s->avg_accept + (1.0 - PGL_HMC_TIME_CONST) * (double)acc;
        double e = s->step * factor;
        e = e < PGL_HMC_MIN_STEP ? PGL_HMC_MIN_STEP : (e > PGL_HMC_MAX_STEP ? PGL_HMC_MAX_STEP : e);
        s->step = e;
    } else if (acc) s->n_accept += 1.0;
    s->t += 1.0;
    return acc;
}

#endif
