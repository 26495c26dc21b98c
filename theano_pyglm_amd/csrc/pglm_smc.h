// Adaptive sequential Monte Carlo (Del Moral, Doucet & Jasra 2006; the ladder rule of Jasra et al. 2011 / Zhou, Johansen &
// Aston 2016) of the per-neuron evidence on the tempered path of pglm_ais.h: the step that couples the K particles of ONE
// neuron -- the next temperature, the evidence increment, the weights, the resampling decision and the ancestors -- as
// scalar rules on top of pglm_ais.h / pglm_hmc.h.  The caller (k_smc_stage of pglm_smc.hip.h, one workgroup per neuron;
// tests/csrc/smc_host.c on the host) owns the loops over the particles and computes the sums in a fixed order.
//
//   rows          the AIS rows: r = k M + i, particle-major, the pgl_ais_state_doubles block (q, gll, ll0, lp0, logw, ...).
//   per neuron    beta, log_Z, step (ONE step size shared by the neuron's particles), stage, done, and the records below.
//   a stage of neuron i (W_k: the normalised weights, exp(logw_k) / sum; a particle with a non-finite ll0 or logw = -inf is
//   dead: W_k = 0 and logw_k = -inf for good):
//     0. step rule (stages after the first): a = acceptances of the previous move stage / (K n_steps),
//        step <- clip(step exp(a - PGL_HMC_TGT_ACCEPT), PGL_HMC_MIN_STEP, PGL_HMC_MAX_STEP).
//     1. next temperature: CESS(d) = K (sum W_k v_k)^2 / sum W_k v_k^2, v_k = exp(d (ll0_k - max ll0)) (max over the live
//        particles).  CESS(1 - beta) >= rho K: d = 1 - beta.  Else PGL_SMC_BISECT halvings of [0, 1 - beta] (the half with
//        CESS(mid) >= rho K keeps the lower end moving up), d = the lower end.  Then d = max(d, delta_min), and d >= 1 - beta
//        gives d = 1 - beta and beta = 1 EXACTLY.
//     2. evidence and weights: log_Z += d max ll0 + log sum W_k v_k;  W_k <- W_k v_k / sum W v;  logw_k = log of it.
//        No live particle: log_Z = -inf and the neuron is done where it stands.
//     3. resampling when ESS = 1 / sum W_k^2 < ess_min K: systematic, ONE uniform u = pgl_smc_uniform(seed, neuron, stage),
//        positions (u + k) / K against the cumulative sums c_j = W_0 + ... + W_j taken in index order:
//        anc[k] = the first j with c_j >= (u + k) / K (rounding at the top end: the last live particle); then logw = 0.
//        Slot k takes q, gll, ll0, lp0 of slot anc[k]; its seed, particle index, t and step stay with the slot.
//     4. retemper: beta, U0 and g of every row from the kept parts at the new beta (pgl_ais_target_row), row step = the
//        neuron's.  beta = 1: done.  Else n_steps HMC transitions follow under the new target.
//   A done neuron never changes again: the stage returns at once, the guarded moves pass its rows by.
//   Adaptive SMC estimates of Z are consistent, not unbiased as Neal's AIS is.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_SMC_H
#define PGLM_SMC_H

#include "pglm_ais.h"

// The per-neuron block of a run of K particles x M neurons with room for S stage records, in doubles, in this order:
//   (PGL_SMC_NSCAL, M)   the fields of PglSmc, field-major
//   (PGL_SMC_NREC, S, M) the stage records: beta after the stage, ESS before resampling, CESS, resampled (0 / 1), accept
//                        rate of the moves that followed (NaN: none followed), the step those moves ran on
//   (R)  anc             ancestor particle index of every row, of the last stage
//   (R)  w               normalised weights after the last stage's update, before its resampling
//   (R)  acc             acceptances of every row since the last stage (the guarded leap adds, the stage sums and clears)
//   (1)  n_active        neurons not done after the last stage: the ONE number the host reads per stage
//   (R, P) tq, (R, P) tg, (2, R) ts   scratch of the out-of-place gather: q, gll and ll0, lp0
#define PGL_SMC_NSCAL 10
#define PGL_SMC_NREC 6
#define PGL_SMC_BISECT 60
enum { PGL_SMC_R_BETA = 0, PGL_SMC_R_ESS = 1, PGL_SMC_R_CESS = 2, PGL_SMC_R_RS = 3, PGL_SMC_R_ACC = 4, PGL_SMC_R_STEP = 5 };

typedef struct {
    double beta, log_Z;         // temperature of the neuron's target, running log evidence
    double step;                // the neuron's step size
    double stage;               // completed stages
    double done;                // 1: beta = 1 was reached, or every particle is dead
    double n_resampled;         // resamplings so far
    double acc;                 // acceptances of the last move stage, summed over the particles
    double live;                // the last stage call changed the neuron's rows (0: it was done before, or all dead)
    double rs;                  // the last stage call resampled
    double ess;                 // ESS of the weights after the last stage's update, before its resampling
} PglSmc;

#define PGL_SMC_SEED_SALT 0x5eed5eed5eed5eedULL
// the resampling uniform of (seed, neuron, stage), in (0, 1): a stream of its own beside the particles' (documented in
// include/pyglm_hip.h)
PGL_HMC_FN double pgl_smc_uniform(pgl_hmc_u64 seed, pgl_hmc_u64 neuron, pgl_hmc_u64 stage)
{
    return pgl_hmc_uniform(pgl_hmc_key(pgl_hmc_mix(seed ^ PGL_SMC_SEED_SALT), neuron, stage), 0);
}

PGL_HMC_FN void pgl_smc_init(PglSmc* s, double step0)
{
    s->beta = 0.0; s->log_Z = 0.0; s->step = step0; s->stage = 0.0; s->done = 0.0; s->n_resampled = 0.0; s->acc = 0.0;
    s->live = 0.0; s->rs = 0.0; s->ess = 0.0;
}
PGL_HMC_FN int pgl_smc_alive(double ll0, double logw) { return pgl_hmc_finite(ll0) && logw != -(double)INFINITY && logw == logw; }

PGL_HMC_FN double pgl_smc_step_rule(double step, double a)
{
    const double e = step * exp(a - PGL_HMC_TGT_ACCEPT);
    return e < PGL_HMC_MIN_STEP ? PGL_HMC_MIN_STEP : (e > PGL_HMC_MAX_STEP ? PGL_HMC_MAX_STEP : e);
}
// the incremental weight of a live particle, scaled by the largest
PGL_HMC_FN double pgl_smc_v(double delta, double ll0, double ll_max) { return exp(delta * (ll0 - ll_max)); }
// CESS from s1 = sum W v, s2 = sum W v^2
PGL_HMC_FN double pgl_smc_cess(int K, double s1, double s2) { return s2 > 0.0 ? (double)K * s1 * s1 / s2 : 0.0; }
// the temperature step from the bisection's lower end: the floor, then the snap to beta = 1.  Returns delta, *beta_new.
PGL_HMC_FN double pgl_smc_delta(double lo, double delta_min, double beta, double* beta_new)
{
    const double rem = 1.0 - beta;
    double d = lo < delta_min ? delta_min : lo;
    if (d >= rem || beta + d >= 1.0) { *beta_new = 1.0; return rem; }
    *beta_new = beta + d;
    return d;
}
// sampling position k of K
PGL_HMC_FN double pgl_smc_position(double u, int k, int K) { return (u + (double)k) / (double)K; }
// the first j in [0, K) with cum[j * stride] >= pos; K - 1 if none (the caller then takes the last live particle)
PGL_HMC_FN int pgl_smc_search(const double* cum, long stride, int K, double pos)
{
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (cum[(long)mid * stride] >= pos) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

#endif
