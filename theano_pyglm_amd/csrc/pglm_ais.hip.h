// annealed importance sampling row kernels: k_ais_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// Annealed importance sampling of the per-neuron evidence (inference/batched_ais.py): K particles of all M neurons of a
// range -- one workgroup per row r = k M + i, particle-major, so block k of any (R, P) array is the (M, P) block one
// pgl_ll_grad_dev takes and returns -- around the launches that do the work: one fused ll+grad evaluation per particle
// block per leapfrog step.  The algorithm (Neal 2001; the moves are Neal 2011 fig. 2), its random numbers and its
// decisions are pglm_ais.h over pglm_hmc.h (compiled for the host by tests/csrc/ais_host.c); these kernels own the
// vectors, the fixed-order reductions (pgl_blk_sum), the priors' part of U and its gradient and the NaN rules.  All state
// lives in ONE device block of doubles laid out by pgl_ais_view.  Every row takes the same number of steps: nothing for
// the host to read before the run has ended.
// ---------------------------------------------------------------------------
#include "pglm_ais.h"

struct AisView {
    int R, M, P;                              // rows = particles x neurons, neurons, parameters
    double *q, *p, *q0, *g, *gll, *gu;        // (R, P): point, momentum, start of the transition, grad U_beta and grad ll at
                                              // the current point, grad U_beta along the running trajectory
    double* sc;                               // (PGL_AIS_NSCAL, R): PglAis, field-major
};
__host__ __device__ inline size_t pgl_ais_doubles(size_t R, size_t P) { return R * P * PGL_AIS_NVEC + R * PGL_AIS_NSCAL; }
__host__ __device__ inline AisView pgl_ais_view(double* st, int K, int M, int P)
{
    AisView v;
    const size_t RP = (size_t)K * M * P;
    v.R = K * M; v.M = M; v.P = P;
    v.q = st; v.p = st + RP; v.q0 = st + 2 * RP; v.g = st + 3 * RP; v.gll = st + 4 * RP; v.gu = st + 5 * RP;
    v.sc = st + PGL_AIS_NVEC * RP;
    return v;
}
// the scalar rows: PglHmc's, at PglHmc's indices, then PglAis's own
#define PGL_AIS_FIELDS(F) PGL_HMC_FIELDS_IN(F, h.) F(ll0, 10) F(lp0, 11) F(beta, 12) F(logw, 13) F(particle, 14)
static_assert(PGL_HMC_NSCAL == 10 && PGL_AIS_NSCAL == 15, "PglAis's own rows follow the PGL_HMC_NSCAL rows of PglHmc");
// The rows of an AIS state as a chain of R rows, for the chain's kernels that start a transition (k_hmc_begin,
// k_hmc_dense_draw): q, p, q0, g are the first four arrays of both blocks, and the scalar rows 0 .. PGL_HMC_NSCAL - 1 are
// PglHmc's by PGL_AIS_FIELDS.  (Not pgl_hmc_view(st, R, P): the scalar blocks start behind NVEC arrays, and NVEC differs.)
__host__ __device__ inline HmcView pgl_ais_hmc_view(const AisView& a)
{
    HmcView v;
    v.M = a.R; v.P = a.P;
    v.q = a.q; v.p = a.p; v.q0 = a.q0; v.g = a.g;
    v.sc = a.sc;
    return v;
}
__device__ __forceinline__ void pgl_ais_load(const AisView& v, int r, PglAis* s)
{
#define PGL_AIS_LD(name, k) s->name = v.sc[(size_t)k * v.R + r];
    PGL_AIS_FIELDS(PGL_AIS_LD)
#undef PGL_AIS_LD
}
__device__ __forceinline__ void pgl_ais_store(const AisView& v, int r, const PglAis* s)
{
#define PGL_AIS_ST(name, k) v.sc[(size_t)k * v.R + r] = s->name;
    PGL_AIS_FIELDS(PGL_AIS_ST)
#undef PGL_AIS_ST
}

// gu = grad U_beta of one row x = [bias, w_stim, w_ir] from gll = grad ll (left as it is), with the rules of pglm_hmc.h;
// returns the log prior, summed in a fixed order, in every thread.  Whole block of 256 threads; every entry of gu is
// written and then finished by the same thread.
__device__ __forceinline__ double pgl_ais_target_row(const double* __restrict__ x, const double* __restrict__ gll,
                                                     double* __restrict__ gu, const double beta, const BfgsPrior& q,
                                                     double* red, const int tid)
{
    double lp = 0.0;
    if (tid == 0) {
        double d;
        lp += pgl_hmc_prior_bias(x[0], q.mu_b, q.sg_b, &d);
        gu[0] = pgl_hmc_grad_elem(pgl_ais_scaled(beta, gll[0]), d);
    }
    for (int c = 1 + tid; c < 1 + q.Dstim; c += 256) {
        double d;
        lp += pgl_hmc_prior_stim(x[c], q.stim_sigma, &d);
        gu[c] = pgl_hmc_grad_elem(pgl_ais_scaled(beta, gll[c]), d);
    }
    const int o = 1 + q.Dstim;
    for (int n = tid; n < q.N; n += 256) {                                     // one presynaptic group per thread
        for (int b = 0; b < q.B; ++b) gu[o + n * q.B + b] = pgl_ais_scaled(beta, gll[o + n * q.B + b]);
        lp += pgl_hmc_prior_group(0, x + o + n * q.B, q.B, q.mu, q.sigma, q.lam, gu + o + n * q.B);
    }
    return pgl_blk_sum(lp, red);
}

// the prior draw of every row into the state and into Xt (the points to evaluate); log w = 0, beta = 0, t = 1
__global__ __launch_bounds__(256) void k_ais_init(const AisView v, double* __restrict__ Xt, const BfgsPrior q, const int n_lo,
                                                  const int particle0, const double step0, const unsigned long long seed)
{
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    PglAis s;
    pgl_ais_init(&s, step0, n_lo + r % v.M, (long long)particle0 + r / v.M, seed);
    const pgl_hmc_u64 key = pgl_hmc_key(pgl_hmc_seed(&s.h), (pgl_hmc_u64)s.h.neuron, 0);
    for (int c = tid; c < P; c += 256) {
        const double x = pgl_ais_draw(pgl_ais_prior_mean(c, q.Dstim, q.mu_b, q.mu),
                                      pgl_ais_prior_sd(c, q.Dstim, q.sg_b, q.stim_sigma, q.sigma), pgl_hmc_normal(key, (pgl_hmc_u64)c));
        v.q[o + c] = x;
        Xt[o + c] = x;
    }
    if (tid == 0) pgl_ais_store(v, r, &s);
}

// (ll, grad) = ll and its gradient at the draws, row by row (left as they are): kept as ll0, gll; lp0; U and grad U at
// beta = 0
__global__ __launch_bounds__(256) void k_ais_start(const AisView v, const double* __restrict__ ll, const double* __restrict__ grad,
                                                   const BfgsPrior q)
{
    __shared__ double red[12];
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    for (int c = tid; c < P; c += 256) v.gll[o + c] = grad[o + c];
    const double lp = pgl_ais_target_row(v.q + o, grad + o, v.g + o, 0.0, q, red, tid);
    if (tid == 0) {
        PglAis s;
        pgl_ais_load(v, r, &s);
        pgl_ais_keep(&s, ll[r], lp);
        s.h.U0 = pgl_ais_energy(0.0, s.ll0, s.lp0);
        pgl_ais_store(v, r, &s);
    }
}

// temperature change: log w += (beta - beta_old) ll0, the target becomes U_beta (U0 and g from ll0, lp0, gll: no
// evaluation), and the row's step becomes step_row[neuron of the row] unless step_row is null
__global__ __launch_bounds__(256) void k_ais_temper(const AisView v, const BfgsPrior q, const double beta,
                                                    const double* __restrict__ step_row)
{
    __shared__ double red[12];
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    pgl_ais_target_row(v.q + o, v.gll + o, v.g + o, beta, q, red, tid);
    if (tid == 0) {
        PglAis s;
        pgl_ais_load(v, r, &s);
        pgl_ais_temper(&s, beta);
        if (step_row) s.h.step = step_row[r % v.M];
        pgl_ais_store(v, r, &s);
    }
}

// end of a transition: H1 from ll1, lp1 (ll and the log prior at q) and ks, the decision (*dec, shared), the step-size rule
// if adapt, t += 1; acc_out[row] += the decision and step_out[row] = the row's step after it (null: none); then accept
// (ll, the log prior, grad ll = grad_row and grad U = gu of the new point are kept) or restore q0
__device__ __forceinline__ void pgl_ais_finish_row(const AisView& v, const int r, const double ll1, const double lp1,
                                                   const double ks, const double* grad_row, const int adapt, double* acc_out,
                                                   double* step_out, int* dec, const int tid)
{
    const size_t o = (size_t)r * v.P;
    if (tid == 0) {
        PglAis s;
        pgl_ais_load(v, r, &s);
        const double u = pgl_hmc_accept_uniform(pgl_hmc_row_key(&s.h));
        *dec = pgl_ais_decide(&s, ll1, lp1, ks, u, adapt);
        pgl_ais_store(v, r, &s);
        if (acc_out) acc_out[r] += (double)*dec;
        if (step_out) step_out[r] = s.h.step;
    }
    __syncthreads();
    if (*dec != 0) {
        for (int c = tid; c < v.P; c += 256) {
            v.g[o + c] = v.gu[o + c];
            v.gll[o + c] = grad_row[c];
        }
    } else {
        for (int c = tid; c < v.P; c += 256) v.q[o + c] = v.q0[o + c];
    }
}

// One leapfrog step of every row after the evaluation of all rows at Xt = q: (ll, grad) come in and are left as they are.
// last == 0: full kick, next drift, Xt[row] = the next point.  last != 0: half kick, H1, the decision (on accept ll, the
// log prior, grad ll and grad U of the new point are kept), the step-size rule if adapt, t += 1; acc_out[row] += the
// decision and step_out[row] = the row's step after it (null: none).
// GUARD (k_smc_leap, pglm_smc.hip.h): done (M), one flag per neuron; a row of a done neuron moves nothing, advances no t and
// (last == 0) writes its current q to Xt.
template <int GUARD>
__device__ __forceinline__ void pgl_ais_leap_row(const AisView& v, const double* __restrict__ minv, const double* __restrict__ ll,
                                                 const double* __restrict__ grad, const BfgsPrior& q, const int last,
                                                 const int adapt, double* __restrict__ Xt, double* __restrict__ acc_out,
                                                 double* __restrict__ step_out, const double* __restrict__ done, double* red,
                                                 int* dec)
{
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P, om = (size_t)(r % v.M) * P;
    if (GUARD && done[r % v.M] != 0.0) {
        if (!last)
            for (int c = tid; c < P; c += 256) Xt[o + c] = v.q[o + c];
        return;
    }
    const double beta = v.sc[(size_t)12 * v.R + r];
    const double lp1 = pgl_ais_target_row(v.q + o, grad + o, v.gu + o, beta, q, red, tid);
    __syncthreads();                                                           // grad U of the row is in memory
    const double step = v.sc[(size_t)2 * v.R + r];
    if (!last) {
        for (int c = tid; c < P; c += 256) {
            const double mi = minv ? minv[om + c] : 1.0;
            const double p = pgl_hmc_kick(v.p[o + c], 1.0, step, v.gu[o + c]);
            const double qn = pgl_hmc_drift(v.q[o + c], step, mi, p);
            v.p[o + c] = p;
            v.q[o + c] = qn;
            Xt[o + c] = qn;
        }
        return;
    }
    const double ks = pgl_hmc_end_kinetic<0>(v.p + o, v.gu + o, minv ? minv + om : nullptr, step, P, red, tid);
    pgl_ais_finish_row(v, r, ll[r], lp1, ks, grad + o, adapt, acc_out, step_out, dec, tid);
}
__global__ __launch_bounds__(256) void k_ais_leap(const AisView v, const double* __restrict__ minv, const double* __restrict__ ll,
                                                  const double* __restrict__ grad, const BfgsPrior q, const int last,
                                                  const int adapt, double* __restrict__ Xt, double* __restrict__ acc_out,
                                                  double* __restrict__ step_out)
{
    __shared__ double red[12];
    __shared__ int dec;
    pgl_ais_leap_row<0>(v, minv, ll, grad, q, last, adapt, Xt, acc_out, step_out, nullptr, red, &dec);
}
