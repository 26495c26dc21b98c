// lock-step HMC row kernels: k_hmc_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// Lock-step Hamiltonian Monte Carlo (inference/batched_hmc.py): the chains of all M neurons of a range -- one workgroup
// per neuron row -- around the one launch that does the work: a fused ll+grad evaluation of all rows per leapfrog step
// (pgl_ll_grad_dev).  The algorithm, its random numbers and its decisions are pglm_hmc.h (Neal 2011 fig. 2 as
// inference/hmc.py states it; compiled for the host by tests/csrc/hmc_host.c); these kernels own the vectors, the
// fixed-order reductions (pgl_blk_sum: wave64 butterflies, then the four waves through LDS), the priors' part of U and
// its gradient and the NaN rules.  All state lives in ONE device block of doubles laid out by pgl_hmc_view.  Every row
// takes the same number of steps: no lists, no flags, nothing for the host to read before the chain has ended.
// ---------------------------------------------------------------------------
#include "pglm_hmc_dense.h"                     // (pglm_hmc.h, and the dense chain's per-element rules)
#include "pglm_adapt.h"                         // (pgl_chain_seed)

struct HmcView {
    int M, P;
    double *q, *p, *q0, *g;                   // (M, P): point, momentum, start of the transition, grad U at the accepted point
    double* sc;                               // (PGL_HMC_NSCAL, M): PglHmc, field-major
};
__host__ __device__ inline size_t pgl_hmc_doubles(int M, int P)
{
    return (size_t)M * P * PGL_HMC_NVEC + (size_t)M * PGL_HMC_NSCAL;
}
__host__ __device__ inline HmcView pgl_hmc_view(double* st, int M, int P)
{
    HmcView v;
    const size_t MP = (size_t)M * P;
    v.M = M; v.P = P;
    v.q = st; v.p = st + MP; v.q0 = st + 2 * MP; v.g = st + 3 * MP;
    v.sc = st + PGL_HMC_NVEC * MP;
    return v;
}
// (IN: the fields as members of IN -- empty here, `h.` for the PglHmc at the head of PglAis, whose rows are these)
#define PGL_HMC_FIELDS_IN(F, IN) F(IN U0, 0) F(IN H0, 1) F(IN step, 2) F(IN avg_accept, 3) F(IN n_accept, 4) F(IN t, 5) \
    F(IN acc, 6) F(IN neuron, 7) F(IN seed_lo, 8) F(IN seed_hi, 9)
#define PGL_HMC_FIELDS(F) PGL_HMC_FIELDS_IN(F, )
__device__ __forceinline__ void pgl_hmc_load(const HmcView& v, int r, PglHmc* s)
{
#define PGL_HMC_LD(name, k) s->name = v.sc[(size_t)k * v.M + r];
    PGL_HMC_FIELDS(PGL_HMC_LD)
#undef PGL_HMC_LD
}
__device__ __forceinline__ void pgl_hmc_store(const HmcView& v, int r, const PglHmc* s)
{
#define PGL_HMC_ST(name, k) v.sc[(size_t)k * v.M + r] = s->name;
    PGL_HMC_FIELDS(PGL_HMC_ST)
#undef PGL_HMC_ST
}

// U = -(ll + log prior) and grad U of one row x = [bias, w_stim, w_ir] with the rules of pglm_hmc.h, in place: g (grad ll)
// -> grad U; returns U in every thread.  Whole block of 256 threads; the log prior is summed in a fixed order.
__device__ __forceinline__ double pgl_hmc_target_row(const double* __restrict__ x, double* __restrict__ g, const double ll,
                                                     const BfgsPrior& q, double* red, const int tid)
{
    double lp = 0.0;
    if (tid == 0) {
        double d;
        lp += pgl_hmc_prior_bias(x[0], q.mu_b, q.sg_b, &d);
        g[0] = pgl_hmc_grad_elem(g[0], d);
    }
    for (int c = 1 + tid; c < 1 + q.Dstim; c += 256) {
        double d;
        lp += pgl_hmc_prior_stim(x[c], q.stim_sigma, &d);
        g[c] = pgl_hmc_grad_elem(g[c], d);
    }
    const int o = 1 + q.Dstim;
    for (int n = tid; n < q.N; n += 256)                                       // one presynaptic group per thread
        lp += pgl_hmc_prior_group(q.kind, x + o + n * q.B, q.B, q.mu, q.sigma, q.lam, g + o + n * q.B);
    const double lpt = pgl_blk_sum(lp, red);
    return pgl_hmc_energy(ll, lpt);
}

// start of a chain: q of every row is in the state, (ll, grad) hold ll and its gradient at q, row by row (overwritten
// with U and grad U).  chain_rows: the rows of one chain -- row r is chain r / chain_rows of neuron n_lo + r % chain_rows
// and runs on pgl_chain_seed(seed, chain) (one chain: chain_rows = M, the seed itself)
__global__ __launch_bounds__(256) void k_hmc_init(const HmcView v, double* __restrict__ ll, double* __restrict__ grad,
                                                  const BfgsPrior q, const int n_lo, const double step0,
                                                  const unsigned long long seed, const int chain_rows)
{
    __shared__ double red[12];
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    const double U = pgl_hmc_target_row(v.q + o, grad + o, ll[r], q, red, tid);
    __syncthreads();                                                           // grad U of the row is in memory
    for (int c = tid; c < P; c += 256) v.g[o + c] = grad[o + c];
    if (tid == 0) {
        PglHmc s;
        pgl_hmc_init(&s, U, step0, n_lo + r % chain_rows, pgl_chain_seed(seed, (pgl_hmc_u64)(r / chain_rows)));
        pgl_hmc_store(v, r, &s);
        ll[r] = U;
    }
}

// start of a transition: momentum, H0, the half kick with grad U at q, the first drift; Xt[row] = the point to evaluate.
// minv (minv_rows, P): row r runs on row r mod minv_rows (the chain: minv_rows = M; the K M rows of an annealed importance
// sampling run, particle-major, share the M rows of their neurons).
// GUARD (k_smc_begin, pglm_smc.hip.h): done (minv_rows), one flag per neuron; a row of a done neuron draws nothing, moves
// nothing and writes its current q to Xt.
template <int GUARD>
__device__ __forceinline__ void pgl_hmc_begin_row(const HmcView& v, const double* __restrict__ minv, const int minv_rows,
                                                  double* __restrict__ Xt, const double* __restrict__ done, double* red)
{
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P, om = (size_t)(r % minv_rows) * P;
    if (GUARD && done[r % minv_rows] != 0.0) {
        for (int c = tid; c < P; c += 256) Xt[o + c] = v.q[o + c];
        return;
    }
    PglHmc s;
    pgl_hmc_load(v, r, &s);
    const pgl_hmc_u64 key = pgl_hmc_row_key(&s);
    double ks = 0.0;
    for (int c = tid; c < P; c += 256) {
        const double mi = minv ? minv[om + c] : 1.0;
        const double q0 = v.q[o + c];
        double p = pgl_hmc_momentum(pgl_hmc_normal(key, (pgl_hmc_u64)c), mi);
        ks += pgl_hmc_kinetic_elem(p, mi);
        p = pgl_hmc_kick(p, 0.5, s.step, v.g[o + c]);
        const double qn = pgl_hmc_drift(q0, s.step, mi, p);
        v.q0[o + c] = q0;
        v.p[o + c] = p;
        v.q[o + c] = qn;
        Xt[o + c] = qn;
    }
    ks = pgl_blk_sum(ks, red);
    if (tid == 0) {
        pgl_hmc_begin(&s, ks);
        v.sc[(size_t)1 * v.M + r] = s.H0;
    }
}
__global__ __launch_bounds__(256) void k_hmc_begin(const HmcView v, const double* __restrict__ minv, const int minv_rows,
                                                   double* __restrict__ Xt)
{
    __shared__ double red[12];
    pgl_hmc_begin_row<0>(v, minv, minv_rows, Xt, nullptr, red);
}

// ---- the end of a transition, shared by the diagonal and the dense kernels of the chain and of annealed importance sampling ----
// The kinetic sum of one row (p, gu, minv: the row's P entries) in every thread.  DENSE 0: the last half kick p -= step/2 gu
// first (p is rewritten), then sum p^2 minv (minv null: 1).  DENSE 1: p holds the whitened momentum, kicked by the product
// already: sum r^2.
template <int DENSE>
__device__ __forceinline__ double pgl_hmc_end_kinetic(double* p, const double* gu, const double* minv, const double step,
                                                      const int P, double* red, const int tid)
{
    double ks = 0.0;
    for (int c = tid; c < P; c += 256) {
        if (DENSE) ks += pgl_hmcd_kinetic_elem(p[c]);
        else {
            const double mi = minv ? minv[c] : 1.0;
            const double pc = pgl_hmc_kick(p[c], 0.5, step, gu[c]);
            p[c] = pc;
            ks += pgl_hmc_kinetic_elem(pc, mi);
        }
    }
    return pgl_blk_sum(ks, red);
}
// H1 from U1 and ks, the decision (*dec, shared), the step-size rule while t < n_warmup, t += 1; then accept (grad_row, grad
// U of the new point, is kept) or restore q0, and the row's point into sample_out[row] (null: none)
__device__ __forceinline__ void pgl_hmc_finish_row(const HmcView& v, const int r, const double U1, const double ks,
                                                   const double* grad_row, const int n_warmup, double* sample_out, int* dec,
                                                   const int tid)
{
    const size_t o = (size_t)r * v.P;
    if (tid == 0) {
        PglHmc s;
        pgl_hmc_load(v, r, &s);
        const double u = pgl_hmc_accept_uniform(pgl_hmc_row_key(&s));
        *dec = pgl_hmc_decide(&s, U1, ks, u, n_warmup);
        pgl_hmc_store(v, r, &s);
    }
    __syncthreads();
    const bool acc = *dec != 0;
    for (int c = tid; c < v.P; c += 256) {
        double qc;
        if (acc) {
            qc = v.q[o + c];
            v.g[o + c] = grad_row[c];
        } else {
            qc = v.q0[o + c];
            v.q[o + c] = qc;
        }
        if (sample_out) sample_out[o + c] = qc;
    }
}

// One leapfrog step of every row after ONE evaluation of all rows at Xt = q: (ll, grad) come in and are turned into U,
// grad U in place.  last == 0: full kick, next drift, Xt[row] = the next point.  last != 0: half kick, H1, the decision,
// the step-size rule while t < n_warmup, t += 1, and the row's current point into sample_out[row] (null: none).
__global__ __launch_bounds__(256) void k_hmc_leap(const HmcView v, const double* __restrict__ minv, double* __restrict__ ll,
                                                  double* __restrict__ grad, const BfgsPrior q, const int last,
                                                  const int n_warmup, double* __restrict__ Xt, double* __restrict__ sample_out)
{
    __shared__ double red[12];
    __shared__ int dec;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    const double U1 = pgl_hmc_target_row(v.q + o, grad + o, ll[r], q, red, tid);
    __syncthreads();                                                           // grad U of the row is in memory
    const double step = v.sc[(size_t)2 * v.M + r];
    if (!last) {
        for (int c = tid; c < P; c += 256) {
            const double mi = minv ? minv[o + c] : 1.0;
            const double p = pgl_hmc_kick(v.p[o + c], 1.0, step, grad[o + c]);
            const double qn = pgl_hmc_drift(v.q[o + c], step, mi, p);
            v.p[o + c] = p;
            v.q[o + c] = qn;
            Xt[o + c] = qn;
        }
        if (tid == 0) ll[r] = U1;
        return;
    }
    const double ks = pgl_hmc_end_kinetic<0>(v.p + o, grad + o, minv ? minv + o : nullptr, step, P, red, tid);
    if (tid == 0) ll[r] = U1;
    pgl_hmc_finish_row(v, r, U1, ks, grad + o, n_warmup, sample_out, &dec, tid);
}
