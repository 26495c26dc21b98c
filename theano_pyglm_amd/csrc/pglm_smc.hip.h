// adaptive sequential Monte Carlo of the per-neuron evidence: k_smc_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// The tempered path of pglm_ais.hip.h walked by a sequential Monte Carlo sampler (inference/batched_smc.py): every neuron
// chooses its next temperature from its own particles, degenerate particle sets are resampled, and the step size is
// adapted from the particle population.  The rows are the AIS rows (r = k M + i, particle-major, the AIS state block); the
// rules are pglm_smc.h (compiled for the host by tests/csrc/smc_host.c).  What is new here is the step that couples the K
// particles of a neuron:
//   k_smc_stage     one workgroup per NEURON, threads strided over its particles (any K >= 1): step rule, bisection for
//                   the next temperature, evidence, weights, ESS, the resampling decision and the ancestors, the record.
//   k_smc_gather    one workgroup per row: q, gll, ll0, lp0 of the row's ancestor into scratch (out of place: no row
//                   reads a slot that another workgroup is overwriting).
//   k_smc_retemper  one workgroup per row: scratch into the row, U0 and g at the neuron's new beta (pgl_ais_target_row),
//                   the row's step = the neuron's; workgroup 0 also counts the neurons that are not done.
// The moves are the bodies of the AIS kernels instantiated with a guard on the neuron's done flag (k_smc_begin, k_smc_leap,
// k_smc_dense_draw, k_smc_tri_matvec_shared, k_smc_dense_target, k_smc_dense_end): a row of a done neuron draws nothing,
// moves nothing, advances no t and writes its current q to Xt; an active row has the bits of the AIS kernel.
// f64, no atomics; every sum over the particles is pgl_blk_sum over per-thread partial sums taken in index order.
// ---------------------------------------------------------------------------
#include "pglm_smc.h"

struct SmcView {
    int K, M, P, S;                           // particles, neurons, parameters, stage records
    double *sc, *rec;                         // (PGL_SMC_NSCAL, M) PglSmc field-major; (PGL_SMC_NREC, S, M)
    double *anc, *w, *acc, *nact;             // (R) each; (1)
    double *tq, *tg, *ts;                     // (R, P), (R, P), (2, R): the gather's scratch
};
__host__ __device__ inline size_t pgl_smc_doubles(size_t K, size_t M, size_t P, size_t S)
{
    const size_t R = K * M;
    return PGL_SMC_NSCAL * M + PGL_SMC_NREC * S * M + 3 * R + 1 + 2 * R * P + 2 * R;
}
__host__ __device__ inline SmcView pgl_smc_view(double* st, int K, int M, int P, int S)
{
    SmcView v;
    const size_t R = (size_t)K * M;
    v.K = K; v.M = M; v.P = P; v.S = S;
    v.sc = st;
    v.rec = v.sc + (size_t)PGL_SMC_NSCAL * M;
    v.anc = v.rec + (size_t)PGL_SMC_NREC * S * M;
    v.w = v.anc + R; v.acc = v.w + R; v.nact = v.acc + R;
    v.tq = v.nact + 1; v.tg = v.tq + R * P; v.ts = v.tg + R * P;
    return v;
}
#define PGL_SMC_FIELDS(F) F(beta, 0) F(log_Z, 1) F(step, 2) F(stage, 3) F(done, 4) F(n_resampled, 5) F(acc, 6) F(live, 7) \
    F(rs, 8) F(ess, 9)
#define PGL_SMC_F_DONE 4
#define PGL_SMC_F_LIVE 7
#define PGL_SMC_F_RS 8
__device__ __forceinline__ void pgl_smc_load(const SmcView& v, int i, PglSmc* s)
{
#define PGL_SMC_LD(name, k) s->name = v.sc[(size_t)k * v.M + i];
    PGL_SMC_FIELDS(PGL_SMC_LD)
#undef PGL_SMC_LD
}
__device__ __forceinline__ void pgl_smc_store(const SmcView& v, int i, const PglSmc* s)
{
#define PGL_SMC_ST(name, k) v.sc[(size_t)k * v.M + i] = s->name;
    PGL_SMC_FIELDS(PGL_SMC_ST)
#undef PGL_SMC_ST
}
__device__ __forceinline__ void pgl_smc_record(const SmcView& v, int i, int stage, double beta, double ess, double cess,
                                               double rs, double step)
{
    if (stage >= v.S) return;
    const size_t SM = (size_t)v.S * v.M, o = (size_t)stage * v.M + i;
    v.rec[PGL_SMC_R_BETA * SM + o] = beta;
    v.rec[PGL_SMC_R_ESS * SM + o] = ess;
    v.rec[PGL_SMC_R_CESS * SM + o] = cess;
    v.rec[PGL_SMC_R_RS * SM + o] = rs;
    v.rec[PGL_SMC_R_ACC * SM + o] = (double)NAN;
    v.rec[PGL_SMC_R_STEP * SM + o] = step;
}

// the start of the per-neuron block: beta = 0, log_Z = 0, the step, no records, identity ancestors, equal weights
__global__ __launch_bounds__(256) void k_smc_init(const SmcView m, const double step0)
{
    const int i = blockIdx.x, tid = threadIdx.x, K = m.K, M = m.M;
    for (int e = tid; e < PGL_SMC_NREC * m.S; e += 256) m.rec[(size_t)e * M + i] = (double)NAN;
    for (int k = tid; k < K; k += 256) {
        const size_t r = (size_t)k * M + i;
        m.anc[r] = (double)k;
        m.w[r] = 1.0 / (double)K;
        m.acc[r] = 0.0;
    }
    if (tid == 0) {
        PglSmc s;
        pgl_smc_init(&s, step0);
        pgl_smc_store(m, i, &s);
        if (i == 0) m.nact[0] = (double)M;
    }
}

// s1 = sum W v, s2 = sum W v^2 over the particles of neuron i at the temperature step d, in every thread
__device__ __forceinline__ void pgl_smc_cess_sums(const SmcView& m, const double* __restrict__ ll0, const int i, const double d,
                                                  const double ll_max, double& s1, double& s2, double* red, const int tid)
{
    s1 = 0.0; s2 = 0.0;
    double c = 0.0;
    for (int k = tid; k < m.K; k += 256) {
        const size_t r = (size_t)k * m.M + i;
        const double W = m.w[r];
        if (W > 0.0) {
            const double vv = pgl_smc_v(d, ll0[r], ll_max);
            s1 += W * vv;
            s2 += W * vv * vv;
        }
    }
    pgl_blk_sum3(s1, s2, c, red);
}

// One stage of every neuron that is not done (pglm_smc.h, steps 0 to 3): reads ll0 and logw of the neuron's rows, writes
// logw, the neuron's scalars, its record, w (normalised weights before resampling) and anc; clears acc.
__global__ __launch_bounds__(256) void k_smc_stage(const AisView v, const SmcView m, const int n_steps, const double rho,
                                                   const double ess_min, const double delta_min, const unsigned long long seed)
{
    __shared__ double red[12];
    __shared__ int last_live;
    const int i = blockIdx.x, tid = threadIdx.x, K = m.K, M = m.M;
    const size_t R = (size_t)v.R;
    const double* ll0 = v.sc + 10 * R;
    double* logw = v.sc + 13 * R;
    PglSmc s;
    pgl_smc_load(m, i, &s);
    if (s.done != 0.0) {                                                       // never changes again
        if (tid == 0) {
            m.sc[(size_t)PGL_SMC_F_LIVE * M + i] = 0.0;
            m.sc[(size_t)PGL_SMC_F_RS * M + i] = 0.0;
        }
        return;
    }
    const int st = (int)s.stage;
    // 0. the step rule from the acceptances of the moves since the last stage
    double a = 0.0;
    for (int k = tid; k < K; k += 256) {
        const size_t r = (size_t)k * M + i;
        a += m.acc[r];
        m.acc[r] = 0.0;
    }
    a = pgl_blk_sum(a, red);
    s.acc = a;
    if (st > 0) {
        const double rate = a / ((double)K * (double)n_steps);
        s.step = pgl_smc_step_rule(s.step, rate);
        if (tid == 0 && st - 1 < m.S) m.rec[((size_t)PGL_SMC_R_ACC * m.S + (st - 1)) * M + i] = rate;
    }
    // the weights W_k from logw; the largest ll0 of the live particles
    double mlw = -(double)INFINITY, mll = -(double)INFINITY;
    for (int k = tid; k < K; k += 256) {
        const size_t r = (size_t)k * M + i;
        if (pgl_smc_alive(ll0[r], logw[r])) {
            mlw = fmax(mlw, logw[r]);
            mll = fmax(mll, ll0[r]);
        }
    }
    mlw = pgl_blk_max(mlw, red);
    mll = pgl_blk_max(mll, red);
    double es = 0.0;
    for (int k = tid; k < K; k += 256) {
        const size_t r = (size_t)k * M + i;
        const double e = pgl_smc_alive(ll0[r], logw[r]) ? exp(logw[r] - mlw) : 0.0;
        m.w[r] = e;
        es += e;
    }
    es = pgl_blk_sum(es, red);
    for (int k = tid; k < K; k += 256) {
        const size_t r = (size_t)k * M + i;
        m.w[r] = es > 0.0 ? m.w[r] / es : 0.0;
    }
    // 1. the next temperature
    const double rem = 1.0 - s.beta, target = rho * (double)K;
    double s1 = 0.0, s2 = 0.0, d = rem, beta_new = 1.0;
    if (es > 0.0) {
        pgl_smc_cess_sums(m, ll0, i, rem, mll, s1, s2, red, tid);
        double lo = rem;
        if (!(pgl_smc_cess(K, s1, s2) >= target)) {
            double hi = rem;
            lo = 0.0;
            for (int it = 0; it < PGL_SMC_BISECT; ++it) {
                const double mid = 0.5 * (lo + hi);
                pgl_smc_cess_sums(m, ll0, i, mid, mll, s1, s2, red, tid);
                if (pgl_smc_cess(K, s1, s2) >= target) lo = mid;
                else hi = mid;
            }
        }
        d = pgl_smc_delta(lo, delta_min, s.beta, &beta_new);
        pgl_smc_cess_sums(m, ll0, i, d, mll, s1, s2, red, tid);
    }
    if (!(es > 0.0) || !(s1 > 0.0)) {                                          // no live particle: the evidence is 0
        for (int k = tid; k < K; k += 256) {
            const size_t r = (size_t)k * M + i;
            logw[r] = -(double)INFINITY;
            m.w[r] = 0.0;
            m.anc[r] = (double)k;
        }
        if (tid == 0) {
            s.log_Z = -(double)INFINITY;
            s.done = 1.0; s.live = 0.0; s.rs = 0.0; s.ess = 0.0;
            pgl_smc_record(m, i, st, s.beta, 0.0, 0.0, 0.0, s.step);
            s.stage += 1.0;
            pgl_smc_store(m, i, &s);
        }
        return;
    }
    // 2. evidence and weights
    const double cess = pgl_smc_cess(K, s1, s2), ls1 = log(s1), les = log(es);
    s.log_Z += d * mll + ls1;
    double q2 = 0.0;
    for (int k = tid; k < K; k += 256) {
        const size_t r = (size_t)k * M + i;
        const double W = m.w[r];
        double Wn = 0.0, lw = -(double)INFINITY;
        if (W > 0.0) {
            Wn = W * pgl_smc_v(d, ll0[r], mll) / s1;
            lw = ((logw[r] - mlw) - les) + d * (ll0[r] - mll) - ls1;
        }
        m.w[r] = Wn;
        logw[r] = lw;
        q2 += Wn * Wn;
    }
    q2 = pgl_blk_sum(q2, red);
    const double ess = 1.0 / q2;
    // 3. resampling
    const int rs = ess < ess_min * (double)K;
    if (rs) {
        // (the cumulative sums in index order by ONE thread: K independent loads at stride M and K dependent adds, once per
        // resampling stage -- a fixed order by construction; a latency tail that grows with K and has not been measured
        // beyond K = 300)
        double* cum = m.ts + i;                                                // (K) at stride M: free until the gather
        if (tid == 0) {
            double c = 0.0;
            int ll = 0;
            for (int k = 0; k < K; ++k) {
                const double W = m.w[(size_t)k * M + i];
                c += W;
                cum[(size_t)k * M] = c;
                if (W > 0.0) ll = k;
            }
            last_live = ll;
        }
        __syncthreads();
        const double u = pgl_smc_uniform(seed, (pgl_hmc_u64)v.sc[7 * R + i], (pgl_hmc_u64)st);
        for (int k = tid; k < K; k += 256) {
            const size_t r = (size_t)k * M + i;
            int j = pgl_smc_search(cum, (long)M, K, pgl_smc_position(u, k, K));
            if (!(m.w[(size_t)j * M + i] > 0.0)) j = last_live;
            m.anc[r] = (double)j;
            logw[r] = 0.0;
        }
    } else {
        for (int k = tid; k < K; k += 256) m.anc[(size_t)k * M + i] = (double)k;
    }
    if (tid == 0) {
        pgl_smc_record(m, i, st, beta_new, ess, cess, (double)rs, s.step);
        s.beta = beta_new;
        s.stage += 1.0;
        s.done = beta_new == 1.0 ? 1.0 : 0.0;
        s.n_resampled += (double)rs;
        s.live = 1.0; s.rs = (double)rs; s.ess = ess;
        pgl_smc_store(m, i, &s);
    }
}

// the kept parts of the row's ancestor into the scratch: only where the neuron resampled in this stage
__global__ __launch_bounds__(256) void k_smc_gather(const AisView v, const SmcView m)
{
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P, i = r % m.M;
    if (m.sc[(size_t)PGL_SMC_F_LIVE * m.M + i] == 0.0 || m.sc[(size_t)PGL_SMC_F_RS * m.M + i] == 0.0) return;
    const size_t R = (size_t)v.R, src = (size_t)m.anc[r] * m.M + i, o = (size_t)r * P, os = src * P;
    for (int c = tid; c < P; c += 256) {
        m.tq[o + c] = v.q[os + c];
        m.tg[o + c] = v.gll[os + c];
    }
    if (tid == 0) {
        m.ts[r] = v.sc[10 * R + src];
        m.ts[R + r] = v.sc[11 * R + src];
    }
}

// the scratch into the row (where the neuron resampled), then the new target: beta, U0 and g from the kept parts, the row's
// step = the neuron's.  Rows of a neuron the stage did not touch stay as they are.  Workgroup 0 counts the unfinished.
__global__ __launch_bounds__(256) void k_smc_retemper(const AisView v, const SmcView m, const BfgsPrior q)
{
    __shared__ double red[12];
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P, i = r % m.M;
    if (r == 0) {
        double c = 0.0;
        for (int j = tid; j < m.M; j += 256) c += m.sc[(size_t)PGL_SMC_F_DONE * m.M + j] == 0.0 ? 1.0 : 0.0;
        c = pgl_blk_sum(c, red);
        if (tid == 0) m.nact[0] = c;
        __syncthreads();
    }
    if (m.sc[(size_t)PGL_SMC_F_LIVE * m.M + i] == 0.0) return;
    const int rs = m.sc[(size_t)PGL_SMC_F_RS * m.M + i] != 0.0;
    const size_t R = (size_t)v.R, o = (size_t)r * P;
    if (rs) {
        for (int c = tid; c < P; c += 256) {
            v.q[o + c] = m.tq[o + c];
            v.gll[o + c] = m.tg[o + c];
        }
        __syncthreads();
    }
    const double beta = m.sc[i];
    pgl_ais_target_row(v.q + o, v.gll + o, v.g + o, beta, q, red, tid);
    if (tid == 0) {
        PglAis s;
        pgl_ais_load(v, r, &s);
        if (rs) pgl_ais_keep(&s, m.ts[r], m.ts[R + r]);
        s.beta = beta;
        s.h.U0 = pgl_ais_energy(beta, s.ll0, s.lp0);
        s.h.step = m.sc[(size_t)2 * m.M + i];
        pgl_ais_store(v, r, &s);
    }
}

// ---- the guarded moves: the AIS kernels' bodies, rows of a done neuron passed by ----
__global__ __launch_bounds__(256) void k_smc_begin(const HmcView v, const double* __restrict__ minv, const int M,
                                                   double* __restrict__ Xt, const double* __restrict__ done)
{
    __shared__ double red[12];
    pgl_hmc_begin_row<1>(v, minv, M, Xt, done, red);
}
__global__ __launch_bounds__(256) void k_smc_leap(const AisView v, const double* __restrict__ minv, const double* __restrict__ ll,
                                                  const double* __restrict__ grad, const BfgsPrior q, const int last,
                                                  double* __restrict__ Xt, double* __restrict__ acc_out,
                                                  const double* __restrict__ done)
{
    __shared__ double red[12];
    __shared__ int dec;
    pgl_ais_leap_row<1>(v, minv, ll, grad, q, last, 0, Xt, acc_out, nullptr, done, red, &dec);
}
__global__ __launch_bounds__(256) void k_smc_dense_draw(const HmcView v, const double* __restrict__ done, const int M)
{
    __shared__ double red[12];
    pgl_hmc_dense_draw_row<1>(v, done, M, red);
}
template <int TRANS, int EPI, int KC>
__global__ __launch_bounds__(256) void k_smc_tri_matvec_shared(const double* __restrict__ W, const double* __restrict__ x,
                                                               const int K, const int M, const int P, double* __restrict__ y,
                                                               double* __restrict__ Xt, const double* __restrict__ step,
                                                               const double scale, const double* __restrict__ done)
{
    __shared__ double part[KC][TRANS ? 4 : 1][PGL_TRI_TILE];
    pgl_tri_matvec_shared_body<TRANS, EPI, KC, 1>(W, x, K, M, P, y, Xt, step, scale, done, part);
}
__global__ __launch_bounds__(256) void k_smc_dense_target(const AisView v, const double* __restrict__ grad, const BfgsPrior q,
                                                          const double* __restrict__ done)
{
    __shared__ double red[12];
    if (done[blockIdx.x % v.M] != 0.0) return;
    pgl_ais_dense_target_row(v, grad, q, red);
}
__global__ __launch_bounds__(256) void k_smc_dense_end(const AisView v, const double* __restrict__ ll,
                                                       const double* __restrict__ grad, const BfgsPrior q,
                                                       double* __restrict__ acc_out, const double* __restrict__ done)
{
    __shared__ double red[12];
    __shared__ int dec;
    if (done[blockIdx.x % v.M] != 0.0) return;
    pgl_ais_dense_end_row(v, ll, grad, q, 0, acc_out, nullptr, red, &dec);
}
