// lock-step proximal gradient row kernels: k_prox_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// Lock-step accelerated proximal gradient for the group-lasso MAP (inference/batched_prox.py): the FISTA state machines
// of all M neurons of a range -- one workgroup per neuron row -- around the one launch that does the work: a fused ll+grad
// evaluation of all rows per call (pgl_ll_grad_dev).  The algorithm and its decisions are pglm_prox.h (compiled for the
// host by tests/csrc/prox_host.c); these kernels own the vectors, the fixed-order reductions (pgl_blk_sum / _sum3 / _max:
// wave64 butterflies, then the four waves through LDS), the smooth priors' part of f and its gradient and the NaN rules.
// A presynaptic group belongs to ONE thread, which walks its B entries in order: a group norm never crosses a lane, so it
// does not matter where the wave boundaries fall (B need not divide 64) or how often the 256 threads stride over the row
// (P > 256).  All state lives in ONE device block of doubles laid out by pgl_prox_view; a row's scalar state sits in LDS
// while its workgroup runs.  A finished row (phase PGL_PROX_DONE) is frozen: its workgroup returns before it writes
// anything, and its row of Xt holds x.
// ---------------------------------------------------------------------------
#include "pglm_prox.h"

struct ProxView {
    int M, P;
    double *x, *xp, *y, *gx, *gy;             // (M, P): point, previous point, extrapolated point, grad f at x and at y
    double* sc;                               // (PGL_PROX_NSCAL, M): PglProx, field-major
};
__host__ __device__ inline size_t pgl_prox_doubles(int M, int P)
{
    return (size_t)M * P * PGL_PROX_NVEC + (size_t)M * PGL_PROX_NSCAL;
}
__host__ __device__ inline ProxView pgl_prox_view(double* st, int M, int P)
{
    ProxView v;
    const size_t MP = (size_t)M * P;
    v.M = M; v.P = P;
    v.x = st; v.xp = st + MP; v.y = st + 2 * MP; v.gx = st + 3 * MP; v.gy = st + 4 * MP;
    v.sc = st + PGL_PROX_NVEC * MP;
    return v;
}
#define PGL_PROX_FIELDS(F) F(f_x, 0) F(F_x, 1) F(f_y, 2) F(t, 3) F(tk, 4) F(iters, 5) F(nfev, 6) F(nbt, 7) F(restarts, 8) \
    F(phase, 9) F(status, 10) F(kkt, 11) F(y_is_x, 12) F(m_sd, 13) F(m_restart, 14) F(m_zero, 15) F(m_kkt, 16)

// a row's scalar state in LDS for the lifetime of its workgroup
struct ProxRow {
    PglProx s;
    int dec;
    double val;
};
__device__ __forceinline__ void pgl_prox_load(const ProxView& v, int r, PglProx* s)
{
#define PGL_PROX_LD(name, k) s->name = v.sc[(size_t)k * v.M + r];
    PGL_PROX_FIELDS(PGL_PROX_LD)
#undef PGL_PROX_LD
}
__device__ __forceinline__ void pgl_prox_store(const ProxView& v, int r, const PglProx* s)
{
#define PGL_PROX_ST(name, k) v.sc[(size_t)k * v.M + r] = s->name;
    PGL_PROX_FIELDS(PGL_PROX_ST)
#undef PGL_PROX_ST
}
// end of a workgroup that has advanced its row: state back to memory, the row's phase to the driver's pinned flags
__device__ __forceinline__ void pgl_prox_leave(const ProxView& v, int r, const ProxRow* w, double* flags, const int tid)
{
    __syncthreads();
    if (tid == 0) {
        pgl_prox_store(v, r, &w->s);
        if (flags) __hip_atomic_store(flags + r, w->s.phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// f = -(ll + log prior of bias and stimulus weights) and grad f of one row x = [bias, w_stim, w_ir] with the rules of
// pglm_prox.h, in place: g (grad ll) -> grad f; returns f in every thread.  Whole block of 256 threads; the log prior is
// summed in a fixed order.  (Ends behind the barriers of the sum, but g is in memory only after the caller's next barrier.)
__device__ __forceinline__ double pgl_prox_smooth_row(const int P, const double* x, double* g, const double ll,
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
    for (int c = 1 + q.Dstim + tid; c < P; c += 256) g[c] = pgl_hmc_grad_elem(g[c], 0.0);
    return pgl_hmc_energy(ll, pgl_blk_sum(lp, red));
}

// the trial z = prox_{t h}(y - t gy) of one row into xt; returns the smallest threshold margin of its groups in every
// thread.  The caller's last barrier lies behind every write of y and gy and every read of xt.
__device__ __forceinline__ double pgl_prox_emit_row(const double* y, const double* gy, double* xt, const BfgsPrior& q,
                                                    const double t, const double lam_s, double* red, const int tid)
{
    for (int c = tid; c < 1 + q.Dstim; c += 256) xt[c] = pgl_prox_plain_step(y[c], t, gy[c]);
    const int o = 1 + q.Dstim;
    const double thr = t * lam_s;
    double mg = (double)INFINITY;
    for (int n = tid; n < q.N; n += 256) {                                     // one presynaptic group per thread
        double m;
        pgl_prox_group(y + o + n * q.B, gy + o + n * q.B, q.B, t, q.mu, thr, xt + o + n * q.B, &m);
        mg = pgl_prox_min(mg, m);
    }
    return -pgl_blk_max(-mg, red);
}

// the KKT residual of one row at x from g = grad f, in every thread
__device__ __forceinline__ double pgl_prox_kkt_row(const double* x, const double* g, const BfgsPrior& q, const double lam_s,
                                                   double* red, const int tid)
{
    double r = 0.0;
    for (int c = tid; c < 1 + q.Dstim; c += 256) r = fmax(r, fabs(g[c]));
    const int o = 1 + q.Dstim;
    for (int n = tid; n < q.N; n += 256) r = fmax(r, pgl_prox_group_kkt(x + o + n * q.B, g + o + n * q.B, q.B, q.mu, lam_s));
    return pgl_blk_max(r, red);
}

// h of one row (a per-thread partial: the caller sums it)
__device__ __forceinline__ double pgl_prox_h_part(const double* x, const BfgsPrior& q, const double lam_s, const int tid)
{
    const int o = 1 + q.Dstim;
    double h = 0.0;
    for (int n = tid; n < q.N; n += 256) h += pgl_prox_group_h(x + o + n * q.B, q.B, q.mu, lam_s);
    return h;
}

struct ProxArgs {
    double* ll;                               // (M) ll of the evaluated points, overwritten with f
    double* grad;                             // (M, P) its gradient, overwritten with grad f
    BfgsPrior q;                              // (q.lam is not used: lam is per row)
    const double* lam;                        // (M)
    double gtol;
    int maxiter, max_backtrack;
    double* Xt;                               // (M, P) the points to evaluate next
    double* flags;
};

// start of a fit: x of every row is in the state, (ll, grad) hold ll and its gradient at x, row by row
__global__ __launch_bounds__(256) void k_prox_init(const ProxView v, const ProxArgs a)
{
    __shared__ double red[12];
    __shared__ ProxRow w;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    const double* x = v.x + o;
    double* g = a.grad + o;
    double* xt = a.Xt + o;
    const double lam_s = a.lam[r] / a.q.sigma;
    const double f = pgl_prox_smooth_row(P, x, g, a.ll[r], a.q, red, tid);
    __syncthreads();                                                           // grad f of the row is in memory
    double gg = 0.0, hx = pgl_prox_h_part(x, a.q, lam_s, tid), zz = 0.0;
    for (int c = tid; c < P; c += 256) {
        const double gc = g[c], xc = x[c];
        gg = fma(gc, gc, gg);
        v.gx[o + c] = gc;
        v.gy[o + c] = gc;
        v.y[o + c] = xc;
        v.xp[o + c] = xc;
    }
    pgl_blk_sum3(gg, hx, zz, red);
    const double kkt = pgl_prox_kkt_row(x, g, a.q, lam_s, red, tid);
    if (tid == 0) {
        pgl_prox_init(&w.s, f, hx, gg);
        w.dec = pgl_prox_kkt_test(&w.s, kkt, a.gtol, a.maxiter);
        a.ll[r] = f;
    }
    __syncthreads();
    if (w.dec) {
        for (int c = tid; c < P; c += 256) xt[c] = x[c];
    } else {
        const double mg = pgl_prox_emit_row(v.y + o, v.gy + o, xt, a.q, w.s.t, lam_s, red, tid);
        if (tid == 0) w.s.m_zero = pgl_prox_min(w.s.m_zero, mg);
    }
    pgl_prox_leave(v, r, &w, a.flags, tid);
}

// One call of the machine for every running row after ONE evaluation of all rows at Xt: (ll, grad) come in and are turned
// into f, grad f in place.  Phase PGL_PROX_Y: they are (f_y, g_y), the trial goes out.  Phase PGL_PROX_TRIAL: sufficient
// decrease, backtrack / restart / accept, the KKT test and the momentum step; Xt[row] = the next point to evaluate.
__global__ __launch_bounds__(256) void k_prox_step(const ProxView v, const ProxArgs a)
{
    __shared__ double red[12];
    __shared__ ProxRow w;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    if (tid == 0) pgl_prox_load(v, r, &w.s);
    __syncthreads();
    if (w.s.phase == (double)PGL_PROX_DONE) return;
    const bool trial = w.s.phase == (double)PGL_PROX_TRIAL;
    double* x = v.x + o;
    double* y = v.y + o;
    double* gx = v.gx + o;
    double* gy = v.gy + o;
    double* g = a.grad + o;
    double* xt = a.Xt + o;
    const double lam_s = a.lam[r] / a.q.sigma;
    const double f = pgl_prox_smooth_row(P, xt, g, a.ll[r], a.q, red, tid);
    __syncthreads();                                                           // grad f of the row is in memory
    if (tid == 0) a.ll[r] = f;
    if (!trial) {
        if (tid == 0) w.dec = pgl_prox_y_arrived(&w.s, f);
        __syncthreads();
        if (w.dec) {
            for (int c = tid; c < P; c += 256) gy[c] = g[c];
        } else {
            for (int c = tid; c < P; c += 256) {
                y[c] = x[c];
                gy[c] = gx[c];
            }
        }
        __syncthreads();
        const double mg = pgl_prox_emit_row(y, gy, xt, a.q, w.s.t, lam_s, red, tid);
        if (tid == 0) w.s.m_zero = pgl_prox_min(w.s.m_zero, mg);
        pgl_prox_leave(v, r, &w, a.flags, tid);
        return;
    }
    double dot = 0.0, dd = 0.0, hz = pgl_prox_h_part(xt, a.q, lam_s, tid);
    for (int c = tid; c < P; c += 256) {
        const double d = xt[c] - y[c];
        dot = fma(gy[c], d, dot);
        dd = fma(d, d, dd);
    }
    pgl_blk_sum3(dot, dd, hz, red);
    if (tid == 0) w.dec = pgl_prox_decide(&w.s, f, hz, dot, dd, a.max_backtrack);
    __syncthreads();
    const int d = w.dec;
    if (d == PGL_PROX_D_FAIL) {
        for (int c = tid; c < P; c += 256) xt[c] = x[c];
        pgl_prox_leave(v, r, &w, a.flags, tid);
        return;
    }
    if (d == PGL_PROX_D_ACCEPT) {
        for (int c = tid; c < P; c += 256) {
            v.xp[o + c] = x[c];
            x[c] = xt[c];
            gx[c] = g[c];
        }
        __syncthreads();
        const double kkt = pgl_prox_kkt_row(x, gx, a.q, lam_s, red, tid);
        if (tid == 0) {
            w.dec = pgl_prox_kkt_test(&w.s, kkt, a.gtol, a.maxiter);
            w.val = w.dec ? 0.0 : pgl_prox_momentum(&w.s);
        }
        __syncthreads();
        if (w.dec) {                                                           // (Xt[row] is z = x already)
            pgl_prox_leave(v, r, &w, a.flags, tid);
            return;
        }
        const double beta = w.val;
        if (beta != 0.0) {
            for (int c = tid; c < P; c += 256) {
                const double yc = pgl_prox_extrapolate(x[c], v.xp[o + c], beta);
                y[c] = yc;
                xt[c] = yc;
            }
            pgl_prox_leave(v, r, &w, a.flags, tid);
            return;
        }
    }
    if (d != PGL_PROX_D_BACKTRACK) {                                           // restart, or beta = 0: the trial leaves from x
        for (int c = tid; c < P; c += 256) {
            y[c] = x[c];
            gy[c] = gx[c];
        }
        __syncthreads();
    }
    const double mg = pgl_prox_emit_row(y, gy, xt, a.q, w.s.t, lam_s, red, tid);
    if (tid == 0) w.s.m_zero = pgl_prox_min(w.s.m_zero, mg);
    pgl_prox_leave(v, r, &w, a.flags, tid);
}
