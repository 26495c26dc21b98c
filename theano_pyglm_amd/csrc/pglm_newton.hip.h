// lock-step dense Newton row kernels: k_newton_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// Lock-step dense Newton (inference/batched_newton.py): the Newton state machines of all M neurons of a range -- one
// workgroup per neuron row -- around the launches that do the work: the Hessian contraction of the rows still running
// (pgl_hvp_prepare_list_dev + pgl_hess_dev), their batched factorisation and solve (pgl_chol_factor_dev,
// pgl_chol_solve_dev) and one fused ll+grad evaluation of the rows still searching per line-search trial.  The algorithm
// and its decisions are pglm_newton.h (compiled for the host by tests/csrc/newton_host.c); these kernels own the vectors,
// the fixed-order reductions (pgl_blk_sum / pgl_blk_max), the priors' part of f, g and the Hessian, and fit_glm's NaN
// rules.  All state lives in ONE device block of doubles laid out by pgl_newton_view, as the Newton-CG block is; a row's
// scalar state sits in LDS while its workgroup runs.  A finished row (phase PGL_NEWTON_DONE) is frozen: its workgroup
// returns before it writes anything.
// ---------------------------------------------------------------------------
#include "pglm_newton.h"

struct NewtonView {
    int M, P;
    double *X, *g, *p, *Xb, *gb;              // (M, P): point, gradient, direction, best trial of the running search
    double* sc;                               // (PGL_NEWTON_NSCAL, M): PglNewton, field-major
    double* ls;                               // (PGL_LS_NDOUBLES, M): line-search state, field-major
};
#define PGL_NEWTON_NVEC 5
#define PGL_NEWTON_F_ALPHA 3                  // index of PglNewton::alpha in PGL_NEWTON_FIELDS
#define PGL_NEWTON_F_SHIFT 4
#define PGL_NEWTON_F_PHASE 10
__host__ __device__ inline size_t pgl_newton_doubles(int M, int P)
{
    return (size_t)M * P * PGL_NEWTON_NVEC + (size_t)M * (PGL_NEWTON_NSCAL + PGL_LS_NDOUBLES);
}
__host__ __device__ inline NewtonView pgl_newton_view(double* st, int M, int P)
{
    NewtonView v;
    const size_t MP = (size_t)M * P;
    v.M = M; v.P = P;
    v.X = st; v.g = st + MP; v.p = st + 2 * MP; v.Xb = st + 3 * MP; v.gb = st + 4 * MP;
    v.sc = st + PGL_NEWTON_NVEC * MP;
    v.ls = v.sc + (size_t)PGL_NEWTON_NSCAL * M;
    return v;
}
#define PGL_NEWTON_FIELDS(F) F(f, 0) F(fprev, 1) F(slope, 2) F(alpha, 3) F(shift, 4) F(nit, 5) F(nfev, 6) F(nhess, 7) \
    F(nfact, 8) F(status, 9) F(phase, 10)

// a row's scalar state in LDS for the lifetime of its workgroup
struct NewtonRow {
    PglNewton s;
    PglLs l;
    int dec[2];
    double val;
};
PGL_ROW_STATE(NewtonView, NewtonRow, PGL_NEWTON_FIELDS)
// max|a[c]| over a row, in every thread
__device__ __forceinline__ double pgl_newton_absmax(const double* __restrict__ a, const int P, double* red, const int tid)
{
    double m = 0.0;
    for (int c = tid; c < P; c += 256) m = fmax(m, fabs(a[c]));
    return pgl_blk_max(m, red);
}

// start of a fit: X of every row is in the state, (d_ll, d_grad) hold ll and its gradient at X, row by row
__global__ __launch_bounds__(256) void k_newton_init(const NewtonView v, double* __restrict__ ll, double* __restrict__ grad,
                                                     const BfgsPrior q, const double gtol, const int maxiter, double* flags)
{
    __shared__ double red[12];
    __shared__ NewtonRow w;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    pgl_bfgs_objective_row(P, v.X + o, grad + o, ll + r, q, red, tid);
    __syncthreads();
    for (int c = tid; c < P; c += 256) v.g[o + c] = grad[o + c];
    const double gmax = pgl_newton_absmax(grad + o, P, red, tid);
    if (tid == 0) {
        pgl_ls_start(&w.l, 1.0, ll[r], -1.0, PGL_NEWTON_C1, PGL_NEWTON_STPMIN, PGL_NEWTON_STPMAX);
        pgl_newton_init(&w.s, ll[r], gmax, gtol, maxiter);
    }
    pgl_row_leave(v, r, &w, flags, tid);
}

// A = -H_ll - H_prior(X) + shift diag(-H_ll - H_prior) of the listed rows, in place on the lower triangle of H (L, P, ld)
// (list position j: row rows[j], null: j), and the right-hand side of the solve, rhs[j] = -g[row] (null: none).  The prior's
// Hessian in the arithmetic of k_ncg_cg_step (priors.py hess_log_p_vec): 0/0 at a zero group is NaN and fails the factor.
__global__ __launch_bounds__(256) void k_newton_assemble(const NewtonView v, const int* __restrict__ rows,
                                                         double* __restrict__ H, const int ld, const BfgsPrior q,
                                                         double* __restrict__ rhs)
{
    const int j = blockIdx.x, r = rows ? rows[j] : j, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = v.P;
    const double* x = v.X + (size_t)r * P;
    const double shift = v.sc[(size_t)PGL_NEWTON_F_SHIFT * v.M + r];
    double* Hm = H + (size_t)j * P * ld;
    const int oi = 1 + q.Dstim;
    const double is2 = 1.0 / (q.sigma * q.sigma);
    if (rhs)
        for (int c = tid; c < P; c += 256) rhs[(size_t)j * P + c] = -v.g[(size_t)r * P + c];
    for (int i = wave; i < P; i += 4) {
        double* row = Hm + (size_t)i * ld;
        // the prior's numbers of row i: its diagonal term, and for the group lasso the group's z and norm
        double dg, zi = 0.0, nrm = 1.0, n3 = 1.0;
        int g0 = P, g1 = P;                                                    // columns of row i's group (kind 1)
        if (i == 0) dg = 1.0 / (q.sg_b * q.sg_b);                              // bias.py:33
        else if (i < oi) dg = 1.0 / (q.stim_sigma * q.stim_sigma);             // bkgd.py:76
        else if (q.kind == 1) {                                                // priors.py GroupLasso.hess_log_p_vec
            g0 = oi + ((i - oi) / q.B) * q.B;
            g1 = g0 + q.B;
            double ss = 0.0;
            for (int b = 0; b < q.B; ++b) {
                const double z = (x[g0 + b] - q.mu) / q.sigma;
                ss += z * z;
            }
            nrm = sqrt(ss);
            n3 = nrm * nrm * nrm;
            zi = (x[i] - q.mu) / q.sigma;
            dg = 0.0;
        } else dg = is2;                                                       // priors.py Gaussian.hess_log_p_vec
        for (int c = lane; c <= i; c += 64) {
            double hp = c == i ? -dg : 0.0;                                    // the Hessian of the log prior
            if (c >= g0 && c < g1) {
                const double zc = (x[c] - q.mu) / q.sigma;
                hp = -q.lam * is2 * ((c == i ? 1.0 : 0.0) / nrm - zi * zc / n3);
            }
            const double a = -(row[c] + hp);
            row[c] = c == i ? fma(shift, a, a) : a;
        }
    }
}

// The factorisation and the solve of the listed rows have run (info[j], sol[j] = -(A + shift diag A)^-1 g by list
// position): the direction and the start of the line search, or a raised shift (phase PGL_NEWTON_REFACTOR), or -g.
__global__ __launch_bounds__(256) void k_newton_direction(const NewtonView v, const int* __restrict__ rows,
                                                          const int* __restrict__ info, const double* __restrict__ sol,
                                                          double* flags)
{
    __shared__ double red[12];
    __shared__ NewtonRow w;
    const int j = blockIdx.x, r = rows ? rows[j] : j, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    if (tid == 0) pgl_row_load(v, r, &w);
    __syncthreads();
    if (w.s.phase != (double)PGL_NEWTON_HESS && w.s.phase != (double)PGL_NEWTON_REFACTOR) return;
    const double* pj = sol + (size_t)j * P;
    const bool failed = info[j] != 0;
    double slope = 0.0, gg = 0.0, z = 0.0;
    for (int c = tid; c < P; c += 256) {
        const double gc = v.g[o + c];
        slope = fma(gc, failed ? 0.0 : pj[c], slope);
        gg = fma(gc, gc, gg);
    }
    pgl_blk_sum3(slope, gg, z, red);
    if (tid == 0) w.dec[0] = pgl_newton_direction(&w.s, &w.l, failed ? 1 : 0, slope, gg);
    __syncthreads();
    const int d = w.dec[0];
    if (d == PGL_NEWTON_DIR_NEWTON)
        for (int c = tid; c < P; c += 256) v.p[o + c] = pj[c];
    else if (d == PGL_NEWTON_DIR_STEEPEST)
        for (int c = tid; c < P; c += 256) v.p[o + c] = -v.g[o + c];
    pgl_row_leave(v, r, &w, flags, tid);
}

// One line-search step of every listed row whose search runs (pgl_row_search_front along p); a row that takes a point
// goes on here: the convergence test on its gradient.
__global__ __launch_bounds__(256) void k_newton_search_step(const NewtonView v, const RowSearchArgs a)
{
    __shared__ double red[12];
    __shared__ NewtonRow w;
    const int j = blockIdx.x, r = a.rows ? a.rows[j] : j, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    const double *xsrc, *gsrc;
    const int d = pgl_row_search_front(
        v, a, j, r, &w, v.p + o,
        [](NewtonRow* w, double f, double dp) { return pgl_newton_search_step(&w->s, &w->l, f, dp, &w->val); }, red, tid, &xsrc,
        &gsrc);
    if (d != PGL_LS_TAKE_TRIAL && d != PGL_LS_TAKE_BEST) return;
    double gmax = 0.0;
    for (int c = tid; c < P; c += 256) {
        const double gc = gsrc[c];
        gmax = fmax(gmax, fabs(gc));
        v.X[o + c] = xsrc[c];
        v.g[o + c] = gc;
    }
    gmax = pgl_blk_max(gmax, red);
    if (tid == 0) pgl_newton_accept(&w.s, w.val, gmax, a.gtol, a.maxiter);
    pgl_row_leave(v, r, &w, a.flags, tid);
}
