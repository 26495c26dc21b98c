// lock-step Newton-CG row kernels: k_ncg_*
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// Lock-step Newton-CG (inference/batched_newton_cg.py): the truncated-Newton state machines of all M neurons of a shard
// -- one workgroup per neuron row -- around the two launches that do the work: ONE Hessian-vector product over all rows
// per CG iteration (pgl_hvp_apply_dev) and one fused ll+grad evaluation of the rows still searching per line-search
// trial (pgl_ll_grad_list_dev).  The algorithm and its decisions are pglm_ncg.h (scipy's Newton-CG as fit_glm(use_rop=True)
// calls it; compiled for the host by tests/csrc/ncg_host.c); these kernels own the vectors, the fixed-order reductions
// (wave64 butterflies, then the four waves through LDS: pgl_blk_sum), the priors' part of f, g and H v and fit_glm's
// NaN rules.  All state lives in ONE device block of doubles laid out by pgl_ncg_view; a row's scalar state sits in
// LDS while its workgroup runs.  A finished row (phase PGL_NCG_DONE) is frozen: its workgroup returns before it
// writes anything, and its product input V[row] has been zeroed when it finished.
// ---------------------------------------------------------------------------
#include "pglm_ncg.h"

struct NcgView {
    int M, P;
    double *X, *g, *xs, *r, *p, *Xb, *gb;    // (M, P): point, gradient, xsupi = pk, ri, psupi, best trial of the search
    double* sc;                               // (PGL_NCG_NSCAL, M): PglNcg, field-major
    double* ls;                               // (PGL_LS_NDOUBLES, M): line-search state, field-major
};
#define PGL_NCG_NVEC 7
#define PGL_NCG_F_PHASE 10                   // indices of PglNcg::phase, ::alpha in PGL_NCG_FIELDS
#define PGL_NCG_F_ALPHA 12
__host__ __device__ inline size_t pgl_ncg_doubles(int M, int P)
{
    return (size_t)M * P * PGL_NCG_NVEC + (size_t)M * (PGL_NCG_NSCAL + PGL_LS_NDOUBLES);
}
__host__ __device__ inline NcgView pgl_ncg_view(double* st, int M, int P)
{
    NcgView v;
    const size_t MP = (size_t)M * P;
    v.M = M; v.P = P;
    v.X = st; v.g = st + MP; v.xs = st + 2 * MP; v.r = st + 3 * MP; v.p = st + 4 * MP; v.Xb = st + 5 * MP; v.gb = st + 6 * MP;
    v.sc = st + PGL_NCG_NVEC * MP;
    v.ls = v.sc + (size_t)PGL_NCG_NSCAL * M;
    return v;
}
#define PGL_NCG_FIELDS(F) F(f, 0) F(fprev, 1) F(dri0, 2) F(termcond, 3) F(cgit, 4) F(alphai, 5) F(nit, 6) F(nhev, 7) \
    F(nfev, 8) F(status, 9) F(phase, 10) F(slope, 11) F(alpha, 12) F(fb, 13) F(alpha_acc, 14) F(moved, 15)

// a row's scalar state in LDS for the lifetime of its workgroup
struct NcgRow {
    PglNcg s;
    PglLs l;
    int dec[2];
    double val;
};
PGL_ROW_STATE(NcgView, NcgRow, PGL_NCG_FIELDS)
__device__ __forceinline__ void pgl_ncg_zero(double* __restrict__ a, const int P, const int tid)
{
    for (int c = tid; c < P; c += 256) a[c] = 0.0;
}

// CG has ended with pk = xsupi: slope and |pk|_1, start of the line search (or the end of the row); V[row] = 0
__device__ __forceinline__ void pgl_ncg_cg_end_row(const NcgView& v, const int r, NcgRow* w, double* __restrict__ Vr,
                                                   double* red, const int tid)
{
    const size_t o = (size_t)r * v.P;
    double slope = 0.0, pn = 0.0, z = 0.0;
    for (int c = tid; c < v.P; c += 256) {
        const double x = v.xs[o + c];
        slope = fma(v.g[o + c], x, slope);
        pn += fabs(x);
        Vr[c] = 0.0;
    }
    pgl_blk_sum3(slope, pn, z, red);
    if (tid == 0) pgl_ncg_cg_end(&w->s, &w->l, slope, pn);
    __syncthreads();
}

// start of an outer iteration at (X, g) of the row: CG start and the first product's input V[row] = psupi = -g
__device__ __forceinline__ void pgl_ncg_outer_begin_row(const NcgView& v, const int r, NcgRow* w, const int maxiter,
                                                        double* __restrict__ Vr, double* red, const int tid)
{
    const size_t o = (size_t)r * v.P;
    double mag = 0.0, gg = 0.0, z = 0.0;
    for (int c = tid; c < v.P; c += 256) {
        const double gc = v.g[o + c];
        mag += fabs(gc);
        gg = fma(gc, gc, gg);
    }
    pgl_blk_sum3(mag, gg, z, red);
    if (tid == 0) w->dec[0] = pgl_ncg_outer_begin(&w->s, mag, gg, maxiter);
    __syncthreads();
    const int ph = w->dec[0];
    if (ph == PGL_NCG_DONE) {
        pgl_ncg_zero(Vr, v.P, tid);
        return;
    }
    for (int c = tid; c < v.P; c += 256) {
        const double gc = v.g[o + c];
        v.xs[o + c] = 0.0;
        v.r[o + c] = gc;
        v.p[o + c] = -gc;
        Vr[c] = ph == PGL_NCG_CG ? -gc : 0.0;
    }
    if (ph == PGL_NCG_SEARCH) pgl_ncg_cg_end_row(v, r, w, Vr, red, tid);
}

// start of a fit: X of every row is in the state, (d_ll, d_grad) hold ll and its gradient at X, row by row
__global__ __launch_bounds__(256) void k_ncg_init(const NcgView v, double* __restrict__ ll, double* __restrict__ grad,
                                                  const BfgsPrior q, const int maxiter, double* __restrict__ V, double* flags)
{
    __shared__ double red[12];
    __shared__ NcgRow w;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    pgl_bfgs_objective_row(P, v.X + o, grad + o, ll + r, q, red, tid);
    __syncthreads();
    for (int c = tid; c < P; c += 256) v.g[o + c] = grad[o + c];
    if (tid == 0) {
        pgl_ls_start(&w.l, 1.0, ll[r], -1.0, PGL_NCG_C1, PGL_NCG_STPMIN, PGL_NCG_STPMAX);
        pgl_ncg_init(&w.s, ll[r]);
    }
    __syncthreads();
    pgl_ncg_outer_begin_row(v, r, &w, maxiter, V + o, red, tid);
    pgl_row_leave(v, r, &w, flags, tid);
}

// One CG iteration of every row whose CG runs, after ONE product over all rows: Hv[row] = H_ll psupi comes in, is
// turned into A psupi = -(H_ll + H_prior) psupi in place (NaN rule: a product holding a NaN is zero), then curvature,
// the three stop tests, the CG update and the next product's input V[row] (zero once the row's CG has ended).
__global__ __launch_bounds__(256) void k_ncg_cg_step(const NcgView v, double* __restrict__ Hv, const BfgsPrior q,
                                                     double* __restrict__ V, double* flags)
{
    __shared__ double red[12];
    __shared__ NcgRow w;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    if (tid == 0) pgl_row_load(v, r, &w);
    __syncthreads();
    if (w.s.phase != (double)PGL_NCG_CG) return;
    double* ap = Hv + o;
    double* Vr = V + o;
    const double* x = v.X + o;
    const double* p = v.p + o;
    bool bad = false;
    if (tid == 0) {                                                            // bias.py:33
        const double a = -(ap[0] - p[0] / (q.sg_b * q.sg_b));
        bad = bad || (a != a);
        ap[0] = a;
    }
    for (int c = 1 + tid; c < 1 + q.Dstim; c += 256) {                         // bkgd.py:76
        const double a = -(ap[c] - p[c] / (q.stim_sigma * q.stim_sigma));
        bad = bad || (a != a);
        ap[c] = a;
    }
    const int oi = 1 + q.Dstim;
    for (int n = tid; n < q.N; n += 256) {                                     // one presynaptic group per thread
        const double* xw = x + oi + n * q.B;
        const double* pw = p + oi + n * q.B;
        double* aw = ap + oi + n * q.B;
        const double is2 = 1.0 / (q.sigma * q.sigma);
        if (q.kind == 1) {                                                     // priors.py GroupLasso.hess_log_p_vec
            double ss = 0.0, zv = 0.0;
            for (int b = 0; b < q.B; ++b) {
                const double z = (xw[b] - q.mu) / q.sigma;
                ss += z * z;
                zv += z * pw[b];
            }
            const double nrm = sqrt(ss), n3 = nrm * nrm * nrm;
            for (int b = 0; b < q.B; ++b) {
                const double z = (xw[b] - q.mu) / q.sigma;
                const double hp = -q.lam * is2 * (pw[b] / nrm - z * zv / n3);  // 0/0 -> NaN like the host prior
                const double a = -(aw[b] + hp);
                bad = bad || (a != a);
                aw[b] = a;
            }
        } else {                                                               // priors.py Gaussian.hess_log_p_vec
            for (int b = 0; b < q.B; ++b) {
                const double a = -(aw[b] - pw[b] * is2);
                bad = bad || (a != a);
                aw[b] = a;
            }
        }
    }
    const bool anybad = pgl_blk_max(bad ? 1.0 : 0.0, red) > 0.0;               // (its barriers: A psupi is in memory)
    double curv = 0.0;
    if (!anybad)
        for (int c = tid; c < P; c += 256) curv = fma(p[c], ap[c], curv);
    curv = pgl_blk_sum(curv, red);
    if (tid == 0) {
        const int d = pgl_ncg_cg_curv(&w.s, curv);
        if (d == PGL_NCG_CURV_FAIL) pgl_ncg_finish(&w.s, PGL_NCG_CGFAIL);
        w.dec[0] = d;
    }
    __syncthreads();
    const int d = w.dec[0];
    if (d == PGL_NCG_CURV_FAIL) {
        pgl_ncg_zero(Vr, P, tid);
        pgl_row_leave(v, r, &w, flags, tid);
        return;
    }
    const double alphai = w.s.alphai;
    if (d == PGL_NCG_CURV_UPDATE) {
        double dri1 = 0.0, rn = 0.0, z = 0.0;
        for (int c = tid; c < P; c += 256) {
            double xc = v.xs[o + c], rc = v.r[o + c];
            const double rnew = pgl_ncg_cg_elem_xr(alphai, p[c], anybad ? 0.0 : ap[c], &xc, &rc);
            v.xs[o + c] = xc;
            v.r[o + c] = rc;
            dri1 = fma(rnew, rnew, dri1);
            rn += fabs(rnew);
        }
        pgl_blk_sum3(dri1, rn, z, red);
        if (tid == 0) {
            double betai = 0.0;
            w.dec[1] = pgl_ncg_cg_next(&w.s, dri1, rn, P, &betai);
            w.val = betai;
        }
        __syncthreads();
        const int go = w.dec[1];
        if (go < 0) {
            pgl_ncg_zero(Vr, P, tid);
            pgl_row_leave(v, r, &w, flags, tid);
            return;
        }
        const double betai = w.val;
        for (int c = tid; c < P; c += 256) {
            const double pn = pgl_ncg_cg_elem_p(betai, v.r[o + c], v.p[o + c]);
            v.p[o + c] = pn;
            Vr[c] = go == 1 ? pn : 0.0;
        }
        if (go == 0) pgl_ncg_cg_end_row(v, r, &w, Vr, red, tid);
    } else {
        if (d == PGL_NCG_CURV_STEEPEST)
            for (int c = tid; c < P; c += 256) v.xs[o + c] = alphai * -v.g[o + c];
        __syncthreads();
        pgl_ncg_cg_end_row(v, r, &w, Vr, red, tid);
    }
    pgl_row_leave(v, r, &w, flags, tid);
}

// One line-search step of every listed row whose search runs (pgl_row_search_front along pk = xsupi); a row that takes a
// point goes on here: the convergence test and the whole start of the next outer iteration (the accepted point carries
// its gradient), V[row] included.
__global__ __launch_bounds__(256) void k_ncg_search_step(const NcgView v, const RowSearchArgs a)
{
    __shared__ double red[12];
    __shared__ NcgRow w;
    const int j = blockIdx.x, r = a.rows ? a.rows[j] : j, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    const double *xsrc, *gsrc;
    const int d = pgl_row_search_front(
        v, a, j, r, &w, v.xs + o, [](NcgRow* w, double f, double dp) { return pgl_ncg_search_step(&w->s, &w->l, f, dp); }, red,
        tid, &xsrc, &gsrc);
    if (d != PGL_LS_TAKE_TRIAL && d != PGL_LS_TAKE_BEST) return;
    const double al = w.s.alpha_acc;
    double un = 0.0;
    for (int c = tid; c < P; c += 256) {
        un += fabs(al * v.xs[o + c]);
        v.X[o + c] = xsrc[c];
        v.g[o + c] = gsrc[c];
    }
    un = pgl_blk_sum(un, red);
    if (tid == 0) w.dec[1] = pgl_ncg_accept(&w.s, d == PGL_LS_TAKE_TRIAL ? a.ft[j] : w.s.fb, un, P);
    __syncthreads();
    if (w.dec[1] == PGL_NCG_CG) pgl_ncg_outer_begin_row(v, r, &w, a.maxiter, a.V + o, red, tid);
    pgl_row_leave(v, r, &w, a.flags, tid);
}
