// what the lock-step Newton-CG and dense Newton row kernels share: a row's scalar state in LDS, the trial kernel and the
// front half of a line-search step
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// Both optimisers keep their state in one device block of doubles: vectors (M, P) first, then the scalar struct and the
// line-search state field-major, (fields, M).  A view V has .M, .P, .X, .Xb, .gb, .sc and .ls; a row struct W has the
// scalar struct .s (with .phase and .alpha), the PglLs .l, and the workgroup's scratch .dec[2] and .val.  The phase
// "its line search runs" is 1 in both (PGL_NCG_SEARCH, PGL_NEWTON_SEARCH).
// ---------------------------------------------------------------------------
#include "pglm_linesearch.h"

#define PGL_ROW_SEARCH 1

#define PGL_ROW_LD_S(name, k) w->s.name = v.sc[(size_t)k * v.M + r];
#define PGL_ROW_LD_L(name, k) w->l.name = v.ls[(size_t)k * v.M + r];
#define PGL_ROW_ST_S(name, k) v.sc[(size_t)k * v.M + r] = w->s.name;
#define PGL_ROW_ST_L(name, k) v.ls[(size_t)k * v.M + r] = w->l.name;
// pgl_row_load / pgl_row_store of a (view, row struct) pair whose scalar struct has the fields FIELDS
#define PGL_ROW_STATE(View, Row, FIELDS)                                                                  \
    __device__ __forceinline__ void pgl_row_load(const View& v, int r, Row* w)                            \
    {                                                                                                     \
        FIELDS(PGL_ROW_LD_S)                                                                              \
        PGL_LS_FIELDS(PGL_ROW_LD_L)                                                                       \
    }                                                                                                     \
    __device__ __forceinline__ void pgl_row_store(const View& v, int r, const Row* w)                     \
    {                                                                                                     \
        FIELDS(PGL_ROW_ST_S)                                                                              \
        PGL_LS_FIELDS(PGL_ROW_ST_L)                                                                       \
    }

// end of a workgroup that has advanced its row: state back to memory, the row's phase to the driver's pinned flags
template <class View, class Row>
__device__ __forceinline__ void pgl_row_leave(const View& v, int r, const Row* w, double* flags, const int tid)
{
    __syncthreads();
    if (tid == 0) {
        pgl_row_store(v, r, w);
        if (flags) __hip_atomic_store(flags + r, w->s.phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// points of the listed rows: Xt[j] = X[r] + alpha[r] d[r] for a row whose search runs, X[r] for any other (the points the
// Hessian of a list is taken at), r = rows[j] (null: r = j).  alpha, phase: the (M) rows of the scalar block.
__global__ __launch_bounds__(256) void k_row_trial(const double* __restrict__ X, const double* __restrict__ d,
                                                   const double* __restrict__ alpha, const double* __restrict__ phase,
                                                   const int P, const int* __restrict__ rows, double* __restrict__ Xt)
{
    const int j = blockIdx.x, r = rows ? rows[j] : j;
    const bool search = phase[r] == (double)PGL_ROW_SEARCH;
    const double a = alpha[r];
    for (int c = threadIdx.x; c < P; c += 256) {
        const double xc = X[(size_t)r * P + c];
        Xt[(size_t)j * P + c] = search ? xc + a * d[(size_t)r * P + c] : xc;
    }
}

// One line-search step of every listed row whose search runs, after ONE ll+grad evaluation of their trial points
// (Xt / ft / gt by list position).  V (the next product's input) and gtol are each read by one optimiser only.
struct RowSearchArgs {
    const int* rows;
    const double* Xt;
    double* ft;
    double* gt;
    BfgsPrior q;
    double gtol;
    int maxiter;
    const int* pos_next;
    double* Xt_next;
    double* V;
    double* flags;
};

// The front half of a search-step kernel for list position j = row r, along the row's direction d: priors and NaN rules
// in place, phi' = g_trial . d, the decision  step(w, f, phi') -> PGL_LS_*;  then, unless the row takes a point, the rest
// of its launch: the trial that became the best step into Xb / gb, the next trial point into the next launch's list
// position, state and flag out.  Returns the decision (-1: the row's search does not run, nothing is written); on
// PGL_LS_TAKE_* the caller moves the row to (*xsrc, *gsrc) and leaves.
template <class View, class Row, class Step>
__device__ __forceinline__ int pgl_row_search_front(const View& v, const RowSearchArgs& a, const int j, const int r, Row* w,
                                                    const double* d, Step step, double* red, const int tid,
                                                    const double** xsrc, const double** gsrc)
{
    const int P = v.P;
    const size_t o = (size_t)r * P;
    if (tid == 0) pgl_row_load(v, r, w);
    __syncthreads();
    if (w->s.phase != (double)PGL_ROW_SEARCH) return -1;
    const double* __restrict__ xt = a.Xt + (size_t)j * P;
    double* __restrict__ gt = a.gt + (size_t)j * P;
    pgl_bfgs_objective_row(P, xt, gt, a.ft + j, a.q, red, tid);
    __syncthreads();
    double dp = 0.0;
    for (int c = tid; c < P; c += 256) dp = fma(gt[c], d[c], dp);
    dp = pgl_blk_sum(dp, red);
    if (tid == 0) w->dec[0] = step(w, a.ft[j], dp);
    __syncthreads();
    const int dc = w->dec[0];
    if (dc == PGL_LS_EVALUATE) {
        if (w->l.moved != 0.0)
            for (int c = tid; c < P; c += 256) {
                v.Xb[o + c] = xt[c];
                v.gb[o + c] = gt[c];
            }
        if (a.Xt_next) {
            const int jn = a.pos_next ? a.pos_next[r] : j;
            if (jn >= 0) {
                const double al = w->s.alpha;
                for (int c = tid; c < P; c += 256) a.Xt_next[(size_t)jn * P + c] = v.X[o + c] + al * d[c];
            }
        }
    }
    if (dc == PGL_LS_EVALUATE || dc == PGL_LS_FAIL) pgl_row_leave(v, r, w, a.flags, tid);
    const bool trial = dc == PGL_LS_TAKE_TRIAL;
    *xsrc = trial ? xt : v.Xb + o;
    *gsrc = trial ? gt : v.gb + o;
    return dc;
}
