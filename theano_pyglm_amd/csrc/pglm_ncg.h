// Truncated-Newton (Newton-CG) optimiser of one row as a reverse-communication state machine: the scalar decisions and the
// per-element updates of the algorithm, no loops over the row and no callbacks -- the caller (the k_ncg_* row kernels of
// pglm_ncg.hip.h, one workgroup per neuron; tests/csrc/ncg_host.c on the host) owns the vectors, computes the reductions
// (dot products, l1 norms) and supplies f, g and H v.  That is what lets all neurons of a shard advance in lock step: one
// Hessian-vector launch per CG iteration, one ll+grad launch per line-search trial (inference/batched_newton_cg.py).
//
// The algorithm is the one fit_glm(use_rop=True) gets from scipy.optimize.minimize(method='Newton-CG', jac=, hessp=)
// (the reference's Rop branch, parallel_coord_descent.py:119-121 / map.py:38-45): the line-search Newton-CG method of
// Nocedal & Wright, "Numerical Optimization", 2nd ed., algorithm 7.1, with scipy's constants:
//   outer iteration k at x_k:  b = -g(x_k), maggrad = |b|_1, eta = min(0.5, sqrt(maggrad)), termcond = eta * maggrad;
//   CG on H p = b from xsupi = 0, ri = g, psupi = -ri, dri0 = ri.ri, at most 20 P iterations:
//     |ri|_1 <= termcond -> done;  curv = psupi . (H psupi);  0 <= curv <= 3 eps -> done;  curv < 0 -> done, on the FIRST
//     CG iteration with the steepest-descent step xsupi = dri0 / (-curv) * b;  else alphai = dri0 / curv,
//     xsupi += alphai psupi, ri += alphai H psupi, betai = ri.ri / dri0, psupi = -ri + betai psupi;
//     20 P iterations without one of these exits end the row with status 3;
//   strong-Wolfe line search along pk = xsupi (pglm_linesearch.h: MINPACK-2 DCSRCH as scipy calls it here: c1 = 1e-4,
//     c2 = 0.9, xtol = 1e-14, steps in [1e-8, 50], at most 100 trials; first trial step 1 on the first outer iteration,
//     then min(1, 1.01 * 2 (f_k - f_{k-1}) / slope), 1 if that is not positive);
//   x_{k+1} = x_k + alpha_k pk;  stop when |alpha_k pk|_1 <= P * xtol (xtol = 1e-5; status 0, or 3 if that norm is NaN),
//   or after maxiter outer iterations (status 1).
// NaN rules of fit_glm (coord_descent.py:170-182 and its hessp wrapper): objective NaN -> 1e16, a gradient holding a NaN
// -> 0, a product holding a NaN -> 0; the caller applies them before it hands the numbers in.
//
// Where this differs from scipy (all outside the iterates of a healthy fit):
//  * scipy falls back on line_search_wolfe2 when DCSRCH gives up (warning, 100 trials, non-finite value).  Here, as in the
//    lock-step BFGS rows, the best sufficient-decrease point of the search is taken if there is one (the trial itself or
//    the best step so far), else the row stops with scipy's status 2 ("precision loss").
//  * a zero direction (pk = 0: the gradient is zero, e.g. zeroed by the NaN rule, or the first curvature is within
//    [0, 3 eps]): DCSRCH refuses phi'(0) = 0 and scipy's fallback search accepts the step 1 along it, i.e. the zero
//    update, and stops with status 0 after that iteration.  pgl_ncg_cg_end reports exactly that without a search.
//    Any other direction with phi'(0) >= 0 ends the row with status 2.
//  * a first trial step below the lower step bound 1e-8 is raised to it (scipy: an error of DCSRCH, then the fallback).
//  * a non-finite curvature ends the row with status 3 at once (scipy runs its 20 P CG iterations on NaNs first).
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_NCG_H
#define PGLM_NCG_H

#include "pglm_linesearch.h"

#define PGL_NCG_FN PGL_LS_FN

// phase of a row
#define PGL_NCG_CG 0        // its CG runs: the next product's input is psupi
#define PGL_NCG_SEARCH 1    // its line search runs: evaluate f, g at x + alpha pk
#define PGL_NCG_DONE 2      // finished (status >= 0): nothing of the row is written again

// scipy's status codes
#define PGL_NCG_RUNNING (-1)
#define PGL_NCG_SUCCESS 0
#define PGL_NCG_MAXITER 1
#define PGL_NCG_PRLOSS 2
#define PGL_NCG_CGFAIL 3    // CG ran out of iterations ("the Hessian is not positive definite") / NaN update norm

#define PGL_NCG_C1 1e-4
#define PGL_NCG_C2 0.9
#define PGL_NCG_LS_XTOL 1e-14
#define PGL_NCG_STPMIN 1e-8
#define PGL_NCG_STPMAX 50.0
#define PGL_NCG_MAX_TRIALS 100
#define PGL_NCG_XTOL 1e-5
#define PGL_NCG_EPS 2.220446049250313e-16

// outcome of pgl_ncg_cg_curv
#define PGL_NCG_CURV_UPDATE 0   // regular CG update with s->alphai
#define PGL_NCG_CURV_END 1      // CG ends, xsupi as it is
#define PGL_NCG_CURV_STEEPEST 2 // CG ends with xsupi = s->alphai * b   (negative curvature on the first iteration)
#define PGL_NCG_CURV_FAIL 3     // non-finite curvature: status 3

// outcome of pgl_ncg_search_step
#define PGL_NCG_LS_EVALUATE PGL_LS_EVALUATE     // evaluate at s->alpha next
#define PGL_NCG_LS_TAKE_TRIAL PGL_LS_TAKE_TRIAL // the row takes the trial just evaluated (step length s->alpha_acc)
#define PGL_NCG_LS_TAKE_BEST PGL_LS_TAKE_BEST   // the row takes the best step saved so far (s->alpha_acc, value s->fb)
#define PGL_NCG_LS_FAIL PGL_LS_FAIL             // no acceptable point: status 2

#define PGL_NCG_NSCAL 16

typedef struct {
    double f, fprev;            // objective at x_k and at x_{k-1}
    double dri0, termcond;      // ri.ri, the CG tolerance of this outer iteration
    double cgit;                // completed CG iterations of this outer iteration
    double alphai;              // CG step (or the steepest-descent factor) chosen by pgl_ncg_cg_curv
    double nit, nhev, nfev;     // outer iterations, products, objective evaluations (the starting point counts)
    double status, phase;
    double slope, alpha;        // phi'(0) of the running search, its next trial step
    double fb;                  // value at the best step of the running search (its point and gradient: the caller's)
    double alpha_acc;           // step length of the accepted point
    double moved;               // 1: the trial just evaluated became the best step (the caller saves point and gradient)
} PglNcg;

PGL_NCG_FN int pgl_ncg_finite(double x) { return pgl_ls_finite(x); }

PGL_NCG_FN void pgl_ncg_finish(PglNcg* s, int status)
{
    s->status = (double)status;
    s->phase = (double)PGL_NCG_DONE;
}

// start of a fit: f = f(x_0) (NaN rule applied)
PGL_NCG_FN void pgl_ncg_init(PglNcg* s, double f)
{
    s->f = f; s->fprev = f;
    s->dri0 = 0.0; s->termcond = 0.0; s->cgit = 0.0; s->alphai = 0.0;
    s->nit = 0.0; s->nhev = 0.0; s->nfev = 1.0;
    s->status = (double)PGL_NCG_RUNNING; s->phase = (double)PGL_NCG_CG;
    s->slope = 0.0; s->alpha = 0.0; s->fb = f; s->alpha_acc = 0.0; s->moved = 0.0;
}

// Start of an outer iteration at x_k with gradient g: maggrad = |g|_1, gg = g.g.  The caller sets xsupi = 0, ri = g,
// psupi = -g.  Returns the phase: PGL_NCG_DONE (maxiter reached: status 1), PGL_NCG_CG (the first product is due), or
// PGL_NCG_SEARCH, which here means "CG has ended before its first product": call pgl_ncg_cg_end next.
PGL_NCG_FN int pgl_ncg_outer_begin(PglNcg* s, double maggrad, double gg, int maxiter)
{
    if (s->nit >= (double)maxiter) {
        pgl_ncg_finish(s, PGL_NCG_MAXITER);
        return PGL_NCG_DONE;
    }
    const double sq = pgl_ls_sqrt(maggrad);
    const double eta = sq < 0.5 ? sq : 0.5;              // min(0.5, sqrt(maggrad))
    s->termcond = eta * maggrad;
    s->dri0 = gg;
    s->cgit = 0.0;
    s->phase = (double)PGL_NCG_CG;
    return (maggrad <= s->termcond) ? PGL_NCG_SEARCH : PGL_NCG_CG;
}

// curv = psupi . (H psupi) of the product just made (NaN rule applied to the product)
PGL_NCG_FN int pgl_ncg_cg_curv(PglNcg* s, double curv)
{
    s->nhev += 1.0;
    if (!pgl_ncg_finite(curv)) return PGL_NCG_CURV_FAIL;
    if (0.0 <= curv && curv <= 3.0 * PGL_NCG_EPS) return PGL_NCG_CURV_END;
    if (curv < 0.0) {
        if (s->cgit > 0.0) return PGL_NCG_CURV_END;
        s->alphai = s->dri0 / (-curv);
        return PGL_NCG_CURV_STEEPEST;
    }
    s->alphai = s->dri0 / curv;
    return PGL_NCG_CURV_UPDATE;
}
// the per-element CG update: xsupi += alphai psupi, ri += alphai Ap; returns the new ri (for ri.ri and |ri|_1)
PGL_NCG_FN double pgl_ncg_cg_elem_xr(double alphai, double psupi, double ap, double* xsupi, double* ri)
{
    *xsupi += alphai * psupi;
    *ri += alphai * ap;
    return *ri;
}
// after the update: dri1 = ri.ri, rnorm1 = |ri|_1.  Returns betai through *betai and 1 when the CG goes on (the caller
// sets psupi = -ri + betai psupi and makes the next product), 0 when it has ended (call pgl_ncg_cg_end), -1 when the
// row has failed (20 P iterations: status 3).
PGL_NCG_FN int pgl_ncg_cg_next(PglNcg* s, double dri1, double rnorm1, int P, double* betai)
{
    *betai = dri1 / s->dri0;
    s->cgit += 1.0;
    s->dri0 = dri1;
    if (s->cgit >= 20.0 * (double)P) {
        pgl_ncg_finish(s, PGL_NCG_CGFAIL);
        return -1;
    }
    return (rnorm1 <= s->termcond) ? 0 : 1;
}
PGL_NCG_FN double pgl_ncg_cg_elem_p(double betai, double ri, double psupi) { return -ri + betai * psupi; }

// CG has ended with the direction pk = xsupi: slope = g . pk, pnorm1 = |pk|_1.  Starts the line search (ls) and returns
// PGL_NCG_SEARCH (evaluate at x + s->alpha pk), or PGL_NCG_DONE (zero direction: status 0 after this iteration;
// no descent: status 2).
PGL_NCG_FN int pgl_ncg_cg_end(PglNcg* s, PglLs* ls, double slope, double pnorm1)
{
    s->slope = slope;
    if (pnorm1 == 0.0) {                                 // the zero update (see the header comment)
        s->nit += 1.0;
        s->nfev += 1.0;
        s->fprev = s->f;
        pgl_ncg_finish(s, PGL_NCG_SUCCESS);
        return PGL_NCG_DONE;
    }
    if (!(slope < 0.0)) {
        pgl_ncg_finish(s, PGL_NCG_PRLOSS);
        return PGL_NCG_DONE;
    }
    double a0 = (s->nit == 0.0) ? 1.0 : pgl_ls_first_step(s->f, s->fprev, slope);
    if (a0 < PGL_NCG_STPMIN) a0 = PGL_NCG_STPMIN;
    pgl_ls_start(ls, a0, s->f, slope, PGL_NCG_C1, PGL_NCG_STPMIN, PGL_NCG_STPMAX);
    s->alpha = a0;
    s->fb = s->f;
    s->moved = 0.0;
    s->phase = (double)PGL_NCG_SEARCH;
    return PGL_NCG_SEARCH;
}

// The trial x + s->alpha pk has been evaluated: f (NaN rule applied), dphi = g_trial . pk.  pgl_ls_guarded_step on the
// exact value at the best step (s->fb), mirrored into the row's own fields.
PGL_NCG_FN int pgl_ncg_search_step(PglNcg* s, PglLs* ls, double f, double dphi)
{
    double facc;                                         // (the caller has both values: f and s->fb)
    s->nfev += 1.0;
    const int d = pgl_ls_guarded_step(ls, f, dphi, s->fb, PGL_NCG_C1, PGL_NCG_C2, PGL_NCG_LS_XTOL, PGL_NCG_STPMIN,
                                      PGL_NCG_STPMAX, PGL_NCG_MAX_TRIALS, &s->alpha_acc, &facc);
    s->moved = 0.0;
    if (d == PGL_LS_EVALUATE) {
        s->alpha = ls->stp;
        if (ls->moved != 0.0) {
            s->fb = f;
            s->moved = 1.0;
        }
    } else if (d == PGL_LS_FAIL) pgl_ncg_finish(s, PGL_NCG_PRLOSS);
    return d;
}

// The row has taken the step alpha_acc pk to a point with value fnew: updnorm1 = |alpha_acc pk|_1.  Returns PGL_NCG_DONE
// (converged: status 0; NaN norm: status 3) or PGL_NCG_CG: the caller starts the next outer iteration with
// pgl_ncg_outer_begin on the gradient of the accepted point.
PGL_NCG_FN int pgl_ncg_accept(PglNcg* s, double fnew, double updnorm1, int P)
{
    s->fprev = s->f;
    s->f = fnew;
    s->nit += 1.0;
    if (!(updnorm1 > (double)P * PGL_NCG_XTOL)) {
        pgl_ncg_finish(s, (updnorm1 != updnorm1) ? PGL_NCG_CGFAIL : PGL_NCG_SUCCESS);
        return PGL_NCG_DONE;
    }
    s->phase = (double)PGL_NCG_CG;
    return PGL_NCG_CG;
}

#endif
