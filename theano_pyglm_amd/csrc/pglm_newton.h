// Dense-Hessian Newton optimiser of one row as a reverse-communication state machine: the scalar decisions of the
// algorithm, no loops over the row and no callbacks -- the caller (the k_newton_* row kernels of pglm_newton.hip.h, one
// workgroup per neuron; tests/csrc/newton_host.c on the host) owns the vectors, computes the reductions (dot products,
// max|g|) and supplies f, g and the solve's output.  That is what lets all neurons of a range advance in lock step: one
// Hessian contraction, one batched factorisation and one batched solve per outer iteration for the rows still running,
// one ll+grad launch per line-search trial (inference/batched_newton.py).
//
// The algorithm is the line-search Newton method with Hessian modification of Nocedal & Wright, "Numerical Optimization",
// 2nd ed., section 3.4 (the reference's default second-order route: parallel_coord_descent.py:62 use_hessian=True,
// map.py:38-45 hands the dense Hessian to scipy's Newton-CG):
//   outer iteration k at x_k with gradient g and A = -(Hessian of ll + Hessian of the log prior):
//     factor  A + shift * diag(A)  (equilibrated Cholesky, pgl_chol_factor_dev),  p = -(A + shift diag A)^-1 g;
//     shift = 0 first.  A factor that fails (A not positive definite, a non-finite entry) or a direction that does not
//     descend (g.p not < 0, or not finite) raises the shift along the ladder
//         0 -> PGL_NEWTON_SHIFT0 = 1e-6 -> x PGL_NEWTON_SHIFT_MUL = 100 -> ... -> PGL_NEWTON_SHIFT_MAX = 1e2
//     (six factorisations at most: 0, 1e-6, 1e-4, 1e-2, 1, 1e2) and asks for the factorisation again -- of the SAME
//     Hessian: the caller keeps it.  The shift scales with diag A, so the modified matrix keeps A's equilibration.  When
//     the last rung fails too the row takes the steepest-descent direction p = -g;
//   strong-Wolfe line search along p (pglm_linesearch.h: MINPACK-2 DCSRCH with the constants the Newton-CG rows use:
//     c1 = 1e-4, c2 = 0.9, xtol = 1e-14, steps in [1e-8, 50], at most 100 trials), first trial step 1 -- the Newton step;
//   x_{k+1} = x_k + alpha p;  stop when max|g(x_{k+1})| <= gtol (status 0), after maxiter outer iterations (status 1);
//   the shift returns to 0 at every new point.
// NaN rules of fit_glm (coord_descent.py:170-182): objective NaN -> 1e16, a gradient holding a NaN -> 0; the caller
// applies them before it hands the numbers in.
// When the search gives up (warning, 100 trials, non-finite value) the best sufficient-decrease point of the search is
// taken if there is one (the trial itself or the best step so far, whose value is the line search's own fx), else the row
// stops with status 2, as the lock-step BFGS and Newton-CG rows do.  Status 3: not even -g descends (its norm is not
// finite or zero with max|g| > gtol).
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_NEWTON_H
#define PGLM_NEWTON_H

#include "pglm_linesearch.h"

#define PGL_NEWTON_FN PGL_LS_FN

// phase of a row
#define PGL_NEWTON_HESS 0       // needs the Hessian at its point: assemble, factor, solve, direction
#define PGL_NEWTON_SEARCH 1     // its line search runs: evaluate f, g at x + alpha p
#define PGL_NEWTON_DONE 2       // finished (status >= 0): nothing of the row is written again
#define PGL_NEWTON_REFACTOR 3   // its shift was raised: assemble from the SAME Hessian, factor, solve, direction

#define PGL_NEWTON_RUNNING (-1)
#define PGL_NEWTON_SUCCESS 0
#define PGL_NEWTON_MAXITER 1
#define PGL_NEWTON_PRLOSS 2     // the line search found no acceptable point
#define PGL_NEWTON_NODESCENT 3  // no descent direction, not even -g

#define PGL_NEWTON_SHIFT0 1e-6
#define PGL_NEWTON_SHIFT_MUL 100.0
#define PGL_NEWTON_SHIFT_MAX 1e2

#define PGL_NEWTON_C1 1e-4
#define PGL_NEWTON_C2 0.9
#define PGL_NEWTON_LS_XTOL 1e-14
#define PGL_NEWTON_STPMIN 1e-8
#define PGL_NEWTON_STPMAX 50.0
#define PGL_NEWTON_MAX_TRIALS 100

// outcome of pgl_newton_direction
#define PGL_NEWTON_DIR_NEWTON 0     // the search starts along the solve's output
#define PGL_NEWTON_DIR_REFACTOR 1   // the shift was raised: factor again
#define PGL_NEWTON_DIR_STEEPEST 2   // the ladder is used up: the search starts along -g
#define PGL_NEWTON_DIR_FAIL 3       // status 3

// outcome of pgl_newton_search_step
#define PGL_NEWTON_LS_EVALUATE PGL_LS_EVALUATE     // evaluate at s->alpha next (ls->moved: the trial became the best step)
#define PGL_NEWTON_LS_TAKE_TRIAL PGL_LS_TAKE_TRIAL // the row takes the trial just evaluated
#define PGL_NEWTON_LS_TAKE_BEST PGL_LS_TAKE_BEST   // the row takes the best step saved so far (value *facc)
#define PGL_NEWTON_LS_FAIL PGL_LS_FAIL             // no acceptable point: status 2

#define PGL_NEWTON_NSCAL 11

typedef struct {
    double f, fprev;            // objective at x_k and at x_{k-1}
    double slope, alpha;        // phi'(0) of the running search, its next trial step
    double shift;               // the diagonal shift of the current factorisation (relative to diag A)
    double nit, nfev;           // outer iterations, objective evaluations (the starting point counts)
    double nhess, nfact;        // Hessians used, factorisations tried
    double status, phase;
} PglNewton;

PGL_NEWTON_FN int pgl_newton_finite(double x) { return pgl_ls_finite(x); }

PGL_NEWTON_FN void pgl_newton_finish(PglNewton* s, int status)
{
    s->status = (double)status;
    s->phase = (double)PGL_NEWTON_DONE;
}

// start of a fit: f = f(x_0) (NaN rule applied), gmax = max|g(x_0)|.  Returns the phase.
PGL_NEWTON_FN int pgl_newton_init(PglNewton* s, double f, double gmax, double gtol, int maxiter)
{
    s->f = f; s->fprev = f; s->slope = 0.0; s->alpha = 0.0; s->shift = 0.0;
    s->nit = 0.0; s->nfev = 1.0; s->nhess = 0.0; s->nfact = 0.0;
    s->status = (double)PGL_NEWTON_RUNNING; s->phase = (double)PGL_NEWTON_HESS;
    if (maxiter <= 0) pgl_newton_finish(s, PGL_NEWTON_MAXITER);
    else if (gmax <= gtol) pgl_newton_finish(s, PGL_NEWTON_SUCCESS);
    return (int)s->phase;
}

// the next rung of the ladder above `shift`, or a negative number when `shift` is the last one (the factor 1.5 absorbs the
// rounding of the repeated product)
PGL_NEWTON_FN double pgl_newton_next_shift(double shift)
{
    const double next = shift == 0.0 ? PGL_NEWTON_SHIFT0 : shift * PGL_NEWTON_SHIFT_MUL;
    return next <= 1.5 * PGL_NEWTON_SHIFT_MAX ? next : -1.0;
}

// The factorisation of A + shift diag A and the solve p = -(..)^-1 g have run: failed = the factor flagged the row,
// slope = g . p, gg = g . g.  Starts the line search (ls) along p or along -g, or asks for another factorisation.
PGL_NEWTON_FN int pgl_newton_direction(PglNewton* s, PglLs* ls, int failed, double slope, double gg)
{
    int d = PGL_NEWTON_DIR_NEWTON;
    if (s->phase == (double)PGL_NEWTON_HESS) s->nhess += 1.0;
    s->nfact += 1.0;
    if (failed || !(slope < 0.0) || !pgl_newton_finite(slope)) {
        const double next = pgl_newton_next_shift(s->shift);
        if (next > 0.0) {
            s->shift = next;
            s->phase = (double)PGL_NEWTON_REFACTOR;
            return PGL_NEWTON_DIR_REFACTOR;
        }
        slope = -gg;
        d = PGL_NEWTON_DIR_STEEPEST;
        if (!(slope < 0.0) || !pgl_newton_finite(slope)) {
            pgl_newton_finish(s, PGL_NEWTON_NODESCENT);
            return PGL_NEWTON_DIR_FAIL;
        }
    }
    s->slope = slope;
    s->alpha = 1.0;
    pgl_ls_start(ls, 1.0, s->f, slope, PGL_NEWTON_C1, PGL_NEWTON_STPMIN, PGL_NEWTON_STPMAX);
    s->phase = (double)PGL_NEWTON_SEARCH;
    return d;
}

// The trial x + s->alpha p has been evaluated: f (NaN rule applied), dphi = g_trial . p.  pgl_ls_guarded_step on the line
// search's own value at the best step (ls->fx).  *facc: the value of the point the row takes (TAKE_TRIAL: f, TAKE_BEST:
// the value at the best step before this call).
PGL_NEWTON_FN int pgl_newton_search_step(PglNewton* s, PglLs* ls, double f, double dphi, double* facc)
{
    double alpha_acc;                                    // (not kept: the row moves to a saved point)
    s->nfev += 1.0;
    *facc = f;
    const int d = pgl_ls_guarded_step(ls, f, dphi, ls->fx, PGL_NEWTON_C1, PGL_NEWTON_C2, PGL_NEWTON_LS_XTOL,
                                      PGL_NEWTON_STPMIN, PGL_NEWTON_STPMAX, PGL_NEWTON_MAX_TRIALS, &alpha_acc, facc);
    if (d == PGL_LS_EVALUATE) s->alpha = ls->stp;
    else if (d == PGL_LS_FAIL) pgl_newton_finish(s, PGL_NEWTON_PRLOSS);
    return d;
}

// The row has moved to a point with value fnew and gradient maximum gmax.  Returns the phase: PGL_NEWTON_DONE (converged:
// status 0; maxiter: status 1) or PGL_NEWTON_HESS.
PGL_NEWTON_FN int pgl_newton_accept(PglNewton* s, double fnew, double gmax, double gtol, int maxiter)
{
    s->fprev = s->f;
    s->f = fnew;
    s->nit += 1.0;
    s->shift = 0.0;
    if (gmax <= gtol) pgl_newton_finish(s, PGL_NEWTON_SUCCESS);
    else if (s->nit >= (double)maxiter) pgl_newton_finish(s, PGL_NEWTON_MAXITER);
    else s->phase = (double)PGL_NEWTON_HESS;
    return (int)s->phase;
}

#endif
