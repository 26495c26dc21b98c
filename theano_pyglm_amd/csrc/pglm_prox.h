// Accelerated proximal gradient (FISTA) for the group-lasso MAP of one row (one neuron's parameter vector) as a
// reverse-communication state machine: the scalar decisions and the per-element / per-group updates of the algorithm, no
// loops over the row and no callbacks -- the caller (the k_prox_* row kernels of pglm_prox.hip.h, one workgroup per neuron;
// tests/csrc/prox_host.c on the host) owns the vectors, computes the reductions and supplies ll and its gradient.  Every
// row asks for exactly one evaluation per call, so M fits advance in lock step: one ll+grad launch per call
// (inference/batched_prox.py).
//
// The objective of a row [b, s (Ds), w (N groups of B)]:
//   smooth      f = -ll - log N(b; mu_b, sg_b) - log N(s; 0, stim_sigma): the bias and stimulus terms of pgl_bfgs_objective_dev
//               (bias.py:33, bkgd.py:76).  Rules of the other row kernels: a non-finite f is +inf (a trial there fails and
//               the step halves), a NaN or infinite gradient entry becomes 0;
//   non-smooth  h = (lam / sigma) sum_g |w_g - mu|_2, minus GroupLasso.log_p (priors.py:202), lam one number PER ROW;
//   F = f + h   minus compute_log_p's per-neuron term under a GroupLasso impulse prior;
//   prox_{t h}  group by group  w_g <- mu + (v_g - mu) max(0, 1 - t lam / (sigma |v_g - mu|)), the factor 0 when the norm is
//               0; bias and stimulus entries pass through.  A shrunk group is EXACTLY mu: the support can be read off.
//
// The algorithm is Beck & Teboulle (2009), FISTA with backtracking, with the function restart of O'Donoghue & Candes
// (2015).  Per iteration, from the extrapolated point y with (f_y, g_y) known:
//   trial       z = prox_{t h}(y - t g_y), evaluated;
//   1           sufficient decrease  f_z <= f_y + <g_y, z - y> + |z - y|^2 / (2 t) + PGL_PROX_C max(1, |f_y|), f_z finite;
//   2           on failure t <- t / 2 and a new trial; after max_backtrack failures in one iteration the row ends (status 2);
//   3           on pass with F_z > F_x and y != x: restart -- z is dropped, y = x with its known (f, g), tk = 1, t <- 2 t,
//               and the new trial goes out at once (no evaluation is wasted);
//   4           otherwise accept: xprev = x, x = z, g_x = g_z, iters += 1;
//   5           the KKT residual r at x from g_x, the largest of |g| over bias and stimulus entries,
//               |g_g + (lam / sigma) (w_g - mu) / |w_g - mu| |_inf over the non-zero groups and max(0, |g_g|_2 - lam / sigma)
//               over the zero groups;
//   6           r <= gtol ends the row (status 0), iters == maxiter ends it (status 1);
//   7           tk' = (1 + sqrt(1 + 4 tk^2)) / 2, beta = (tk - 1) / tk'.  beta = 0 (the iteration after a start or a restart):
//               y = x, whose (f, g) are known, and the next trial goes out directly; else y = x + beta (x - xprev) is
//               evaluated first (phase PGL_PROX_Y) and the trial follows.  A non-finite f_y forces a restart from x (tk = 1,
//               t kept).
// So an iteration costs two evaluations, one on the iteration after a restart.
// What differs from the textbook: the function restart; t doubles on a restart and never grows otherwise (a restart is the
// sign that the momentum overshot, and the only moment at which a larger step is tried); the first step is BFGS's,
// t = min(1, 1.01 / |g|_2); and the rounding allowance PGL_PROX_C in test 1.
//
// PGL_PROX_C: at convergence |z - y|^2 / (2 t) falls below the rounding of f, and test 1 without an allowance fails for
// ever on noise.  The noise is that of ll: between two summation orders of the same arithmetic (oracle/glm_oracle.c against
// oracle/glm_blocked.c, and the numpy oracle against both) ll of the test problems (N = 1 .. 70, nT = 2000 .. 5000, both
// nonlinearities, dense and all-zero impulse weights) differs by at most 2.4e-14 max(1, |ll|) (C against C) and 9.6e-14 (numpy
// against C).  The allowance is ten times the larger figure.  It bounds how much an accepted step from y = x can raise F:
// F_z <= F_x - |z - x|^2 / (2 t) + PGL_PROX_C max(1, |f_x|).
//
// The machine records the smallest margin of each kind of decision it has taken (m_*: how far the compared quantities
// were apart, relative to their size), so a test can tell whether a last-place difference could have flipped one.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_PROX_H
#define PGLM_PROX_H

#include "pglm_hmc.h"

#define PGL_PROX_FN PGL_LS_FN

#define PGL_PROX_C 1e-12

// phase of a row: what its row of d_Xt holds
#define PGL_PROX_Y 0            // the extrapolated point y: (f_y, g_y) come in with the next call
#define PGL_PROX_TRIAL 1        // the trial z
#define PGL_PROX_DONE 2         // x: the row has ended (status) and is never written again
// status of an ended row
#define PGL_PROX_CONVERGED 0
#define PGL_PROX_MAXITER 1
#define PGL_PROX_STEPFAIL 2
// outcome of a trial
#define PGL_PROX_D_BACKTRACK 0
#define PGL_PROX_D_FAIL 1
#define PGL_PROX_D_RESTART 2
#define PGL_PROX_D_ACCEPT 3

// The state of M rows of P parameters is ONE block of doubles: PGL_PROX_NVEC (M, P) arrays -- x, xprev, y, g_x, g_y --
// then PGL_PROX_NSCAL (M) arrays, field-major, the fields of PglProx in order.
#define PGL_PROX_NVEC 5
#define PGL_PROX_NSCAL 17

typedef struct {
    double f_x, F_x, f_y;       // smooth part and objective at x, smooth part at y
    double t, tk;               // step, momentum parameter
    double iters, nfev;         // accepted steps, evaluations (the one before init included)
    double nbt, restarts;       // failed trials of the running iteration, restarts so far
    double phase, status;
    double kkt;                 // KKT residual at x
    double y_is_x;              // 1: y = x (a start or a restart: test 3 is off)
    double m_sd, m_restart, m_zero, m_kkt;   // smallest margins: test 1, test 3, a group against its threshold, r against gtol
} PglProx;

PGL_PROX_FN double pgl_prox_min(double a, double b) { return b < a ? b : a; }
PGL_PROX_FN double pgl_prox_size(double a) { const double m = pgl_ls_abs(a); return m > 1.0 ? m : 1.0; }

// ---- per group ----
// z_g = prox of v_g = y_g - t g_g with threshold thr = t lam / sigma.  *margin: |1 - thr / |v_g - mu|| (inf when the norm
// is 0 or the threshold infinite: nothing was decided).
PGL_PROX_FN void pgl_prox_group(const double* y, const double* g, int B, double t, double mu, double thr, double* z,
                                double* margin)
{
    double ss = 0.0;
    for (int b = 0; b < B; ++b) {
        const double d = (y[b] - t * g[b]) - mu;
        ss += d * d;
    }
    const double nrm = sqrt(ss);
    double fac = 0.0;
    *margin = (double)INFINITY;
    if (nrm > 0.0) {
        const double q = thr / nrm;
        fac = q < 1.0 ? 1.0 - q : 0.0;
        if (pgl_hmc_finite(q)) *margin = pgl_ls_abs(1.0 - q);
    }
    for (int b = 0; b < B; ++b) z[b] = mu + ((y[b] - t * g[b]) - mu) * fac;
}
// the group's term of h: (lam / sigma) |w_g - mu|, 0 for a zero group whatever lam is (lam = +inf included)
PGL_PROX_FN double pgl_prox_group_h(const double* w, int B, double mu, double lam_s)
{
    double ss = 0.0;
    for (int b = 0; b < B; ++b) {
        const double d = w[b] - mu;
        ss += d * d;
    }
    return ss > 0.0 ? lam_s * sqrt(ss) : 0.0;
}
// the group's term of the KKT residual from g = grad f
PGL_PROX_FN double pgl_prox_group_kkt(const double* w, const double* g, int B, double mu, double lam_s)
{
    double ss = 0.0, gg = 0.0;
    for (int b = 0; b < B; ++b) {
        const double d = w[b] - mu;
        ss += d * d;
        gg += g[b] * g[b];
    }
    if (ss > 0.0) {
        const double nrm = sqrt(ss);
        double r = 0.0;
        for (int b = 0; b < B; ++b) {
            const double v = g[b] + lam_s * ((w[b] - mu) / nrm);
            const double a = v == v ? pgl_ls_abs(v) : (double)INFINITY;
            r = a > r ? a : r;
        }
        return r;
    }
    const double e = sqrt(gg) - lam_s;
    return e > 0.0 ? e : 0.0;
}

// ---- the scalar state ----
PGL_PROX_FN void pgl_prox_finish(PglProx* s, int status)
{
    s->phase = (double)PGL_PROX_DONE;
    s->status = (double)status;
}
// start: f_x, h_x at x, gg = |g_x|_2^2
PGL_PROX_FN void pgl_prox_init(PglProx* s, double f_x, double h_x, double gg)
{
    const double t0 = 1.01 / sqrt(gg);
    s->f_x = f_x; s->F_x = f_x + h_x; s->f_y = f_x;
    s->t = t0 < 1.0 ? t0 : 1.0;
    s->tk = 1.0;
    s->iters = 0.0; s->nfev = 1.0; s->nbt = 0.0; s->restarts = 0.0;
    s->phase = (double)PGL_PROX_TRIAL; s->status = 0.0;
    s->kkt = (double)INFINITY;
    s->y_is_x = 1.0;
    s->m_sd = s->m_restart = s->m_zero = s->m_kkt = (double)INFINITY;
}
// steps 5 and 6 with the residual r at x.  Returns 1 when the row has ended.
PGL_PROX_FN int pgl_prox_kkt_test(PglProx* s, double r, double gtol, int maxiter)
{
    s->kkt = r;
    if (pgl_hmc_finite(r)) s->m_kkt = pgl_prox_min(s->m_kkt, pgl_ls_abs(r - gtol) / gtol);
    if (r <= gtol) {
        pgl_prox_finish(s, PGL_PROX_CONVERGED);
        return 1;
    }
    if (s->iters >= (double)maxiter) {
        pgl_prox_finish(s, PGL_PROX_MAXITER);
        return 1;
    }
    return 0;
}
// steps 1 to 4 for the evaluated trial z: f_z, h_z = h(z), dot = <g_y, z - y>, dd = |z - y|^2
PGL_PROX_FN int pgl_prox_decide(PglProx* s, double f_z, double h_z, double dot, double dd, int max_backtrack)
{
    s->nfev += 1.0;
    const double rhs = s->f_y + dot + dd / (2.0 * s->t) + PGL_PROX_C * pgl_prox_size(s->f_y);
    const int pass = pgl_hmc_finite(f_z) && f_z <= rhs;
    if (pgl_hmc_finite(f_z) && pgl_hmc_finite(rhs)) s->m_sd = pgl_prox_min(s->m_sd, pgl_ls_abs(rhs - f_z) / pgl_prox_size(s->f_y));
    if (!pass) {
        s->nbt += 1.0;
        if (s->nbt >= (double)max_backtrack) {
            pgl_prox_finish(s, PGL_PROX_STEPFAIL);
            return PGL_PROX_D_FAIL;
        }
        s->t *= 0.5;
        return PGL_PROX_D_BACKTRACK;
    }
    const double F_z = f_z + h_z;
    if (s->y_is_x == 0.0) {
        if (pgl_hmc_finite(F_z) && pgl_hmc_finite(s->F_x))
            s->m_restart = pgl_prox_min(s->m_restart, pgl_ls_abs(F_z - s->F_x) / pgl_prox_size(s->F_x));
        if (F_z > s->F_x) {
            s->y_is_x = 1.0; s->f_y = s->f_x; s->tk = 1.0; s->t *= 2.0; s->restarts += 1.0;
            return PGL_PROX_D_RESTART;
        }
    }
    s->f_x = f_z; s->F_x = F_z;
    s->iters += 1.0; s->nbt = 0.0;
    return PGL_PROX_D_ACCEPT;
}
// step 7.  Returns beta; beta == 0: y = x (the caller copies x and g_x), the phase stays PGL_PROX_TRIAL.
PGL_PROX_FN double pgl_prox_momentum(PglProx* s)
{
    const double tk1 = 0.5 * (1.0 + sqrt(1.0 + 4.0 * s->tk * s->tk));
    const double beta = (s->tk - 1.0) / tk1;
    s->tk = tk1;
    if (beta == 0.0) {
        s->y_is_x = 1.0; s->f_y = s->f_x;
        s->phase = (double)PGL_PROX_TRIAL;
    } else {
        s->y_is_x = 0.0;
        s->phase = (double)PGL_PROX_Y;
    }
    return beta;
}
// phase PGL_PROX_Y: f_y has arrived.  Returns 1 when y stands, 0 when the caller has to restart from x (y = x, g_y = g_x).
PGL_PROX_FN int pgl_prox_y_arrived(PglProx* s, double f_y)
{
    s->nfev += 1.0;
    s->phase = (double)PGL_PROX_TRIAL;
    if (!pgl_hmc_finite(f_y)) {
        s->y_is_x = 1.0; s->f_y = s->f_x; s->tk = 1.0; s->restarts += 1.0;
        return 0;
    }
    s->f_y = f_y;
    return 1;
}
// per element
PGL_PROX_FN double pgl_prox_extrapolate(double x, double xprev, double beta) { return x + beta * (x - xprev); }
PGL_PROX_FN double pgl_prox_plain_step(double y, double t, double g) { return y - t * g; }

#endif
