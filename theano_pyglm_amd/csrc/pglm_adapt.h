// Windowed adaptation of a diagonal mass matrix during the warm-up of the lock-step samplers (mass='adapt' of
// inference/batched_hmc.py and batched_nuts.py), and the seeds of several chains per neuron, in the style of pglm_hmc.h:
// the per-row scalar rules and the per-element updates, no loops over the row -- the caller (the kernels of
// pglm_adapt.hip.h and the ADAPT variant of the NUTS step kernel, one workgroup per row; tests/csrc/adapt_host.c on the
// host) owns the vectors.
//
// The scheme is Stan's (Stan Reference Manual, "Automatic parameter tuning": the windowed adaptation of the inverse metric):
//   schedule      computed on the host (inference/mass_adapt.py: adapt_windows) from n = n_warmup:  n < 20: no window;
//                 n >= 150: init = 75, term = 50, base = 25;  else init = floor(0.15 n), term = floor(0.10 n), base =
//                 n - init - term.  Windows start at init, have sizes base, 2 base, 4 base, ... and end no later than
//                 n - term; a window whose doubled successor would not fit completely is stretched to n - term.
//                 The kernels get it as ints  sched = [n_win, start of window 0, end of window 0, end of window 1, ...]
//                 (window k + 1 starts where window k ends).
//   estimate      per row and parameter a Welford count n, mean and M2 over the row's point q after every transition t of
//                 the running window (a rejected transition contributes the repeated point):
//                     d = q - mean;  mean += d / n;  M2 += d (q - mean).
//                 After the transition t with t + 1 = the window's end:  var = M2 / (n - 1),
//                     minv = n / (n + 5) var + 1e-3 * 5 / (n + 5)        (a non-finite value becomes 1),
//                 the row of minv is rewritten, count, mean and M2 are zeroed, the window index advances, and the
//                 step-size adaptation of the row restarts:  HMC: avg_accept = PGL_HMC_AVG0, step kept;  NUTS: mu =
//                 log(10 step), hbar = 0, log ebar = 0 and the iterate m of pgl_nuts_adapt_from counts from the window's end.
//                 After the last window minv is never written again.
//   exactness     a transition runs wholly under one minv: the switch happens after the end of transition t and before the
//                 momentum of transition t + 1 is drawn.
//   chains        chain c of a run with seed s runs on the seed pgl_chain_seed(s, c):  c = 0: s itself;  else
//                 mix(mix(s + G) ^ (G c)), mix and G of pglm_hmc.h.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_ADAPT_H
#define PGLM_ADAPT_H

#include "pglm_nuts.h"

#define PGL_ADAPT_FN PGL_HMC_FN
#define PGL_ADAPT_REG 1e-3
#define PGL_ADAPT_SHRINK 5.0

// The adaptation state of R rows of P parameters is ONE block of doubles: mean (R, P), M2 (R, P), then the fields of
// PglAdapt, field-major (R) each.
#define PGL_ADAPT_NVEC 2
#define PGL_ADAPT_NSCAL 2
typedef struct {
    double count;               // points in the running window so far
    double widx;                // index of the running window (n_win: adaptation has ended)
} PglAdapt;

enum { PGL_ADAPT_ACC = 1,       // the row's point enters the running window (a->count is its number, from 1)
       PGL_ADAPT_SWITCH = 2 };  // ... and completes it: finalise with n = *n_out, then zero mean and M2

// after transition t of a row (t counted from 0).  *n_out: the count to use in the element rules.
PGL_ADAPT_FN int pgl_adapt_row(PglAdapt* a, const int* sched, int t, double* n_out)
{
    const int w = (int)a->widx;
    if (w >= sched[0] || t < sched[1]) return 0;
    a->count += 1.0;
    *n_out = a->count;
    if (t + 1 != sched[2 + w]) return PGL_ADAPT_ACC;
    a->count = 0.0;
    a->widx += 1.0;
    return PGL_ADAPT_ACC | PGL_ADAPT_SWITCH;
}
// the transitions completed when the row's step-size adaptation was last restarted (pgl_nuts_adapt_from's m0)
PGL_ADAPT_FN double pgl_adapt_restart_t(const PglAdapt* a, const int* sched)
{
    const int w = (int)a->widx;
    return w > 0 ? (double)sched[1 + w] : 0.0;
}

// ---- per element ----
PGL_ADAPT_FN void pgl_adapt_welford(double q, double n, double* mean, double* m2)
{
    const double d = q - *mean;
    const double mn = *mean + d / n;
    *mean = mn;
    *m2 += d * (q - mn);
}
PGL_ADAPT_FN double pgl_adapt_minv(double m2, double n)
{
    const double var = m2 / (n - 1.0);
    const double v = (n / (n + PGL_ADAPT_SHRINK)) * var + PGL_ADAPT_REG * (PGL_ADAPT_SHRINK / (n + PGL_ADAPT_SHRINK));
    return pgl_hmc_finite(v) ? v : 1.0;
}

// ---- the restart of the step-size adaptation at a window's end ----
PGL_ADAPT_FN void pgl_adapt_restart_hmc(PglHmc* s) { s->avg_accept = PGL_HMC_AVG0; }
PGL_ADAPT_FN void pgl_adapt_restart_nuts(PglNuts* s)
{
    s->mu = log(10.0 * s->step);
    s->hbar = 0.0;
    s->logeps_bar = 0.0;
}

// ---- chains ----
PGL_ADAPT_FN pgl_hmc_u64 pgl_chain_seed(pgl_hmc_u64 seed, pgl_hmc_u64 c)
{
    return c == 0 ? seed : pgl_hmc_mix(pgl_hmc_mix(seed + PGL_HMC_G) ^ (PGL_HMC_G * c));
}

#endif
