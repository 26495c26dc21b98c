// Running accumulation over posterior draws of one pointwise log-likelihood term (one time block of one neuron), in the
// style of pglm_adapt.h: the rule of one (block, neuron) and nothing else -- the caller (k_pw_block of
// pglm_pointwise.hip.h, one thread per (block, neuron); tests/csrc/pointwise_host.c on the host) owns the arrays.
//
// WAIC (Watanabe 2010; Vehtari, Gelman & Gabry 2017) needs two things of the values l_0 .. l_{S-1} a term takes over the
// draws: log mean_s exp(l_s) and the sample variance.  The state is four doubles:
//   m      the running maximum of l;
//   e      sum_s exp(l_s - m), rescaled by exp(m_old - m_new) when m rises: every term is <= 1 and the newest maximum
//          contributes exactly 1, so e lies in [1, S] and   log mean exp = log(e / S) + m;
//   mean   Welford's running mean:  d = l - mean;  mean += d / (s + 1);
//   M2     M2 += d (l - mean), the sum of squared deviations:  var = M2 / (S - 1).
// Draw s = 0 initialises the state (m = l, e = 1, mean = l, M2 = 0): the caller need not clear it.  s >= 1 updates it.  A
// non-finite l (NaN or +-inf) makes the four values NaN, and NaN stays: a state that has met one says so.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_POINTWISE_H
#define PGLM_POINTWISE_H

#include "pglm_hmc.h"

#define PGL_PW_FN PGL_HMC_FN
#define PGL_PW_NACC 4           // planes of the accumulator block (4, n_blocks, N): m, e, mean, M2

PGL_PW_FN void pgl_pw_fold(double l, long long s, double* m, double* e, double* mean, double* m2)
{
    if (!pgl_hmc_finite(l) || (s > 0 && !pgl_hmc_finite(*m))) {
        *m = *e = *mean = *m2 = __builtin_nan("");
        return;
    }
    if (s == 0) {
        *m = l; *e = 1.0; *mean = l; *m2 = 0.0;
        return;
    }
    if (l > *m) {
        *e = *e * exp(*m - l) + 1.0;
        *m = l;
    } else {
        *e += exp(l - *m);
    }
    const double d = l - *mean;
    const double mn = *mean + d / (double)(s + 1);
    *mean = mn;
    *m2 += d * (l - mn);
}

#endif
