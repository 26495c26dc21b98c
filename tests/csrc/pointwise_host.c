/* Host build of the accumulation of pointwise log-likelihood terms over draws (theano_pyglm_amd/csrc/pglm_pointwise.h) for
 * the CPU tests and as the mirror of k_pw_block's fold:
 *   pw_fold   one draw's values l (n) folded into the state acc (4, n) -- planes m, e, mean, M2, the device's layout with
 *             n = n_blocks * N -- as draw index s;
 *   pw_run    S draws ll (S, n), draw after draw from index 0, into acc (4, n). */
#include "../../theano_pyglm_amd/csrc/pglm_pointwise.h"

int pw_planes(void) { return PGL_PW_NACC; }

void pw_fold(const double* l, long long n, long long s, double* acc)
{
    for (long long i = 0; i < n; ++i) pgl_pw_fold(l[i], s, acc + i, acc + n + i, acc + 2 * n + i, acc + 3 * n + i);
}

void pw_run(const double* ll, long long S, long long n, double* acc)
{
    for (long long s = 0; s < S; ++s) pw_fold(ll + s * n, n, s, acc);
}
