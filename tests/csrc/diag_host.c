/* Host build of the convergence-diagnostics rule of one column (theano_pyglm_amd/csrc/pglm_diag.h) for the CPU tests and as the
 * mirror of k_diag_column:
 *   diag_run    x (n, C, K) with leading dimension ld (draw i of chain c of column k at (i * C + c) * ld + k) -> out
 *               (PGL_DIAG_NOUT, K); returns 0, or 1 when the work space could not be had;
 *   diag_score  pgl_diag_score;  diag_max_draws  PGL_DIAG_MAX_DRAWS;  diag_rows  PGL_DIAG_NOUT. */
#include <stdlib.h>
#include "../../theano_pyglm_amd/csrc/pglm_diag.h"

int diag_rows(void) { return PGL_DIAG_NOUT; }
long long diag_max_draws(void) { return PGL_DIAG_MAX_DRAWS; }
double diag_score(double r, double S) { return pgl_diag_score(r, S); }

int diag_run(const double* x, long long n, long long C, long long K, long long ld, double* out)
{
    double* work = (double*)malloc((size_t)(3 * n * C + 2 * C) * sizeof(double));
    if (!work) return 1;
    for (long long k = 0; k < K; ++k) pgl_diag_column(x + k, n, C, C * ld, ld, out + k, K, work);
    free(work);
    return 0;
}
