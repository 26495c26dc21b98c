/* Host build of the PSIS-LOO rule of one column (theano_pyglm_amd/csrc/pglm_psis.h) for the CPU tests and as the mirror of
 * k_psis_column:
 *   psis_run   ll (S, C) contiguous -> out (4, C) and, where lw is not null, the log weights (S, C); returns 0, or 1 when the
 *              work space could not be had;
 *   psis_tail  pgl_psis_tail_len;  psis_max_draws  PGL_PSIS_MAX_DRAWS;  psis_planes  PGL_PSIS_NOUT. */
#include <stdlib.h>
#include "../../theano_pyglm_amd/csrc/pglm_psis.h"

int psis_planes(void) { return PGL_PSIS_NOUT; }
long long psis_max_draws(void) { return PGL_PSIS_MAX_DRAWS; }
long long psis_tail(long long S) { return pgl_psis_tail_len(S); }

int psis_run(const double* ll, long long S, long long C, double* out, double* lw)
{
    int* pos = (int*)malloc((size_t)S * sizeof(int));
    double* tail = (double*)malloc((size_t)(2 * pgl_psis_tail_len(S) + 2) * sizeof(double));
    if (!pos || !tail) {
        free(pos);
        free(tail);
        return 1;
    }
    for (long long c = 0; c < C; ++c) pgl_psis_column(ll + c, S, C, out + c, C, lw ? lw + c : (double*)0, pos, tail);
    free(pos);
    free(tail);
    return 0;
}
