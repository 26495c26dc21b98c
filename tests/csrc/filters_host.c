/* Host build of the rule of the filter bands of one group (theano_pyglm_amd/csrc/pglm_filters.h) for the CPU tests and as the
 * mirror of k_filter_bands:
 *   filters_run   samples (n, C M, P) in the samplers' layout, basis (R, B), c (B) -> out (M, G, R, 5), grp (M, G, 8);
 *                 work: (B + 2) n C doubles;
 *   filters_max_b / filters_max_draws / filters_piece  the constants. */
#include "../../theano_pyglm_amd/csrc/pglm_filters.h"

int filters_max_b(void) { return PGL_FILT_MAX_B; }
int filters_max_draws(void) { return PGL_FILT_MAX_DRAWS; }
int filters_piece(void) { return PGL_FILT_PIECE; }

void filters_run(const double* x, long long n, long long C, long long M, long long P, long long first, long long G, int B,
                 const double* basis, long long R, const double* c, double level, double* out, double* grp, double* work)
{
    for (long long m = 0; m < M; ++m)
        for (long long g = 0; g < G; ++g)
            pgl_filt_group(x + m * P + first + g * B, n, C, C * M * P, M * P, B, basis, R, c, level,
                           out + (m * G + g) * R * PGL_FILT_NLAG, grp + (m * G + g) * PGL_FILT_NGRP, work);
}
