/* Host build of the Wald rule of one coupling group (theano_pyglm_amd/csrc/pglm_wald.h) for the CPU tests and as the mirror of
 * k_wald_groups:
 *   wald_run    W (M, P, ld), theta (M, P), c (B), info (M) int32 or null -> out (M, G, 4) and, where u is not null,
 *               u (G M, P) with row g M + m; a row with info != 0 is NaN throughout and is not read;
 *   wald_max_b / wald_nout / wald_lanes  the constants. */
#include "../../theano_pyglm_amd/csrc/pglm_wald.h"

int wald_max_b(void) { return PGL_WALD_MAX_B; }
int wald_nout(void) { return PGL_WALD_NOUT; }
int wald_lanes(void) { return PGL_WALD_LANES; }

void wald_run(const double* W, long long M, long long P, long long ld, const double* theta, long long first, long long G, int B,
              const double* c, const int* info, double* out, double* u)
{
    const double nan = __builtin_nan("");
    for (long long m = 0; m < M; ++m)
        for (long long g = 0; g < G; ++g) {
            double* o4 = out + (m * G + g) * PGL_WALD_NOUT;
            double* ur = u ? u + (g * M + m) * P : (double*)0;
            if (info && info[m] != 0) {
                for (int q = 0; q < PGL_WALD_NOUT; ++q) o4[q] = nan;
                if (ur) for (long long k = 0; k < P; ++k) ur[k] = nan;
                continue;
            }
            pgl_wald_group(W + m * P * ld, P, ld, theta + m * P, first + g * B, B, c, o4, ur);
        }
}
