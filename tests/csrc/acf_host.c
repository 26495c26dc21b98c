/* Host build of the independence rule (theano_pyglm_amd/csrc/pglm_acf.h) for the CPU tests and as the mirror of k_acf_segment:
 *   acf_score        pgl_acf_score;  acf_max_lag / acf_nhead / acf_piece  the constants;
 *   acf_segments     segments of runs of tau -> out (M, 6 + L) and the scores (the length of tau);
 *   acf_from_scores  the same statistics from GIVEN scores g (the device's own, say); tau is read for the void rule only.
 * Returns 1 where memory runs out. */
#include <stdlib.h>
#include "../../theano_pyglm_amd/csrc/pglm_acf.h"

double acf_score(double tau) { return pgl_acf_score(tau); }
int acf_max_lag(void) { return PGL_ACF_MAX_LAG; }
int acf_nhead(void) { return PGL_ACF_NHEAD; }
int acf_piece(void) { return PGL_ACF_PIECE; }

int acf_from_scores(const double* tau, const double* g, const long long* run_off, const long long* seg_run, long long M, int L,
                    double* out)
{
    for (long long m = 0; m < M; ++m) {
        const long long r0 = seg_run[m], r1 = seg_run[m + 1], o0 = run_off[r0], n = run_off[r1] - o0;
        double* d = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
        long long* end = (long long*)malloc((size_t)(n > 0 ? n : 1) * sizeof(long long));
        if (!d || !end) {
            free(d); free(end);
            return 1;
        }
        pgl_acf_stats(g + o0, run_off + r0, r1 - r0, L, pgl_acf_bad_any(tau + o0, n), d, end, out + m * (PGL_ACF_NHEAD + L));
        free(d); free(end);
    }
    return 0;
}

int acf_segments(const double* tau, const long long* run_off, const long long* seg_run, long long M, int L, double* out, double* g)
{
    const long long total = run_off[seg_run[M]];
    for (long long i = run_off[seg_run[0]]; i < total; ++i) g[i] = pgl_acf_score(tau[i]);
    return acf_from_scores(tau, g, run_off, seg_run, M, L, out);
}
