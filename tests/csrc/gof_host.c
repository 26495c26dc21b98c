/* Host build of the goodness-of-fit rules (theano_pyglm_amd/csrc/pglm_gof.h) for the CPU tests and as the mirror of
 * k_rcorr_chunk / k_rcorr_finish and k_ks_segment:
 *   gof_uniform   pgl_gof_uniform;  gof_event_term  pgl_gof_event_term;  gof_tile  PGL_KS_TILE;  gof_nout  PGL_KS_NOUT;
 *   gof_ks        segments tau[off[m] .. off[m+1]) -> ks (M, 4) and zs (the length of tau), the network of the header;
 *   gof_corr      the corrected intervals of ONE neuron from its rates lam[0 .. T) over the time range [t_lo, t_lo + T) (stride
 *                 ld) and its event bins ev[0 .. K) relative to t_lo, by the kernels' decomposition: chunks on the ABSOLUTE grid
 *                 of 256 bins (the first and last may be partial), in-chunk sums that start anew behind every event -- per
 *                 event the sum before its bin (pre) and the bin's own rate (qev), per chunk the sum behind its last event
 *                 (tail); j0 = index of ev[0] in the neuron's whole event list.  Writes max(K - 1, 0) doubles. */
#include <stdlib.h>
#include "../../theano_pyglm_amd/csrc/pglm_gof.h"

#define RS_CHUNK 256

double gof_uniform(unsigned long long seed, unsigned long long draw, unsigned long long n, unsigned long long j)
{
    return pgl_gof_uniform(seed, draw, n, j);
}
double gof_event_term(double q, double u) { return pgl_gof_event_term(q, u); }
int gof_tile(void) { return PGL_KS_TILE; }
int gof_nout(void) { return PGL_KS_NOUT; }

void gof_ks(const double* tau, const long long* off, long long M, double* ks, double* zs)
{
    for (long long m = 0; m < M; ++m) pgl_gof_ks_segment(tau + off[m], off[m + 1] - off[m], zs + off[m], ks + m * PGL_KS_NOUT);
}

int gof_corr(const double* lam, long long ld, long long T, long long t_lo, const int* ev, int K, long long j0, int n,
             unsigned long long seed, long long draw, double dt, double* tau)
{
    const long long c0 = t_lo / RS_CHUNK, nchunks = (t_lo + T + RS_CHUNK - 1) / RS_CHUNK - c0;
    double* tail = (double*)malloc((size_t)(nchunks > 0 ? nchunks : 1) * sizeof(double));
    double* pre = (double*)malloc((size_t)(K > 0 ? K : 1) * sizeof(double));
    double* qev = (double*)malloc((size_t)(K > 0 ? K : 1) * sizeof(double));
    if (!tail || !pre || !qev) {
        free(tail); free(pre); free(qev);
        return 1;
    }
    int e = 0;
    for (long long c = 0; c < nchunks; ++c) {
        double since = 0.0;
        long long a = (c0 + c) * RS_CHUNK - t_lo, b = a + RS_CHUNK;
        if (a < 0) a = 0;
        if (b > T) b = T;
        for (long long t = a; t < b; ++t) {
            if (e < K && ev[e] == t) {
                pre[e] = since;
                qev[e] = lam[t * ld];
                since = 0.0;
                ++e;
            } else {
                since += lam[t * ld];
            }
        }
        tail[c] = since;
    }
    for (int i = 1; i < K; ++i) {
        const long long ca = (t_lo + ev[i - 1]) / RS_CHUNK - c0, cb = (t_lo + ev[i]) / RS_CHUNK - c0;
        double s = pre[i];
        if (ca != cb) {
            s = tail[ca];
            for (long long c = ca + 1; c < cb; ++c) s += tail[c];
            s += pre[i];
        }
        tau[i - 1] = pgl_gof_corrected(dt * s, dt * qev[i], pgl_gof_uniform(seed, (pgl_hmc_u64)draw, (pgl_hmc_u64)n, (pgl_hmc_u64)(j0 + i)));
    }
    free(tail); free(pre); free(qev);
    return 0;
}
