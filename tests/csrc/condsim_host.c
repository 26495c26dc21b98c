/* Host build of the rules of the clamped simulation (theano_pyglm_amd/csrc/pglm_condsim.h) for the CPU tests and as the mirror
 * of k_cond_currents / k_simulate_cond:
 *   condsim_currents   X0 (nT, N), AW (N, R, N), the event lists -> Xc (nT, N);
 *   condsim_run        Xc, AW -> S (n_rep, nT, N) uint8 of the replicates rep0 .. rep0 + n_rep - 1; exc (N) is ADDED to; the
 *                      smallest decision margin of all chains; work: nT + R doubles;
 *   condsim_fold       S (n_rep, nT, N), obs (n_win, N) -> acc (6, n_win, N), initialised unless accumulate;
 *   condsim_queue / condsim_cap   the constants. */
#include "../../theano_pyglm_amd/csrc/pglm_condsim.h"

int condsim_queue(void) { return PGL_CS_QUEUE; }
int condsim_cap(void) { return PGL_CS_CAP; }

void condsim_currents(const double* X0, const double* AW, const int* ev_pre, const unsigned char* ev_cnt, const long long* bin_off,
                      long long nT, int N, int R, double* Xc)
{
    for (long long t = 0; t < nT; ++t)
        for (int q = 0; q < N; ++q) Xc[t * N + q] = pgl_cs_current(t, q, N, R, X0, AW, ev_pre, ev_cnt, bin_off);
}

double condsim_run(const double* Xc, const double* AW, long long nT, int N, int R, int nlin, double dt, unsigned long long seed,
                   int rep0, int n_rep, unsigned char* S, long long* exc, double* work)
{
    double closest = __builtin_huge_val();
    double* x = work;
    double* h = work + nT;
    for (int i = 0; i < n_rep; ++i)
        for (int n = 0; n < N; ++n) {
            for (long long t = 0; t < nT; ++t) x[t] = Xc[t * N + n];
            for (int tau = 0; tau < R; ++tau) h[tau] = AW[((long long)n * R + tau) * N + n];
            exc[n] += pgl_cs_chain(nT, R, nlin, dt, x, h, seed, (pgl_cs_u64)(rep0 + i), (pgl_cs_u64)n, S + (i * nT) * N + n, N,
                                   &closest);
        }
    return closest;
}

void condsim_fold(const unsigned char* S, int n_rep, long long nT, int N, long long win, const long long* obs, long long* acc,
                  int accumulate)
{
    const long long plane = pgl_cs_windows(nT, win) * N;
    if (!accumulate) pgl_cs_acc_init(acc, plane);
    for (int i = 0; i < n_rep; ++i)
        for (int n = 0; n < N; ++n) pgl_cs_fold(nT, win, S + (i * nT) * N + n, N, obs + n, acc + n, plane, N);
}
