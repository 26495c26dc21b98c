/* Host build of the rate-window rule (theano_pyglm_amd/csrc/pglm_ratewin.h) for the CPU tests and as the mirror of
 * k_rw_window's fold:
 *   rw_midp     the mid-p values u (n) of the counts y (n) under Poisson laws of means lam (n);
 *   rw_fold     one draw's expected counts lam (n) and the observed counts y (n) folded into the state acc (5, n) -- planes
 *               mean, M2, min, max, pit, the device's layout with n = n_win * N -- as draw index s;
 *   rw_run      S draws lam (S, n), draw after draw from index 0, into acc (5, n);
 *   rw_counts   Lam (n_win) and obs (n_win) of one neuron from its rates lam_t (n bins) and spike counts, in the header's order:
 *               pieces of at most 256 bins from the window's own first bin, each summed in time order, added in piece order. */
#include "../../theano_pyglm_amd/csrc/pglm_ratewin.h"

int rw_planes(void) { return PGL_RW_NACC; }
int rw_max_count(void) { return PGL_RW_MAX_COUNT; }
double rw_max_lam(void) { return PGL_RW_MAX_LAM; }
long long rw_windows(long long n, long long win) { return pgl_rw_windows(n, win); }

void rw_midp(const double* lam, const double* y, long long n, double* u)
{
    for (long long i = 0; i < n; ++i) u[i] = pgl_rw_midp(lam[i], y[i]);
}

void rw_fold(const double* lam, const double* y, long long n, long long s, double* acc)
{
    for (long long i = 0; i < n; ++i)
        pgl_rw_fold(lam[i], y[i], s, acc + i, acc + n + i, acc + 2 * n + i, acc + 3 * n + i, acc + 4 * n + i);
}

void rw_run(const double* lam, const double* y, long long S, long long n, double* acc)
{
    for (long long s = 0; s < S; ++s) rw_fold(lam + s * n, y, n, s, acc);
}

void rw_counts(const double* lam_t, const int* spikes, long long n, long long win, double dt, double* Lam, double* obs)
{
    const long long n_win = pgl_rw_windows(n, win);
    for (long long w = 0; w < n_win; ++w) {
        const long long t0 = w * win, len = (n - t0 < win) ? n - t0 : win;
        double sum = 0.0;
        long long cnt = 0;
        for (long long k = 0; k < pgl_rw_pieces(len); ++k) {
            const long long a = t0 + k * PGL_RW_PIECE, b = (a + PGL_RW_PIECE < t0 + len) ? a + PGL_RW_PIECE : t0 + len;
            double piece = 0.0;
            for (long long t = a; t < b; ++t) {
                piece += lam_t[t];
                cnt += spikes[t];
            }
            sum += piece;
        }
        Lam[w] = dt * sum;
        obs[w] = (double)cnt;
    }
}
