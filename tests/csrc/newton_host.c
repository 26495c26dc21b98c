/* Host build of the product's dense Newton row state machine (theano_pyglm_amd/csrc/pglm_newton.h) for the tests: one row,
 * driven by reverse communication the way the k_newton_* row kernels drive it -- the caller (tests/newton_mirror.py)
 * supplies f, g (priors applied), the factor's flag and the solve's output from numpy.
 *   sc:  PGL_NEWTON_NSCAL doubles (PglNewton), ls: PGL_LS_NDOUBLES doubles (PglLs),
 *   vec: (6, P) doubles: x, g, p, xb, gb (best trial of the running search), xt (the trial point).
 * Every call returns the row's phase: 0 = supply factor and solve at x with the row's shift (newton_feed_direction),
 * 1 = supply f, g at xt (newton_feed_fg), 2 = done, 3 = the shift was raised: factor and solve again, same Hessian. */
#include "../../theano_pyglm_amd/csrc/pglm_newton.h"

enum { VX, VG, VP, VXB, VGB, VXT };

static double absmax(const double* a, int P)
{
    double m = 0.0;
    for (int c = 0; c < P; ++c) {
        const double v = pgl_ls_abs(a[c]);
        if (v > m) m = v;
    }
    return m;
}

/* x in vec[0]; f, g at x (NaN rules: here) */
int newton_start(double* sc, double* lsd, double* v, int P, int maxiter, double gtol, double f, const double* g)
{
    PglNewton* s = (PglNewton*)sc;
    int bad = 0;
    for (int c = 0; c < P; ++c) bad |= g[c] != g[c];
    for (int c = 0; c < P; ++c) v[VG * P + c] = bad ? 0.0 : g[c];
    f = f != f ? 1e16 : f;
    pgl_ls_start((PglLs*)lsd, 1.0, f, -1.0, PGL_NEWTON_C1, PGL_NEWTON_STPMIN, PGL_NEWTON_STPMAX);
    return pgl_newton_init(s, f, absmax(v + VG * P, P), gtol, maxiter);
}

/* info: the factor's flag of A + shift diag A; sol = -(A + shift diag A)^-1 g (anything where info != 0) */
int newton_feed_direction(double* sc, double* lsd, double* v, int P, int info, const double* sol)
{
    PglNewton* s = (PglNewton*)sc;
    PglLs* ls = (PglLs*)lsd;
    double slope = 0.0, gg = 0.0;
    for (int c = 0; c < P; ++c) {
        const double g = v[VG * P + c];
        slope += g * (info ? 0.0 : sol[c]);
        gg += g * g;
    }
    const int d = pgl_newton_direction(s, ls, info != 0, slope, gg);
    if (d == PGL_NEWTON_DIR_NEWTON)
        for (int c = 0; c < P; ++c) v[VP * P + c] = sol[c];
    else if (d == PGL_NEWTON_DIR_STEEPEST)
        for (int c = 0; c < P; ++c) v[VP * P + c] = -v[VG * P + c];
    if (s->phase == (double)PGL_NEWTON_SEARCH)
        for (int c = 0; c < P; ++c) v[VXT * P + c] = v[VX * P + c] + s->alpha * v[VP * P + c];
    return (int)s->phase;
}

/* f, g at xt */
int newton_feed_fg(double* sc, double* lsd, double* v, int P, int maxiter, double gtol, double f, const double* g)
{
    PglNewton* s = (PglNewton*)sc;
    PglLs* ls = (PglLs*)lsd;
    int bad = 0;
    double dphi = 0.0, facc = 0.0;
    for (int c = 0; c < P; ++c) bad |= g[c] != g[c];
    for (int c = 0; c < P; ++c) dphi += (bad ? 0.0 : g[c]) * v[VP * P + c];
    const double fv = f != f ? 1e16 : f;
    const int d = pgl_newton_search_step(s, ls, fv, dphi, &facc);
    if (d == PGL_NEWTON_LS_FAIL) return PGL_NEWTON_DONE;
    if (d == PGL_NEWTON_LS_EVALUATE) {
        if (ls->moved != 0.0)
            for (int c = 0; c < P; ++c) {
                v[VXB * P + c] = v[VXT * P + c];
                v[VGB * P + c] = bad ? 0.0 : g[c];
            }
        for (int c = 0; c < P; ++c) v[VXT * P + c] = v[VX * P + c] + s->alpha * v[VP * P + c];
        return PGL_NEWTON_SEARCH;
    }
    for (int c = 0; c < P; ++c) {
        v[VX * P + c] = d == PGL_NEWTON_LS_TAKE_TRIAL ? v[VXT * P + c] : v[VXB * P + c];
        v[VG * P + c] = d == PGL_NEWTON_LS_TAKE_TRIAL ? (bad ? 0.0 : g[c]) : v[VGB * P + c];
    }
    return pgl_newton_accept(s, facc, absmax(v + VG * P, P), gtol, maxiter);
}

int newton_nscal(void) { return (int)(sizeof(PglNewton) / sizeof(double)); }
int newton_nls(void) { return (int)(sizeof(PglLs) / sizeof(double)); }
double newton_next_shift(double shift) { return pgl_newton_next_shift(shift); }
