/* Host build of the product's Newton-CG row state machine (theano_pyglm_amd/csrc/pglm_ncg.h) for the CPU tests: one row,
 * driven by reverse communication the way the k_ncg_* row kernels drive it -- the test supplies f, g and H v from numpy
 * and compares the iterates with scipy.optimize.minimize(method='Newton-CG').
 *   sc:  PGL_NCG_NSCAL doubles (PglNcg), ls: PGL_LS_NDOUBLES doubles (PglLs),
 *   vec: (8, P) doubles: x, g, xsupi, ri, psupi, xb, gb (best trial of the running search), xt (the trial point).
 * Every call returns the row's phase: 0 = supply H psupi (ncg_feed_hv), 1 = supply f, g at xt (ncg_feed_fg), 2 = done. */
#include "../../theano_pyglm_amd/csrc/pglm_ncg.h"

enum { VX, VG, VXS, VR, VP, VXB, VGB, VXT };

static int cg_end(PglNcg* s, PglLs* ls, double* v, int P)
{
    double slope = 0.0, pn = 0.0;
    for (int c = 0; c < P; ++c) {
        slope += v[VG * P + c] * v[VXS * P + c];
        pn += pgl_ls_abs(v[VXS * P + c]);
    }
    const int ph = pgl_ncg_cg_end(s, ls, slope, pn);
    if (ph == PGL_NCG_SEARCH)
        for (int c = 0; c < P; ++c) v[VXT * P + c] = v[VX * P + c] + s->alpha * v[VXS * P + c];
    return ph;
}

static int outer_begin(PglNcg* s, PglLs* ls, double* v, int P, int maxiter)
{
    double mag = 0.0, gg = 0.0;
    for (int c = 0; c < P; ++c) {
        const double g = v[VG * P + c];
        mag += pgl_ls_abs(g);
        gg += g * g;
        v[VXS * P + c] = 0.0;
        v[VR * P + c] = g;
        v[VP * P + c] = -g;
    }
    const int ph = pgl_ncg_outer_begin(s, mag, gg, maxiter);
    if (ph == PGL_NCG_SEARCH) return cg_end(s, ls, v, P);
    return ph;
}

/* x in vec[0]; f, g at x (NaN rules: here) */
int ncg_start(double* sc, double* lsd, double* v, int P, int maxiter, double f, const double* g)
{
    PglNcg* s = (PglNcg*)sc;
    int bad = 0;
    for (int c = 0; c < P; ++c) bad |= g[c] != g[c];
    for (int c = 0; c < P; ++c) v[VG * P + c] = bad ? 0.0 : g[c];
    pgl_ncg_init(s, f != f ? 1e16 : f);
    return outer_begin(s, (PglLs*)lsd, v, P, maxiter);
}

/* hv = H psupi of the objective */
int ncg_feed_hv(double* sc, double* lsd, double* v, int P, int maxiter, const double* hv)
{
    PglNcg* s = (PglNcg*)sc;
    PglLs* ls = (PglLs*)lsd;
    int bad = 0;
    double curv = 0.0;
    for (int c = 0; c < P; ++c) bad |= hv[c] != hv[c];
    for (int c = 0; c < P; ++c) curv += v[VP * P + c] * (bad ? 0.0 : hv[c]);
    const int d = pgl_ncg_cg_curv(s, curv);
    if (d == PGL_NCG_CURV_FAIL) {
        pgl_ncg_finish(s, PGL_NCG_CGFAIL);
        return PGL_NCG_DONE;
    }
    if (d == PGL_NCG_CURV_STEEPEST)
        for (int c = 0; c < P; ++c) v[VXS * P + c] = s->alphai * -v[VG * P + c];
    if (d != PGL_NCG_CURV_UPDATE) return cg_end(s, ls, v, P);
    double dri1 = 0.0, rn = 0.0, betai;
    for (int c = 0; c < P; ++c) {
        const double r = pgl_ncg_cg_elem_xr(s->alphai, v[VP * P + c], bad ? 0.0 : hv[c], &v[VXS * P + c], &v[VR * P + c]);
        dri1 += r * r;
        rn += pgl_ls_abs(r);
    }
    const int go = pgl_ncg_cg_next(s, dri1, rn, P, &betai);
    if (go < 0) return PGL_NCG_DONE;
    for (int c = 0; c < P; ++c) v[VP * P + c] = pgl_ncg_cg_elem_p(betai, v[VR * P + c], v[VP * P + c]);
    if (go == 0) return cg_end(s, ls, v, P);
    return PGL_NCG_CG;
}

/* f, g at xt */
int ncg_feed_fg(double* sc, double* lsd, double* v, int P, int maxiter, double f, const double* g)
{
    PglNcg* s = (PglNcg*)sc;
    PglLs* ls = (PglLs*)lsd;
    int bad = 0;
    double dphi = 0.0;
    for (int c = 0; c < P; ++c) bad |= g[c] != g[c];
    for (int c = 0; c < P; ++c) dphi += (bad ? 0.0 : g[c]) * v[VXS * P + c];
    const double fv = f != f ? 1e16 : f;
    const int d = pgl_ncg_search_step(s, ls, fv, dphi);
    if (d == PGL_NCG_LS_FAIL) return PGL_NCG_DONE;
    if (d == PGL_NCG_LS_EVALUATE) {
        if (s->moved != 0.0)
            for (int c = 0; c < P; ++c) {
                v[VXB * P + c] = v[VXT * P + c];
                v[VGB * P + c] = bad ? 0.0 : g[c];
            }
        for (int c = 0; c < P; ++c) v[VXT * P + c] = v[VX * P + c] + s->alpha * v[VXS * P + c];
        return PGL_NCG_SEARCH;
    }
    double un = 0.0;
    for (int c = 0; c < P; ++c) {
        un += pgl_ls_abs(s->alpha_acc * v[VXS * P + c]);
        v[VX * P + c] = d == PGL_NCG_LS_TAKE_TRIAL ? v[VXT * P + c] : v[VXB * P + c];
        v[VG * P + c] = d == PGL_NCG_LS_TAKE_TRIAL ? (bad ? 0.0 : g[c]) : v[VGB * P + c];
    }
    if (pgl_ncg_accept(s, d == PGL_NCG_LS_TAKE_TRIAL ? fv : s->fb, un, P) == PGL_NCG_DONE) return PGL_NCG_DONE;
    return outer_begin(s, ls, v, P, maxiter);
}

int ncg_nscal(void) { return (int)(sizeof(PglNcg) / sizeof(double)); }
int ncg_nls(void) { return (int)(sizeof(PglLs) / sizeof(double)); }
