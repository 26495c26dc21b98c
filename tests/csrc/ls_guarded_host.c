/* Host test of the guarded line-search step (pgl_ls_guarded_step, theano_pyglm_amd/csrc/pglm_linesearch.h) and of its two
 * wrappers (pgl_ncg_search_step, pgl_newton_search_step): scripted searches on two 1-D functions, each run under both
 * constant sets (0: the Newton-CG / dense Newton rows', 1: the BFGS rows').  On every call three copies of the search
 * advance: the direct call fed the exact value at the best step (what the Newton-CG and BFGS rows keep), the Newton-CG
 * wrapper, and the dense Newton wrapper next to a direct call fed the same fb as that wrapper reads (ls->fx).  They must
 * agree on the decision, on the step length and the value of the point taken, and on all PGL_LS_NDOUBLES doubles of the
 * line-search state (the wrappers only under set 0: the constants are theirs).
 * lsg_run(set, reached): 0, or 100 * (case + 1) + the check that failed; reached[k] counts the searches that ended in
 * outcome k of enum reach.  With -DLSG_MAIN: a stand-alone program (the sanitizer run builds this). */
#include <math.h>
#include <string.h>

#include "../../theano_pyglm_amd/csrc/pglm_ncg.h"
#include "../../theano_pyglm_amd/csrc/pglm_newton.h"

enum reach { R_CONVERGED, R_WARN_TRIAL, R_WARN_BEST, R_WARN_FAIL, R_CUT_MOVED, R_NONFINITE_F, R_NONFINITE_DPHI, R_COUNT };

/* the BFGS rows' constants (pglm_bfgs.hip.h: scipy's line_search_wolfe1) */
static const double KSET[2][5] = {{PGL_NCG_C1, PGL_NCG_C2, PGL_NCG_LS_XTOL, PGL_NCG_STPMIN, PGL_NCG_STPMAX},
                                  {1e-4, 0.9, 1e-14, 1e-100, 1e100}};

/* phi(a) and phi'(a) along the search direction */
enum fn { QUARTIC, KINK, RISE };
static void phi(int fn, double kink, double a, double* f, double* g)
{
    if (fn == QUARTIC) {                                   /* (a - 2)^4: phi(0) = 16, phi'(0) = -32 */
        const double d = a - 2.0;
        *f = d * d * d * d;
        *g = 4.0 * d * d * d;
    } else if (fn == KINK) {                               /* slope -1 down to the kink, slope +10 behind it */
        *f = a < kink ? kink - a : 10.0 * (a - kink);
        *g = a < kink ? -1.0 : 10.0;
    } else {                                               /* a kink AT the start: |a|, searched with the slope -1 */
        *f = a;
        *g = 1.0;
    }
}

enum script { NONE, F_INF, DPHI_NAN, F_NOISE };             /* f = +inf; dphi = NaN; f + 0.25: the value did not repeat */
typedef struct {
    int fn;
    double kink, stp0;
    int nfev0;        /* trials the search claims to have behind it at its start (reaches the max_trials cut-off) */
    int script;       /* what the scripted call's evaluation is replaced by (enum script) */
    int at[2];        /* the scripted call (from 1) under set 0, set 1 */
    int expect[2];    /* enum reach under set 0, set 1 */
} lsg_case;

#define LAST_KINK 84   /* the trial on which the search of the case before it ends, under either set */
static const lsg_case CASES[] = {
    {QUARTIC, 0.0, 0.05, 0, NONE, {0, 0}, {R_CONVERGED, R_CONVERGED}},         /* several trials, then strong Wolfe */
    {QUARTIC, 0.0, 1.0, 0, NONE, {0, 0}, {R_CONVERGED, R_CONVERGED}},          /* the first trial */
    {KINK, 60.0, 1.0, 0, NONE, {0, 0}, {R_WARN_TRIAL, R_WARN_TRIAL}},          /* set 0: stopped by stpmax = 50 on the way down */
    {KINK, 1.0, 0.5, 0, NONE, {0, 0}, {R_WARN_TRIAL, R_WARN_TRIAL}},           /* the interval closes on the kink */
    {KINK, 1.0, 3.0, 0, NONE, {0, 0}, {R_WARN_TRIAL, R_WARN_TRIAL}},           /* ... from behind it */
    {KINK, 1.0, 0.5, 0, F_NOISE, {LAST_KINK, LAST_KINK}, {R_WARN_BEST, R_WARN_BEST}},  /* ... and its last trial, at the best step
                                                                                  again, comes out higher than before */
    {RISE, 0.0, 1.0, 0, NONE, {0, 0}, {R_WARN_FAIL, R_WARN_FAIL}},             /* no step decreases */
    {QUARTIC, 0.0, 0.05, 99, NONE, {0, 0}, {R_CUT_MOVED, R_CUT_MOVED}},        /* trial 100 becomes the best step: cut off */
    {QUARTIC, 0.0, 0.05, 0, F_INF, {2, 2}, {R_NONFINITE_F, R_NONFINITE_F}},    /* the best step saved by call 1 is taken */
    {QUARTIC, 0.0, 0.05, 0, F_INF, {1, 1}, {R_NONFINITE_F, R_NONFINITE_F}},    /* nothing saved: fail */
    {QUARTIC, 0.0, 0.05, 0, DPHI_NAN, {2, 2}, {R_NONFINITE_DPHI, R_NONFINITE_DPHI}},
    {KINK, 1.0, 0.5, 0, DPHI_NAN, {3, 3}, {R_NONFINITE_DPHI, R_NONFINITE_DPHI}},
};
#define NCASES ((int)(sizeof(CASES) / sizeof(CASES[0])))

int lsg_ncases(void) { return NCASES; }
int lsg_nreach(void) { return R_COUNT; }
int lsg_expected(int c, int set) { return CASES[c].expect[set]; }

static int same(const void* a, const void* b, size_t n) { return memcmp(a, b, n) == 0; }

/* one scripted search; *how: the enum reach it ended in, *dec: its last decision, *calls: its trials.  Returns 0 or the check that failed. */
static int run_case(const lsg_case* c, int set, int* how, int* dec, int* calls)
{
    const double* k = KSET[set];
    double f0, g0;
    phi(c->fn, c->kink, 0.0, &f0, &g0);
    if (c->fn == RISE) g0 = -1.0;
    PglLs ld, ln, lc, lw;                                   /* direct (exact fb), direct (fb = fx), Newton-CG, dense Newton */
    PglNcg sc;
    PglNewton sw;
    pgl_ls_start(&ld, c->stp0, f0, g0, k[0], k[3], k[4]);
    ld.nfev = (double)c->nfev0;
    ln = lc = lw = ld;
    pgl_ncg_init(&sc, f0);
    sc.phase = (double)PGL_NCG_SEARCH;
    sc.alpha = c->stp0;
    pgl_newton_init(&sw, f0, 1.0, 0.0, 1000);
    sw.phase = (double)PGL_NEWTON_SEARCH;
    sw.alpha = c->stp0;
    double fb = f0;                                        /* the exact value at the best step, as the rows keep it */
    for (int call = 1; call <= 400; ++call) {
        double f, g;
        phi(c->fn, c->kink, ld.stp, &f, &g);
        const int scr = call == c->at[set] ? c->script : NONE;
        if (scr == F_INF) f = INFINITY;
        if (scr == DPHI_NAN) g = NAN;
        if (scr == F_NOISE) f += 0.25;
        const double stp = ld.stp, stx = ld.stx;
        double ad = -1.0, fd = -1.0, an = -1.0, fn_ = -1.0, fw = -1.0;
        const int d = pgl_ls_guarded_step(&ld, f, g, fb, k[0], k[1], k[2], k[3], k[4], PGL_NCG_MAX_TRIALS, &ad, &fd);
        const int dn = pgl_ls_guarded_step(&ln, f, g, ln.fx, k[0], k[1], k[2], k[3], k[4], PGL_NCG_MAX_TRIALS, &an, &fn_);
        if (dn != d || !same(&ln, &ld, sizeof(ld))) return 1;
        if (d == PGL_LS_TAKE_TRIAL && !(ad == stp && fd == f && an == stp && fn_ == f)) return 2;
        if (d == PGL_LS_TAKE_BEST && !(ad == stx && fd == fb && an == stx)) return 3;
        if ((d == PGL_LS_EVALUATE || d == PGL_LS_FAIL) && !(ad == -1.0 && fd == -1.0)) return 4;
        if (ld.moved != 0.0 && d != PGL_LS_EVALUATE) return 5;
        if (set == 0) {
            const double nf_c = sc.nfev, nf_w = sw.nfev;
            const int dc = pgl_ncg_search_step(&sc, &lc, f, g);
            const int dw = pgl_newton_search_step(&sw, &lw, f, g, &fw);
            if (dc != d || dw != d) return 6;
            if (!same(&lc, &ld, sizeof(ld)) || !same(&lw, &ld, sizeof(ld))) return 7;
            if (sc.nfev != nf_c + 1.0 || sw.nfev != nf_w + 1.0) return 8;
            if (d == PGL_LS_EVALUATE && !(sc.alpha == ld.stp && sw.alpha == ld.stp && sc.moved == ld.moved)) return 9;
            if ((d == PGL_LS_TAKE_TRIAL || d == PGL_LS_TAKE_BEST) && !(sc.alpha_acc == ad && fw == fn_)) return 10;
            if (d == PGL_LS_TAKE_BEST && sc.fb != fd) return 11;
            if (d == PGL_LS_FAIL && !(sc.status == (double)PGL_NCG_PRLOSS && sc.phase == (double)PGL_NCG_DONE &&
                                      sw.status == (double)PGL_NEWTON_PRLOSS && sw.phase == (double)PGL_NEWTON_DONE))
                return 12;
            if (d != PGL_LS_FAIL && !(sc.status == (double)PGL_NCG_RUNNING && sw.status == (double)PGL_NEWTON_RUNNING)) return 13;
        }
        if (d == PGL_LS_EVALUATE) {
            if (ld.moved != 0.0) fb = f;
            if (set == 0 && sc.fb != fb) return 14;
            continue;
        }
        /* how the search ended (a trial that became the best step in a call that did not go on: the cut-off) */
        *dec = d;
        *calls = call;
        if (scr == F_INF || scr == DPHI_NAN) *how = scr == F_INF ? R_NONFINITE_F : R_NONFINITE_DPHI;
        else if (d == PGL_LS_TAKE_TRIAL && fabs(g) <= k[1] * -ld.ginit && f <= ld.finit + stp * ld.gtest) *how = R_CONVERGED;
        else if (ld.stx == stp && stx != stp) *how = ld.nfev >= (double)PGL_NCG_MAX_TRIALS ? R_CUT_MOVED : -2;
        else *how = d == PGL_LS_TAKE_TRIAL ? R_WARN_TRIAL : d == PGL_LS_TAKE_BEST ? R_WARN_BEST : R_WARN_FAIL;
        return 0;
    }
    return 15;                                             /* the search never ended */
}

int lsg_run(int set, int* reached)
{
    for (int i = 0; i < R_COUNT; ++i) reached[i] = 0;
    for (int c = 0; c < NCASES; ++c) {
        int how = -1, dec = -1, calls = 0;
        const int bad = run_case(&CASES[c], set, &how, &dec, &calls);
        if (bad) return 100 * (c + 1) + bad;
        if (how != CASES[c].expect[set]) return 100 * (c + 1) + 50 + how;
        reached[how] += 1;
    }
    return 0;
}

#ifdef LSG_MAIN
#include <stdio.h>
int main(void)
{
    int bad = 0;
    for (int set = 0; set < 2; ++set) {
        int reached[R_COUNT];
        const int rc = lsg_run(set, reached);
        printf("set %d: rc %d, reached", set, rc);
        for (int i = 0; i < R_COUNT; ++i) {
            printf(" %d", reached[i]);
            bad |= reached[i] == 0;
        }
        printf("\n");
        bad |= rc;
    }
    return bad ? 1 : 0;
}
#endif
