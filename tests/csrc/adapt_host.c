/* Host build of the warm-up mass adaptation (theano_pyglm_amd/csrc/pglm_adapt.h) for the CPU tests and as the mirror of the
 * device chains under mass='adapt':
 *   adapt_hmc_step   pgl_mass_adapt_dev with host pointers, on the state block of hmc_host.c (called between the last leap
 *                    of a transition and the next begin);
 *   adapt_nuts_step  pgl_nuts_adapt_step_dev with host pointers: nuts_host.c's nuts_step for the diagonal chain with the
 *                    adaptation at the row's transition boundary (nuts_host.c is included for nuts_init and the helpers).
 * The adaptation state has the device's layout: mean (R, P), M2 (R, P), count (R), window index (R).  sched: ints
 * [n_win, start of window 0, end of window 0, ...].  Sums run in index order. */
#include "nuts_host.c"
#include "../../theano_pyglm_amd/csrc/pglm_adapt.h"

long long adapt_state_doubles(int R, int P) { return (long long)R * P * PGL_ADAPT_NVEC + (long long)R * PGL_ADAPT_NSCAL; }
unsigned long long adapt_chain_seed(unsigned long long seed, unsigned long long c) { return pgl_chain_seed(seed, c); }
double adapt_minv(double m2, double n) { return pgl_adapt_minv(m2, n); }
void adapt_welford(double q, double n, double* mean, double* m2) { pgl_adapt_welford(q, n, mean, m2); }
/* the restart rules on one row's scalar fields (PglHmc / PglNuts as doubles) */
void adapt_restart_hmc(double* f) { pgl_adapt_restart_hmc((PglHmc*)f); }
void adapt_restart_nuts(double* f) { pgl_adapt_restart_nuts((PglNuts*)f); }
void adapt_fresh_hmc(double* f, double step) { pgl_hmc_init((PglHmc*)f, 0.0, step, 0, 0); }
void adapt_fresh_nuts(double* f, double step) { pgl_nuts_init((PglNuts*)f, 1, 0.0, step, 0, 0, 1); }

/* one row's rules: the scalars, then the elements.  Returns the action bits. */
static int adapt_point(double* ad, int R, int P, int r, const int* sched, int t, const double* q, double* minv_row,
                       double* restart_t)
{
    double *mean = ad + (long)r * P, *m2 = ad + (long)R * P + (long)r * P, *count = ad + 2L * R * P, *widx = count + R;
    PglAdapt a = {count[r], widx[r]};
    double n = 0.0;
    if (restart_t) *restart_t = pgl_adapt_restart_t(&a, sched);
    const int act = pgl_adapt_row(&a, sched, t, &n);
    count[r] = a.count; widx[r] = a.widx;
    if (!act) return 0;
    for (int c = 0; c < P; ++c) {
        pgl_adapt_welford(q[c], n, mean + c, m2 + c);
        if (act & PGL_ADAPT_SWITCH) {
            minv_row[c] = pgl_adapt_minv(m2[c], n);
            mean[c] = 0.0; m2[c] = 0.0;
        }
    }
    return act;
}

void adapt_hmc_step(double* st, int R, int P, double* ad, const int* sched, double* minv)
{
    const long RP = (long)R * P;
    double *Q = st, *sc = st + PGL_HMC_NVEC * RP;
    for (int r = 0; r < R; ++r) {
        const int t = (int)sc[5L * R + r] - 1;
        const int act = adapt_point(ad, R, P, r, sched, t, Q + (long)r * P, minv + (long)r * P, 0);
        if (act & PGL_ADAPT_SWITCH) {
            PglHmc s;
            double* f = (double*)&s;
            for (int k = 0; k < PGL_HMC_NSCAL; ++k) f[k] = sc[(long)k * R + r];
            pgl_adapt_restart_hmc(&s);
            for (int k = 0; k < PGL_HMC_NSCAL; ++k) sc[(long)k * R + r] = f[k];
        }
    }
}

/* nuts_step of nuts_host.c, diagonal mass minv (M, P) (read, and rewritten at a row's window ends), no margins */
void adapt_nuts_step(double* st, int M, int P, int D, double* ll, double* grad, int kind, int N, int B, int Dstim,
                     const double* prm, double* minv, double* ad, const int* sched, double delta, int n_warmup, int thin,
                     int n_keep, double* Xt, double* samples, double* stats, int* acts, double* tmp)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double* sc = st + (long)(PGL_NUTS_NVEC + 2 * D) * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        double* mr = minv + o;
        PglNuts s;
        load(sc, M, r, &s);
        acts[r] = 0;
        if (s.done != 0.0) continue;
        double *qw = VEC(PGL_NUTS_QW), *rw = VEC(PGL_NUTS_RW), *hb = VEC(PGL_NUTS_HB), *rhos = VEC(PGL_NUTS_RHOS);
        double* g = grad + o;
        const double U1 = target(&q, P, qw, g, ll[r]);
        apply(0, mr, P, 1, g, hb);
        const int i = (int)s.i, size = 1 << ((int)s.depth - 1), right = s.v > 0.0;
        const int nb = pgl_nuts_trailing_ones(i), pc = pgl_nuts_popcount(i);
        double ks = 0.0;
        for (int c = 0; c < P; ++c) {
            rw[c] = pgl_nuts_half_kick(rw[c], s.ve, hb[c]);
            ks += rw[c] * rw[c];
            if (!(i & 1)) {
                VEC(PGL_NUTS_NVEC + pc)[c] = rw[c];
                VEC(PGL_NUTS_NVEC + D + pc)[c] = rhos[c];
            }
            rhos[c] += rw[c];
        }
        double dots[2 * PGL_NUTS_MAX_DEPTH], dot_l = 0.0, dot_r = 0.0;
        for (int k = 1; k <= nb; ++k) {
            const double *cr = VEC(PGL_NUTS_NVEC + pc - k), *crho = VEC(PGL_NUTS_NVEC + D + pc - k);
            double a = 0.0, b = 0.0;
            for (int c = 0; c < P; ++c) {
                const double rb = rhos[c] - crho[c];
                a += rb * cr[c]; b += rb * rw[c];
            }
            dots[2 * (k - 1)] = a; dots[2 * (k - 1) + 1] = b;
        }
        if (i == size - 1) {
            const double *el = right ? VEC(PGL_NUTS_RL) : rw, *er = right ? rw : VEC(PGL_NUTS_RR);
            for (int c = 0; c < P; ++c) {
                const double rt = VEC(PGL_NUTS_RHO)[c] + rhos[c];
                dot_l += rt * el[c]; dot_r += rt * er[c];
            }
        }
        int slot = -1;
        const double* cnt = ad + 2L * M * P;
        PglAdapt a0 = {cnt[r], cnt[M + r]};
        const int act = pgl_nuts_leaf_from(&s, P, D, U1, ks, dots, dot_l, dot_r, delta, n_warmup, thin, n_keep, &slot, 0,
                                           pgl_adapt_restart_t(&a0, sched));
        acts[r] = act;
        for (int c = 0; c < P; ++c) {
            if (act & PGL_NUTS_TAKE_LEAF) {
                VEC(PGL_NUTS_QS)[c] = qw[c]; VEC(PGL_NUTS_GS)[c] = g[c]; VEC(PGL_NUTS_HS)[c] = hb[c];
            }
            if (act & PGL_NUTS_MERGE) {
                VEC(right ? PGL_NUTS_QR : PGL_NUTS_QL)[c] = qw[c];
                VEC(right ? PGL_NUTS_RR : PGL_NUTS_RL)[c] = rw[c];
                VEC(right ? PGL_NUTS_HR : PGL_NUTS_HL)[c] = hb[c];
                VEC(PGL_NUTS_RHO)[c] += rhos[c];
            }
            if (act & PGL_NUTS_TAKE_SUB) {
                VEC(PGL_NUTS_QC)[c] = VEC(PGL_NUTS_QS)[c]; VEC(PGL_NUTS_GC)[c] = VEC(PGL_NUTS_GS)[c];
                VEC(PGL_NUTS_HC)[c] = VEC(PGL_NUTS_HS)[c];
            }
            if ((act & PGL_NUTS_END) && slot >= 0 && samples) samples[((long)slot * M + r) * P + c] = VEC(PGL_NUTS_QC)[c];
            if (act & PGL_NUTS_CONT) rw[c] = pgl_nuts_half_kick(rw[c], s.ve, hb[c]);
        }
        if ((act & PGL_NUTS_END) && slot >= 0 && stats) {
            stats[((long)slot * 2 + 0) * M + r] = s.last_depth;
            stats[((long)slot * 2 + 1) * M + r] = s.last_nleaf;
        }
        if (act & PGL_NUTS_END) {                                              /* the transition boundary */
            const int aa = adapt_point(ad, M, P, r, sched, (int)s.t - 1, VEC(PGL_NUTS_QC), mr, 0);
            if (aa & PGL_ADAPT_SWITCH) {
                pgl_adapt_restart_nuts(&s);
                apply(0, mr, P, 1, VEC(PGL_NUTS_GC), VEC(PGL_NUTS_HC));
            }
        }
        if (act & PGL_NUTS_DONE) {
            for (int c = 0; c < P; ++c) {
                Xt[o + c] = qw[c] = VEC(PGL_NUTS_QC)[c];
                rw[c] = 0.0;
            }
        } else {
            if (act & PGL_NUTS_END) draw(st, MP, o, P, &s);
            if (act & PGL_NUTS_NEWSUB) from_edge(st, MP, o, P, &s);
            drift(st, MP, o, P, 0, mr, &s, Xt + o, tmp);
        }
        store(sc, M, r, &s);
    }
}
