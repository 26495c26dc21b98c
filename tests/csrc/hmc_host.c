/* Host build of the product's HMC row state machine (theano_pyglm_amd/csrc/pglm_hmc.h) for the CPU tests and as the
 * mirror of the device chain: M rows, driven by reverse communication the way the k_hmc_* row kernels drive it -- the
 * caller supplies ll and its gradient at the points the machine asks for.  The three calls are pgl_hmc_init_dev /
 * _begin_dev / _leap_dev with host pointers; the state block has the device's layout:
 *   st: (4, M, P) q, p, q0, g, then (PGL_HMC_NSCAL, M) the fields of PglHmc.
 * prior_kind < 0: no prior (ll is the whole log density, rows need not be theta rows); else rows are
 * [bias, w_stim (Dstim), w_ir (N, B)] under the priors of pglm_hmc.h.  Sums run in index order. */
#include "../../theano_pyglm_amd/csrc/pglm_hmc.h"

typedef struct {
    int kind, N, B, Dstim;
    double mu_b, sg_b, stim_sigma, mu, sigma, lam;
} Prior;

static void load(const double* sc, int M, int r, PglHmc* s)
{
    double* f = (double*)s;
    for (int k = 0; k < PGL_HMC_NSCAL; ++k) f[k] = sc[(long)k * M + r];
}
static void store(double* sc, int M, int r, const PglHmc* s)
{
    const double* f = (const double*)s;
    for (int k = 0; k < PGL_HMC_NSCAL; ++k) sc[(long)k * M + r] = f[k];
}

/* g: grad ll -> grad U in place; returns U */
static double target(const Prior* q, int P, const double* x, double* g, double ll)
{
    double lp = 0.0;
    if (q->kind < 0) {
        for (int c = 0; c < P; ++c) g[c] = pgl_hmc_grad_elem(g[c], 0.0);
        return pgl_hmc_energy(ll, 0.0);
    }
    double d;
    lp += pgl_hmc_prior_bias(x[0], q->mu_b, q->sg_b, &d);
    g[0] = pgl_hmc_grad_elem(g[0], d);
    for (int c = 1; c < 1 + q->Dstim; ++c) {
        lp += pgl_hmc_prior_stim(x[c], q->stim_sigma, &d);
        g[c] = pgl_hmc_grad_elem(g[c], d);
    }
    const int o = 1 + q->Dstim;
    for (int n = 0; n < q->N; ++n)
        lp += pgl_hmc_prior_group(q->kind, x + o + n * q->B, q->B, q->mu, q->sigma, q->lam, g + o + n * q->B);
    return pgl_hmc_energy(ll, lp);
}

static Prior prior(int kind, int N, int B, int Dstim, const double* prm)
{
    Prior q = {kind, N, B, Dstim, prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]};
    return q;
}

/* prm: mu_b, sg_b, stim_sigma, mu, sigma, lam */
void hmc_init(double* st, int M, int P, int n_lo, double* ll, double* grad, int kind, int N, int B, int Dstim,
              const double* prm, double step0, unsigned long long seed)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double *Q = st, *G = st + 3 * MP, *sc = st + PGL_HMC_NVEC * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        const double U = target(&q, P, Q + o, grad + o, ll[r]);
        for (int c = 0; c < P; ++c) G[o + c] = grad[o + c];
        PglHmc s;
        pgl_hmc_init(&s, U, step0, n_lo + r, seed);
        store(sc, M, r, &s);
        ll[r] = U;
    }
}

/* p_in (M, P) or NULL: momenta to use instead of the stateless draw (the CPU tests feed a trajectory its own reversed
 * momentum this way) */
void hmc_begin(double* st, int M, int P, const double* minv, double* Xt, const double* p_in)
{
    const long MP = (long)M * P;
    double *Q = st, *Pm = st + MP, *Q0 = st + 2 * MP, *G = st + 3 * MP, *sc = st + PGL_HMC_NVEC * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        PglHmc s;
        load(sc, M, r, &s);
        const pgl_hmc_u64 key = pgl_hmc_row_key(&s);
        double ks = 0.0;
        for (int c = 0; c < P; ++c) {
            const double mi = minv ? minv[o + c] : 1.0;
            double p = p_in ? p_in[o + c] : pgl_hmc_momentum(pgl_hmc_normal(key, (pgl_hmc_u64)c), mi);
            ks += pgl_hmc_kinetic_elem(p, mi);
            p = pgl_hmc_kick(p, 0.5, s.step, G[o + c]);
            Q0[o + c] = Q[o + c];
            Pm[o + c] = p;
            Q[o + c] = pgl_hmc_drift(Q[o + c], s.step, mi, p);
            Xt[o + c] = Q[o + c];
        }
        pgl_hmc_begin(&s, ks);
        store(sc, M, r, &s);
    }
}

/* margin_out (M) or NULL: |log u - (H0 - H1)| of each row's decision (last != 0) */
void hmc_leap(double* st, int M, int P, const double* minv, double* ll, double* grad, int kind, int N, int B, int Dstim,
              const double* prm, int last, int n_warmup, double* Xt, double* sample_out, double* margin_out)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double *Q = st, *Pm = st + MP, *Q0 = st + 2 * MP, *G = st + 3 * MP, *sc = st + PGL_HMC_NVEC * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        PglHmc s;
        load(sc, M, r, &s);
        const double U1 = target(&q, P, Q + o, grad + o, ll[r]);
        ll[r] = U1;
        if (!last) {
            for (int c = 0; c < P; ++c) {
                const double mi = minv ? minv[o + c] : 1.0;
                Pm[o + c] = pgl_hmc_kick(Pm[o + c], 1.0, s.step, grad[o + c]);
                Q[o + c] = pgl_hmc_drift(Q[o + c], s.step, mi, Pm[o + c]);
                Xt[o + c] = Q[o + c];
            }
            continue;
        }
        double ks = 0.0;
        for (int c = 0; c < P; ++c) {
            const double mi = minv ? minv[o + c] : 1.0;
            Pm[o + c] = pgl_hmc_kick(Pm[o + c], 0.5, s.step, grad[o + c]);
            ks += pgl_hmc_kinetic_elem(Pm[o + c], mi);
        }
        const double u = pgl_hmc_accept_uniform(pgl_hmc_row_key(&s));
        if (margin_out) margin_out[r] = pgl_ls_abs(log(u) - (s.H0 - (U1 + 0.5 * ks)));
        const int acc = pgl_hmc_decide(&s, U1, ks, u, n_warmup);
        for (int c = 0; c < P; ++c) {
            if (acc) G[o + c] = grad[o + c];
            else Q[o + c] = Q0[o + c];
            if (sample_out) sample_out[o + c] = Q[o + c];
        }
        store(sc, M, r, &s);
    }
}

double hmc_normal(unsigned long long seed, unsigned long long n, unsigned long long t, unsigned long long j)
{
    return pgl_hmc_normal(pgl_hmc_key(seed, n, t), j);
}
double hmc_uniform(unsigned long long seed, unsigned long long n, unsigned long long t)
{
    return pgl_hmc_accept_uniform(pgl_hmc_key(seed, n, t));
}
int hmc_nscal(void) { return (int)(sizeof(PglHmc) / sizeof(double)); }
long long hmc_state_doubles(int M, int P) { return (long long)M * P * PGL_HMC_NVEC + (long long)M * PGL_HMC_NSCAL; }
