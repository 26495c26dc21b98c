/* Host build of the product's proximal-gradient row state machine (theano_pyglm_amd/csrc/pglm_prox.h) for the CPU tests
 * and as the mirror of the device fit: M rows, driven by reverse communication the way the k_prox_* row kernels drive it --
 * the caller supplies ll and its gradient at the points the machine asks for.  The two calls are pgl_prox_init_dev /
 * _step_dev with host pointers; the state block has the device's layout:
 *   st: (5, M, P) x, xprev, y, g_x, g_y, then (PGL_PROX_NSCAL, M) the fields of PglProx.
 * Rows are [bias, w_stim (Dstim), w_ir (N, B)].  kind < 0: no prior on bias and stimulus weights (f = -ll); else the
 * Gaussian terms of pglm_prox.h.  Sums run in index order. */
#include "../../theano_pyglm_amd/csrc/pglm_prox.h"

typedef struct {
    int kind, N, B, Dstim;
    double mu_b, sg_b, stim_sigma, mu, sigma;
} Prior;

static void load(const double* sc, int M, int r, PglProx* s)
{
    double* f = (double*)s;
    for (int k = 0; k < PGL_PROX_NSCAL; ++k) f[k] = sc[(long)k * M + r];
}
static void store(double* sc, int M, int r, const PglProx* s)
{
    const double* f = (const double*)s;
    for (int k = 0; k < PGL_PROX_NSCAL; ++k) sc[(long)k * M + r] = f[k];
}

/* g: grad ll -> grad f in place; returns f */
static double smooth(const Prior* q, int P, const double* x, double* g, double ll)
{
    double lp = 0.0, d;
    if (q->kind < 0) {
        for (int c = 0; c < P; ++c) g[c] = pgl_hmc_grad_elem(g[c], 0.0);
        return pgl_hmc_energy(ll, 0.0);
    }
    lp += pgl_hmc_prior_bias(x[0], q->mu_b, q->sg_b, &d);
    g[0] = pgl_hmc_grad_elem(g[0], d);
    for (int c = 1; c < 1 + q->Dstim; ++c) {
        lp += pgl_hmc_prior_stim(x[c], q->stim_sigma, &d);
        g[c] = pgl_hmc_grad_elem(g[c], d);
    }
    for (int c = 1 + q->Dstim; c < P; ++c) g[c] = pgl_hmc_grad_elem(g[c], 0.0);
    return pgl_hmc_energy(ll, lp);
}

static double emit(const Prior* q, const double* y, const double* gy, double* xt, double t, double lam_s)
{
    const int o = 1 + q->Dstim;
    double mg = (double)INFINITY, m;
    for (int c = 0; c < o; ++c) xt[c] = pgl_prox_plain_step(y[c], t, gy[c]);
    for (int n = 0; n < q->N; ++n) {
        pgl_prox_group(y + o + n * q->B, gy + o + n * q->B, q->B, t, q->mu, t * lam_s, xt + o + n * q->B, &m);
        mg = pgl_prox_min(mg, m);
    }
    return mg;
}

static double kkt(const Prior* q, const double* x, const double* g, double lam_s)
{
    const int o = 1 + q->Dstim;
    double r = 0.0;
    for (int c = 0; c < o; ++c) r = pgl_ls_abs(g[c]) > r ? pgl_ls_abs(g[c]) : r;
    for (int n = 0; n < q->N; ++n) {
        const double e = pgl_prox_group_kkt(x + o + n * q->B, g + o + n * q->B, q->B, q->mu, lam_s);
        r = e > r ? e : r;
    }
    return r;
}

static double hsum(const Prior* q, const double* x, double lam_s)
{
    double h = 0.0;
    for (int n = 0; n < q->N; ++n) h += pgl_prox_group_h(x + 1 + q->Dstim + n * q->B, q->B, q->mu, lam_s);
    return h;
}

static Prior prior(int kind, int N, int B, int Dstim, const double* prm)
{
    Prior q = {kind, N, B, Dstim, prm[0], prm[1], prm[2], prm[3], prm[4]};
    return q;
}

/* prm: mu_b, sg_b, stim_sigma, mu, sigma */
void prox_init(double* st, int M, int P, double* ll, double* grad, int kind, int N, int B, int Dstim, const double* prm,
               const double* lam, double gtol, int maxiter, double* Xt)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double *X = st, *Xp = st + MP, *Y = st + 2 * MP, *Gx = st + 3 * MP, *Gy = st + 4 * MP, *sc = st + PGL_PROX_NVEC * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        const double lam_s = lam[r] / q.sigma;
        const double f = smooth(&q, P, X + o, grad + o, ll[r]);
        double gg = 0.0;
        for (int c = 0; c < P; ++c) {
            gg += grad[o + c] * grad[o + c];
            Gx[o + c] = Gy[o + c] = grad[o + c];
            Y[o + c] = Xp[o + c] = X[o + c];
        }
        PglProx s;
        pgl_prox_init(&s, f, hsum(&q, X + o, lam_s), gg);
        ll[r] = f;
        if (pgl_prox_kkt_test(&s, kkt(&q, X + o, grad + o, lam_s), gtol, maxiter)) {
            for (int c = 0; c < P; ++c) Xt[o + c] = X[o + c];
        } else {
            s.m_zero = pgl_prox_min(s.m_zero, emit(&q, Y + o, Gy + o, Xt + o, s.t, lam_s));
        }
        store(sc, M, r, &s);
    }
}

/* F_out (M) or NULL: F_x of every row that accepted a step in this call, NaN elsewhere */
void prox_step(double* st, int M, int P, double* ll, double* grad, int kind, int N, int B, int Dstim, const double* prm,
               const double* lam, double gtol, int maxiter, int max_backtrack, double* Xt, double* F_out)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double *X = st, *Xp = st + MP, *Y = st + 2 * MP, *Gx = st + 3 * MP, *Gy = st + 4 * MP, *sc = st + PGL_PROX_NVEC * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        double *x = X + o, *xp = Xp + o, *y = Y + o, *gx = Gx + o, *gy = Gy + o, *g = grad + o, *xt = Xt + o;
        PglProx s;
        load(sc, M, r, &s);
        if (F_out) F_out[r] = (double)NAN;
        if (s.phase == (double)PGL_PROX_DONE) continue;
        const double lam_s = lam[r] / q.sigma;
        const int trial = s.phase == (double)PGL_PROX_TRIAL;
        const double f = smooth(&q, P, xt, g, ll[r]);
        ll[r] = f;
        int from_x = 0;
        if (!trial) {
            if (pgl_prox_y_arrived(&s, f)) {
                for (int c = 0; c < P; ++c) gy[c] = g[c];
            } else from_x = 1;
        } else {
            double dot = 0.0, dd = 0.0;
            for (int c = 0; c < P; ++c) {
                const double d = xt[c] - y[c];
                dot += gy[c] * d;
                dd += d * d;
            }
            const int d = pgl_prox_decide(&s, f, hsum(&q, xt, lam_s), dot, dd, max_backtrack);
            if (d == PGL_PROX_D_FAIL) {
                for (int c = 0; c < P; ++c) xt[c] = x[c];
                store(sc, M, r, &s);
                continue;
            }
            if (d == PGL_PROX_D_ACCEPT) {
                for (int c = 0; c < P; ++c) {
                    xp[c] = x[c];
                    x[c] = xt[c];
                    gx[c] = g[c];
                }
                if (F_out) F_out[r] = s.F_x;
                if (pgl_prox_kkt_test(&s, kkt(&q, x, gx, lam_s), gtol, maxiter)) {
                    store(sc, M, r, &s);
                    continue;
                }
                const double beta = pgl_prox_momentum(&s);
                if (beta != 0.0) {
                    for (int c = 0; c < P; ++c) y[c] = xt[c] = pgl_prox_extrapolate(x[c], xp[c], beta);
                    store(sc, M, r, &s);
                    continue;
                }
            }
            from_x = d != PGL_PROX_D_BACKTRACK;
        }
        if (from_x)
            for (int c = 0; c < P; ++c) {
                y[c] = x[c];
                gy[c] = gx[c];
            }
        s.m_zero = pgl_prox_min(s.m_zero, emit(&q, y, gy, xt, s.t, lam_s));
        store(sc, M, r, &s);
    }
}

/* z (P) = prox_{t h}(v) of one row: the machine's group function with y = v, g = 0.  Returns 0, or -1 when B exceeds the
 * zero gradient kept here (nothing is written then). */
#define PROX_APPLY_MAXB 64
int prox_apply(const double* v, int P, int N, int B, int Dstim, double mu, double sigma, double lam, double t, double* z)
{
    const int o = 1 + Dstim;
    double m, zero[PROX_APPLY_MAXB] = {0};
    if (B <= 0 || B > PROX_APPLY_MAXB || P != o + N * B) return -1;
    for (int c = 0; c < o; ++c) z[c] = pgl_prox_plain_step(v[c], t, 0.0);
    for (int n = 0; n < N; ++n) pgl_prox_group(v + o + n * B, zero, B, t, mu, t * (lam / sigma), z + o + n * B, &m);
    return 0;
}

int prox_nscal(void) { return (int)(sizeof(PglProx) / sizeof(double)); }
double prox_allowance(void) { return PGL_PROX_C; }
long long prox_state_doubles(int M, int P) { return (long long)M * P * PGL_PROX_NVEC + (long long)M * PGL_PROX_NSCAL; }
