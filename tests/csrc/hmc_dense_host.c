/* Host build of the dense-mass HMC chain (theano_pyglm_amd/csrc/pglm_hmc_dense.h over pglm_hmc.h) for the CPU tests and as
 * the mirror of the device chain: hmc_host.c (included as text: its target, its state block, hmc_init and the rest are
 * this file's too) plus the two calls that differ, pgl_hmc_dense_begin_dev / _leap_dev with host pointers.
 *   W: (M, P, P) row-major, lower-triangular factors of the inverse mass matrices; only j <= i is read.
 * The state's p array holds the whitened momentum r = W^T p.  Sums run in index order. */
#include "hmc_host.c"
#include "../../theano_pyglm_amd/csrc/pglm_hmc_dense.h"

/* r[c] -= scale step (W^T g)[c] for every c of one row */
static void kick(const double* W, int P, double* r, double scale, double step, const double* g)
{
    for (int c = 0; c < P; ++c) r[c] = pgl_hmcd_kick(r[c], scale, step, pgl_hmcd_col_dot(W, P, c, g, 0, 1));
}
/* q[c] += step (W r)[c], Xt = q */
static void drift(const double* W, int P, double* q, double step, const double* r, double* Xt)
{
    for (int c = 0; c < P; ++c) {
        q[c] = pgl_hmcd_drift(q[c], step, pgl_hmcd_row_dot(W, P, c, r, 0, 1));
        Xt[c] = q[c];
    }
}

/* y (M, P) = W x (trans == 0) or W^T x */
void hmcd_tri_matvec(const double* W, int M, int P, int trans, const double* x, double* y)
{
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < P; ++c)
            y[(long)r * P + c] = trans ? pgl_hmcd_col_dot(W + (long)r * P * P, P, c, x + (long)r * P, 0, 1)
                                       : pgl_hmcd_row_dot(W + (long)r * P * P, P, c, x + (long)r * P, 0, 1);
}

void hmcd_begin(double* st, int M, int P, const double* W, double* Xt)
{
    const long MP = (long)M * P;
    double *Q = st, *R = st + MP, *Q0 = st + 2 * MP, *G = st + 3 * MP, *sc = st + PGL_HMC_NVEC * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        PglHmc s;
        load(sc, M, r, &s);
        const pgl_hmc_u64 key = pgl_hmc_row_key(&s);
        double ks = 0.0;
        for (int c = 0; c < P; ++c) {
            R[o + c] = pgl_hmc_normal(key, (pgl_hmc_u64)c);
            ks += pgl_hmcd_kinetic_elem(R[o + c]);
            Q0[o + c] = Q[o + c];
        }
        pgl_hmc_begin(&s, ks);
        store(sc, M, r, &s);
        kick(W + o * P, P, R + o, 0.5, s.step, G + o);
        drift(W + o * P, P, Q + o, s.step, R + o, Xt + o);
    }
}

/* margin_out (M) or NULL: |log u - (H0 - H1)| of each row's decision (last != 0) */
void hmcd_leap(double* st, int M, int P, const double* W, double* ll, double* grad, int kind, int N, int B, int Dstim,
               const double* prm, int last, int n_warmup, double* Xt, double* sample_out, double* margin_out)
{
    const Prior q = prior(kind, N, B, Dstim, prm);
    const long MP = (long)M * P;
    double *Q = st, *R = st + MP, *Q0 = st + 2 * MP, *G = st + 3 * MP, *sc = st + PGL_HMC_NVEC * MP;
    for (int r = 0; r < M; ++r) {
        const long o = (long)r * P;
        PglHmc s;
        load(sc, M, r, &s);
        const double U1 = target(&q, P, Q + o, grad + o, ll[r]);
        ll[r] = U1;
        kick(W + o * P, P, R + o, last ? 0.5 : 1.0, s.step, grad + o);
        if (!last) {
            drift(W + o * P, P, Q + o, s.step, R + o, Xt + o);
            continue;
        }
        double ks = 0.0;
        for (int c = 0; c < P; ++c) ks += pgl_hmcd_kinetic_elem(R[o + c]);
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
