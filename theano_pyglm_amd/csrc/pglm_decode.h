// Stimulus decoding: the MAP stimulus given the spikes of a fitted population (the decoding half of Pillow et al., Nature 454
// (2008) 995-999).  The rules and nothing else -- the callers (the k_dec_* kernels of pglm_decode.hip.h on the device,
// pgl_decode_host and tests/csrc/decode_host.c on the host) own the arrays.
//
// Served: a 'basis' stimulus (BasisStimulus: identity spatial basis, feature column d * B + b), exp and explinear.  The unknown
// is u (Tu, D) on the stimulus grid, dt_stim = q dt with an integer q >= 1.
//   s = L u          the stimulus on the bin grid: for t = q i + r,  s[t] = (1 - r / q) u[i] + (r / q) u[i + 1],  and
//                    s[t] = u[Tu - 1] for i >= Tu - 1 (np.interp's clamp; frames past the recording are not read);
//   K[tau, d, n]   = sum_b basis[tau, b] w_stim[n, d B + b], b ascending, tau = 0 .. Rt - 1;
//   I[t, n]        = sum_d sum_tau K[tau, d, n] s[t - 1 - tau, d], d ascending then tau ascending, strictly causal, s = 0
//                    before bin 0;
//   x = c + I        c[t, n] = bias_n + GX0[t, n], the currents of the recorded spikes at theta with the stimulus weights zero;
//   F(u)           = sum_t sum_n [S log lam(x) - dt lam(x)] + log p(u);   a bin with S = 0 contributes -dt lam (no 0 log 0);
//   r[t, n]        = S (log lam)'(x) - dt lam'(x):   exp: S - dt e^x;   explinear: (S / lam - dt) sig,  sig = 1 / (1 + e^-x);
//   cc[t, n]       = -dt lam''(x) + S (log lam)''(x), the c_t of pgl_hvp_* with its limits (include/pyglm_hip.h);
//   g_s[t', d]     = sum_n sum_tau K[tau, d, n] r[t' + 1 + tau, n], rows past nT are zero; n ascending, inside tau ascending;
//   g_u            = L^T g_s + grad log p(u):   frame i collects the bins q (i - 1) + 1 .. q i - 1 with weight r / q and, for
//                    i < Tu - 1, the bins q i .. q i + q - 1 with weight 1 - r / q; the last frame all bins >= q (Tu - 1) with
//                    weight 1; bins ascending;
//   H v            = L^T K^T (cc o (K L v)) + hess log p . v: the same two convolutions with cc in place of the rate function.
// Prior, per stimulus dimension: Gaussian with mean mu and precision (1 / sigma^2) I + (1 / rho^2) D^T D, D the first
// differences in time (tridiagonal); rho = inf gives the iid prior; the normalising constant is dropped:
//   log p(u)       = sum_d [ -1/2 sum_i (u_i - mu)^2 / sigma^2 - 1/2 sum_{i < Tu - 1} (u_{i+1} - u_i)^2 / rho^2 ]
//   grad_i         = -(u_i - mu) / sigma^2 - ((u_i - u_{i-1}) [i > 0] + (u_i - u_{i+1}) [i < Tu - 1]) / rho^2
//   (hess . v)_i   = -v_i / sigma^2 - ((v_i - v_{i-1}) [i > 0] + (v_i - v_{i+1}) [i < Tu - 1]) / rho^2.
//
// Plain C subset, usable from host and device code.  The host takes libm for the rate function, the device its own f64
// functions with the series of log1p chosen per lane (pgl_rw_lambda: an element's bits do not depend on its neighbours in the
// wave, so a result does not depend on how the grid is cut).
#ifndef PGLM_DECODE_H
#define PGLM_DECODE_H

#include "pglm_hmc.h"

#define PGL_DEC_FN PGL_HMC_FN
#define PGL_DEC_CHUNK 256         // bins per chunk of the ll partial sums (the chunk of pglm_binwalk.hip.h)
#define PGL_DEC_NF 3              // the doubles of an evaluation's result: F, log likelihood, log prior

typedef struct {
    double mu, sigma, rho;        // rho = inf (or <= 0): no smoothness term
} PglDecPrior;

PGL_DEC_FN double pgl_dec_inv_sq(double a) { return (a > 0.0 && a < __builtin_huge_val()) ? 1.0 / (a * a) : 0.0; }

// ---- L and L^T -------------------------------------------------------------------------------------------------------------
// s[t, d] of u (Tu, D)
PGL_DEC_FN double pgl_dec_interp_at(const double* u, long long Tu, int D, int q, long long t, int d)
{
    const long long i = t / q;
    if (i >= Tu - 1) return u[(Tu - 1) * D + d];
    const double w = (double)(t - i * q) / (double)q;
    return (1.0 - w) * u[i * D + d] + w * u[(i + 1) * D + d];
}

// (L^T g)[i, d] of g (nT, D): bins ascending
PGL_DEC_FN double pgl_dec_interp_t_at(const double* g, long long nT, int D, int q, long long Tu, long long i, int d)
{
    double a = 0.0;
    long long t = (i > 0) ? q * (i - 1) + 1 : 0;
    for (; t < q * i && t < nT; ++t) a += ((double)(t - q * (i - 1)) / (double)q) * g[t * D + d];
    if (i < Tu - 1) {
        for (t = q * i; t < q * (i + 1) && t < nT; ++t) a += (1.0 - (double)(t - q * i) / (double)q) * g[t * D + d];
    } else {
        for (t = q * i; t < nT; ++t) a += g[t * D + d];
    }
    return a;
}

// ---- the prior ---------------------------------------------------------------------------------------------------------------
// the term of element (i, d) of log p(u): its own square and the difference to its successor
PGL_DEC_FN double pgl_dec_prior_term(const double* u, long long Tu, int D, long long i, int d, const PglDecPrior* p)
{
    const double a = u[i * D + d] - p->mu;
    double v = -0.5 * pgl_dec_inv_sq(p->sigma) * a * a;
    if (i + 1 < Tu) {
        const double e = u[(i + 1) * D + d] - u[i * D + d];
        v -= 0.5 * pgl_dec_inv_sq(p->rho) * e * e;
    }
    return v;
}
// element (i, d) of grad log p at u (center = mu) or of hess log p . v (u = v, center = 0)
PGL_DEC_FN double pgl_dec_prior_lin(const double* u, long long Tu, int D, long long i, int d, const PglDecPrior* p, double center)
{
    const double ui = u[i * D + d];
    double lap = 0.0;
    if (i > 0) lap += ui - u[(i - 1) * D + d];
    if (i + 1 < Tu) lap += ui - u[(i + 1) * D + d];
    return -pgl_dec_inv_sq(p->sigma) * (ui - center) - pgl_dec_inv_sq(p->rho) * lap;
}

// ---- rate, residual, curvature of one element -----------------------------------------------------------------------------
// the ll term S log lam - dt lam, the residual r and the curvature cc at the current x and the spike count S
PGL_DEC_FN void pgl_dec_point(double x, double S, int nlin, double dt, double* term, double* r, double* cc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const double lam = pgl_rw_lambda(x, nlin, PGL_C);
    *cc = pgl_curvature(x, S, nlin, dt, PGL_C);
    if (nlin == 1) {
        const double e = pgl_exp(-fmin(fabs(x), 800.0), PGL_C);
        const double inv = pgl_rcp(1.0 + e);
        const double sig = (x >= 0.0) ? inv : e * inv;
        double t = -dt * lam, w = -dt;
        if (S > 0.0) {
            t = fma(S, pgl_log(lam, PGL_C), t);
            w = fma(S, pgl_rcp(lam), w);
        }
        *term = t;
        *r = w * sig;
    } else {
        *term = (S > 0.0) ? fma(S, x, -dt * lam) : -dt * lam;
        *r = fma(-dt, lam, S);
    }
#else
    if (nlin == 1) {
        const double e = exp(-fabs(x));
        const double lam = fmax(x, 0.0) + log1p(e);
        const double inv = 1.0 / (1.0 + e);
        const double sig = (x >= 0.0) ? inv : e * inv;
        double c = -dt * e * inv * inv;
        *term = -dt * lam;
        *r = -dt * sig;
        if (S > 0.0) {
            double h;
            *term += S * log(lam);
            *r = (S / lam - dt) * sig;
            if (x >= 0.0) h = inv * inv * (e * lam - 1.0) / (lam * lam);
            else if (e < 1.0e-2) {
                double l = 0.1, q = 2.0 / 11.0;            // l = log1p(e) / e, q = -2 (log1p(e) - e) / e^2, degree 9
                for (int k = 8; k >= 0; --k) {
                    l = 1.0 / (k + 1) - e * l;
                    q = 2.0 / (k + 2) - e * q;
                }
                h = -0.5 * e * inv * inv * q / (l * l);
            } else h = e * inv * inv * (lam - e) / (lam * lam);
            c += S * h;
        }
        *cc = c;
    } else {
        const double lam = exp(fmax(fmin(x, 709.0), -800.0));
        *term = -dt * lam + ((S > 0.0) ? S * x : 0.0);
        *r = S - dt * lam;
        *cc = -dt * lam;
    }
#endif
}

// ---- the filters and the two convolutions (host order; the kernels keep the same order per element) ------------------------
// K (Rt, D, N) from basis (Rt, B) and theta (N, P): the stimulus weights of neuron n are theta[n P + 1 + d B + b]
PGL_DEC_FN double pgl_dec_filter_at(const double* basis, int B, const double* theta, int P, int tau, int d, int n)
{
    double a = 0.0;
    for (int b = 0; b < B; ++b) a += basis[tau * B + b] * theta[(long long)n * P + 1 + d * B + b];
    return a;
}
// I[t, n] of s (nT, D)
PGL_DEC_FN double pgl_dec_conv_at(const double* K, int Rt, int D, int N, const double* s, long long t, int n)
{
    double a = 0.0;
    for (int d = 0; d < D; ++d)
        for (int tau = 0; tau < Rt && tau < t; ++tau) a += K[((long long)tau * D + d) * N + n] * s[(t - 1 - tau) * D + d];
    return a;
}
// (K^T y)[t', d] of y (nT, N)
PGL_DEC_FN double pgl_dec_corr_at(const double* K, int Rt, int D, int N, const double* y, long long nT, long long t, int d)
{
    double a = 0.0;
    for (int n = 0; n < N; ++n) {
        double b = 0.0;
        for (int tau = 0; tau < Rt && t + 1 + tau < nT; ++tau) b += K[((long long)tau * D + d) * N + n] * y[(t + 1 + tau) * N + n];
        a += b;
    }
    return a;
}

// ---- the whole evaluation on the host ---------------------------------------------------------------------------------------
// c, S (nT, N) (S: spike counts as doubles), K (Rt, D, N), u (Tu, D) -> F[PGL_DEC_NF], grad (Tu, D) or null; r, cc (nT, N) and
// s, gs (nT, D) are the caller's work arrays (r and cc are what pgl_dec_hvp_host reads).  The ll terms are added per
// (256-bin chunk, neuron), then chunks ascending, then neurons ascending, as the kernels add them.
PGL_DEC_FN void pgl_dec_eval_host(long long nT, int N, int nlin, double dt, const double* c, const double* S, const double* K, int Rt,
                                  int D, const double* u, long long Tu, int q, const PglDecPrior* prior, double* F, double* grad,
                                  double* r, double* cc, double* s, double* gs)
{
    for (long long t = 0; t < nT; ++t)
        for (int d = 0; d < D; ++d) s[t * D + d] = pgl_dec_interp_at(u, Tu, D, q, t, d);
    double ll = 0.0;
    for (int n = 0; n < N; ++n) {
        double col = 0.0;
        for (long long t0 = 0; t0 < nT; t0 += PGL_DEC_CHUNK) {
            double part = 0.0;
            for (long long t = t0; t < t0 + PGL_DEC_CHUNK && t < nT; ++t) {
                double term;
                pgl_dec_point(c[t * N + n] + pgl_dec_conv_at(K, Rt, D, N, s, t, n), S[t * N + n], nlin, dt, &term, &r[t * N + n],
                              &cc[t * N + n]);
                part += term;
            }
            col += part;
        }
        ll += col;
    }
    double lp = 0.0;
    for (long long i = 0; i < Tu; ++i)
        for (int d = 0; d < D; ++d) lp += pgl_dec_prior_term(u, Tu, D, i, d, prior);
    F[0] = ll + lp; F[1] = ll; F[2] = lp;
    if (!grad) return;
    for (long long t = 0; t < nT; ++t)
        for (int d = 0; d < D; ++d) gs[t * D + d] = pgl_dec_corr_at(K, Rt, D, N, r, nT, t, d);
    for (long long i = 0; i < Tu; ++i)
        for (int d = 0; d < D; ++d)
            grad[i * D + d] = pgl_dec_interp_t_at(gs, nT, D, q, Tu, i, d) + pgl_dec_prior_lin(u, Tu, D, i, d, prior, prior->mu);
}

// hv (Tu, D) = H v at the point whose curvature is in cc; s (nT, D), y (nT, N), gs (nT, D): work arrays
PGL_DEC_FN void pgl_dec_hvp_host(long long nT, int N, const double* cc, const double* K, int Rt, int D, const double* v, long long Tu,
                                 int q, const PglDecPrior* prior, double* hv, double* s, double* y, double* gs)
{
    for (long long t = 0; t < nT; ++t)
        for (int d = 0; d < D; ++d) s[t * D + d] = pgl_dec_interp_at(v, Tu, D, q, t, d);
    for (long long t = 0; t < nT; ++t)
        for (int n = 0; n < N; ++n) y[t * N + n] = cc[t * N + n] * pgl_dec_conv_at(K, Rt, D, N, s, t, n);
    for (long long t = 0; t < nT; ++t)
        for (int d = 0; d < D; ++d) gs[t * D + d] = pgl_dec_corr_at(K, Rt, D, N, y, nT, t, d);
    for (long long i = 0; i < Tu; ++i)
        for (int d = 0; d < D; ++d)
            hv[i * D + d] = pgl_dec_interp_t_at(gs, nT, D, q, Tu, i, d) + pgl_dec_prior_lin(v, Tu, D, i, d, prior, 0.0);
}

#endif
