// Goodness of fit by time rescaling, the rules every implementation shares (k_rcorr_chunk / k_rcorr_finish and k_ks_segment
// of pglm_gof.hip.h, the host mirror tests/csrc/gof_host.c): the discrete-time correction of the event bin's term
// (Haslinger, Pipa & Brown 2010) and the Kolmogorov-Smirnov distance of a sample of rescaled intervals from Exp(1).
//
// Corrected interval.  The model is Poisson per bin: P(event in bin s) = 1 - exp(-q_s), q_s = dt lam_s, so Haslinger's
// q = -log(1 - p) is the term the rescaling sums anyway, and only the event bin's own term changes -- the event happened
// somewhere inside its bin, not at its end:
//     open_k = dt sum_{s = t_{k-1}+1 .. t_k - 1} lam_s      the bins strictly between the two events (none: 0), summed on
//                                                            the absolute chunk grid, anew behind every event (pglm_rescale.hip.h)
//     q_k    = dt lam_{t_k}
//     e_k    = -log1p(u_k expm1(-q_k))                       in (0, q_k]: the inverse of the law of the event's place in
//                                                            its bin given that it lies there, at the uniform u_k
//     tau'_k = open_k + e_k
// u_k is stateless, the threshold stream of the simulation with the draw where that has the replicate:
//     u = ((double)(mix(mix(mix(mix(seed + G) + G (draw + 1)) + G (n + 1)) + G (j + 1)) >> 11) + 0.5) 2^-53      in (0, 1]
// n: NEURON index, j: the index of the event t_k in the neuron's whole event list of the data sequence (not in the time
// range: an interval has the same u whatever range it is computed in).  The corrected statistic is therefore a random
// function of `seed`; two calls with the same seed and draw give the same bits.
//
// KS distance of one segment tau_0 .. tau_{n-1}:
//     z_i = -expm1(-tau_i);  with z sorted ascending  D+ = max_p ((double)(p + 1) / (double)n - z_(p)),
//     D- = max_p (z_(p) - (double)p / (double)n),  p from 0;  D = max(D+, D-)     (numpy's arithmetic in gof.ks_uniform)
//     n < 2: the three distances are NaN;  any tau that is NaN or negative: NaN too (n is reported);  tau = +inf: z = 1.
// The maxima and the sorted values do not depend on how ties are ordered.
//
// The sort is a fixed network on the index space padded to a power of two P >= n, the indices >= n holding a virtual
// +inf that is never stored: merges k = 2, 4 .. P, each a flip step (i, i ^ (k - 1)) and half-cleaners (i, i + j),
// j = k / 4 .. 1.  EVERY compare-exchange puts the smaller value at the smaller index, so a pair whose upper index is >= n
// is already in order and is skipped; P log2(P) (log2(P) + 1) / 4 pairs whatever the values.  pgl_gof_pair_* are the index
// rules; PGL_KS_TILE consecutive elements hold every pair of a step whose span is below the tile.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_GOF_H
#define PGLM_GOF_H

#include "pglm_hmc.h"

#define PGL_GOF_FN PGL_HMC_FN
#define PGL_KS_NOUT 4             // columns of the result (M, 4): D, D+, D-, n
#define PGL_KS_TILE 4096          // doubles of a tile: the steps of span < PGL_KS_TILE run on one tile at a time

PGL_GOF_FN double pgl_gof_uniform(pgl_hmc_u64 seed, pgl_hmc_u64 draw, pgl_hmc_u64 n, pgl_hmc_u64 j)
{
    return pgl_hmc_uniform(pgl_hmc_key(seed, draw, n), j);
}

// the event bin's term: q = dt lam of the bin, u in (0, 1]
PGL_GOF_FN double pgl_gof_event_term(double q, double u) { return -log1p(u * expm1(-q)); }

PGL_GOF_FN double pgl_gof_corrected(double open, double q, double u) { return open + pgl_gof_event_term(q, u); }

PGL_GOF_FN double pgl_gof_z(double tau) { return -expm1(-tau); }

// a value that voids its segment: NaN or negative
PGL_GOF_FN int pgl_gof_bad(double tau) { return !(tau >= 0.0); }

PGL_GOF_FN double pgl_gof_dplus(double z, long long p, long long n) { return (double)(p + 1) / (double)n - z; }
PGL_GOF_FN double pgl_gof_dminus(double z, long long p, long long n) { return z - (double)p / (double)n; }

// smallest power of two >= n (n >= 1)
PGL_GOF_FN long long pgl_gof_pow2(long long n)
{
    long long P = 1;
    while (P < n) P <<= 1;
    return P;
}

// pair p (0 <= p < P / 2) of the flip step of merge k: the blocks of k elements, element r of the lower half against its mirror
PGL_GOF_FN void pgl_gof_pair_flip(long long p, long long k, long long* i, long long* l)
{
    const long long h = k >> 1, b = (p & ~(h - 1)) << 1, r = p & (h - 1);      // (b = (p / h) k: k is a power of two)
    *i = b + r;
    *l = b + k - 1 - r;
}

// pair p of the half-cleaner of stride j
PGL_GOF_FN void pgl_gof_pair_half(long long p, long long j, long long* i, long long* l)
{
    *i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
    *l = *i + j;
}

// the distances of a SORTED segment z_0 <= .. <= z_{n-1}, n >= 2, in ascending p; out: D, D+, D-, n
PGL_GOF_FN void pgl_gof_ks_sorted(const double* z, long long n, double* out)
{
    double dp = pgl_gof_dplus(z[0], 0, n), dm = pgl_gof_dminus(z[0], 0, n);
    for (long long p = 1; p < n; ++p) {
        const double a = pgl_gof_dplus(z[p], p, n), b = pgl_gof_dminus(z[p], p, n);
        if (a > dp) dp = a;
        if (b > dm) dm = b;
    }
    out[0] = dp > dm ? dp : dm;
    out[1] = dp;
    out[2] = dm;
    out[3] = (double)n;
}

// the network, serial, on z[0 .. n) in place (the host mirror's sort)
PGL_GOF_FN void pgl_gof_step(double* z, long long n, long long P, long long k, long long j)     // j = 0: the flip step of k
{
    for (long long p = 0; p < P / 2; ++p) {
        long long i, l;
        if (j == 0) pgl_gof_pair_flip(p, k, &i, &l);
        else pgl_gof_pair_half(p, j, &i, &l);
        if (l < n && z[i] > z[l]) {
            const double t = z[i];
            z[i] = z[l];
            z[l] = t;
        }
    }
}
PGL_GOF_FN void pgl_gof_sort_network(double* z, long long n)
{
    const long long P = pgl_gof_pow2(n);
    for (long long k = 2; k <= P; k <<= 1) {
        pgl_gof_step(z, n, P, k, 0);
        for (long long j = k >> 2; j >= 1; j >>= 1) pgl_gof_step(z, n, P, k, j);
    }
}

// one segment: tau[0 .. n) -> zs[0 .. n) (sorted where the segment is valid) and out (4)
PGL_GOF_FN void pgl_gof_ks_segment(const double* tau, long long n, double* zs, double* out)
{
    int bad = 0;
    for (long long i = 0; i < n; ++i) {
        bad |= pgl_gof_bad(tau[i]);
        zs[i] = pgl_gof_z(tau[i]);
    }
    out[3] = (double)n;
    if (n < 2 || bad) {
        out[0] = out[1] = out[2] = __builtin_nan("");
        return;
    }
    pgl_gof_sort_network(zs, n);
    pgl_gof_ks_sorted(zs, n, out);
}

// ---- the argument rules of the segmented entry points (pgl_ks_uniform*, pgl_rescale_acf*); each caller turns a nonzero
// answer into its own message
// the segment count M, one workgroup each along a grid's x: 1 .. 2^31 - 1.  0: fine, 1: not
PGL_GOF_FN int pgl_gof_bad_count(long long M) { return M < 1 || M > 0x7fffffffLL; }

// the offsets off[0 .. n] of n segments start at or above 0 and do not decrease.  0: fine; else 1 + the first index that
// breaks the rule -- 1: off[0] < 0, 1 + i: off[i] < off[i - 1]
PGL_GOF_FN long long pgl_gof_bad_offsets(const long long* off, long long n)
{
    if (off[0] < 0) return 1;
    for (long long i = 1; i <= n; ++i)
        if (off[i] < off[i - 1]) return 1 + i;
    return 0;
}

#endif
