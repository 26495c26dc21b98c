// Clamped simulation: every neuron simulated with only its OWN spikes fed back, all the other neurons held at their recorded
// spikes (the single-neuron prediction given the population activity of Pillow et al., Nature 454 (2008) 995-999).  The rules
// and nothing else -- the callers (k_cond_currents / k_simulate_cond of pglm_condsim.hip.h on the device, pgl_simulate_cond_streams
// and tests/csrc/condsim_host.c on the host) own the arrays.
//
// Clamped currents.  Xc[t, q] = X0[t, q] (bias + stimulus), then the recorded spikes of the OTHER neurons are added in a fixed
// order: bins s = max(0, t - R) .. t - 1 ascending; inside a bin the presynaptic neurons p != q ascending; AW[p, t - s - 1, q]
// added once per spike of the recorded count (repeated addition, no multiply).  The order is part of the rule.  The events
// come as lists sorted by (bin, pre): ev_pre (E) int32, ev_cnt (E) uint8 (>= 1), bin_off (nT + 1) int64 with bin s owning
// events bin_off[s] .. bin_off[s + 1] - 1.  AW is [n_pre][tau][n_post], (N, R, N), as pgl_simulate_streams takes it.
//
// One chain (replicate r, neuron n).  pgl_simulate_streams' loop for a neuron that is alone: the same threshold stream
// thr(seed, r, n, k), the same rate function, acc update, clamp and redraw.  Per bin t:
//     x = Xc[t, n] + the self-history: h_n[t - s - 1] = AW[n, t - s - 1, n] for every OWN spike at a bin s in t - R .. t - 1 that
//         a round scattered, in ascending s, once per spike (the order in which pgl_simulate_streams' scatter reaches X[t, n]);
//     acc += rate(x) * dt;  S = (acc > thr);
//     while acc > thr:  if S >= 10: one exception, the round is dropped (no scatter, acc and thr stay)  -- else the spike is
//         scattered, acc -= thr, a new threshold is drawn, acc = max(acc, 0), and S += (acc > thr).
// The 10-spikes-per-bin cap is population-wide in pgl_simulate_streams (any neuron at 10 drops the round of all); here it is
// the neuron's own, as if the neuron were alone, and exceptions are counted per neuron.  As there, the bin that hits the cap
// records S = 10 although only 9 rounds were scattered.  Whenever pgl_simulate_streams(N, X = Xc, AW with only its [n, :, n]
// entries kept, rep = r, seed) reports 0 exceptions its column n is this chain, spike for spike.
//
// Accumulators.  Windows of win bins counted from bin 0, the last one may be short: n_win = ceil(nT / win).  Per (window,
// neuron), over the replicates of a call, six int64 planes (6, n_win, N): sum c, sum c^2, #(c < obs), #(c = obs), min c, max c
// with c the replicate's count in the window and obs the recorded one.  Integers: the result does not depend on the order.
// An initialising call starts from (0, 0, 0, 0, INT64_MAX, 0) -- counts are >= 0 and a call has at least one replicate, so 0
// is the identity of max; a continuing call folds onto what is there.
//
// Plain C subset, usable from host and device code.
#ifndef PGLM_CONDSIM_H
#define PGLM_CONDSIM_H

#include "pglm_hmc.h"

#define PGL_CS_FN PGL_HMC_FN
#define PGL_CS_NACC 6             // planes of the accumulator block
#define PGL_CS_CAP 10             // spikes per bin and neuron
#define PGL_CS_QUEUE 32           // the device's per-chain queue of own spike bins; beyond it a chain moves to a ring
#define PGL_CS_MAX_R 4096         // taps of the self-history the kernel keeps in LDS
#define PGL_CS_MIN_INIT 0x7fffffffffffffffLL

typedef unsigned long long pgl_cs_u64;

PGL_CS_FN long long pgl_cs_windows(long long nT, long long win) { return (nT + win - 1) / win; }

// the stream rule of pgl_simulate_streams (include/pyglm_hip.h)
PGL_CS_FN pgl_cs_u64 pgl_cs_key(pgl_cs_u64 seed, pgl_cs_u64 r, pgl_cs_u64 n)
{
    return pgl_hmc_mix(pgl_hmc_mix(pgl_hmc_mix(seed + PGL_HMC_G) + PGL_HMC_G * (r + 1)) + PGL_HMC_G * (n + 1));
}
PGL_CS_FN double pgl_cs_uniform(pgl_cs_u64 key, pgl_cs_u64 k)
{
    const pgl_cs_u64 z = pgl_hmc_mix(key + PGL_HMC_G * (k + 1));
    return ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// rate and threshold: the host takes libm as pgl_simulate_streams does, the device its own f64 functions with the series of
// log1p chosen per lane (pgl_rw_lambda: a chain's bits do not depend on its neighbours in the wave)
PGL_CS_FN double pgl_cs_rate(double x, int nlin)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return pgl_rw_lambda(x, nlin, PGL_C);
#else
    return nlin == 1 ? fmax(x, 0.0) + log1p(exp(-fabs(x))) : exp(x);
#endif
}
PGL_CS_FN double pgl_cs_threshold(pgl_cs_u64 key, pgl_cs_u64 k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return -pgl_log(pgl_cs_uniform(key, k), PGL_C);
#else
    return -log(pgl_cs_uniform(key, k));
#endif
}

// Xc[t, q]
PGL_CS_FN double pgl_cs_current(long long t, int q, int N, int R, const double* X0, const double* AW, const int* ev_pre,
                                const unsigned char* ev_cnt, const long long* bin_off)
{
    double x = X0[t * N + q];
    for (long long s = (t > R) ? t - R : 0; s < t; ++s) {
        const long long tau = t - s - 1;
        for (long long e = bin_off[s]; e < bin_off[s + 1]; ++e) {
            const int pre = ev_pre[e];
            if (pre == q) continue;
            const double a = AW[((long long)pre * R + tau) * N + q];
            for (int c = ev_cnt[e]; c > 0; --c) x += a;
        }
    }
    return x;
}

// One bin of one chain at the total current x.  Returns the bin's spike count S; *nscat = the rounds that scattered (S, or 9
// where the cap dropped the tenth); *nexc += 1 for a dropped round; *closest (may be NULL) = the smallest |acc - thr| / thr of
// the comparisons so far.
PGL_CS_FN int pgl_cs_bin(double x, int nlin, double dt, pgl_cs_u64 key, pgl_cs_u64* k, double* acc, double* thr, int* nscat,
                         long long* nexc, double* closest)
{
    double a = *acc + pgl_cs_rate(x, nlin) * dt, th = *thr;
    int sb = 0, ns = 0;
    for (;;) {                                     // at most 10 rounds: every round but the last increments sb
        if (closest) {
            const double m = fabs(a - th) / th;
            if (m < *closest) *closest = m;
        }
        if (!(a > th)) break;
        ++sb;
        if (sb >= PGL_CS_CAP) {                    // the check sits after the increment and before the scatter
            ++*nexc;
            break;
        }
        ++ns;
        a -= th;
        th = pgl_cs_threshold(key, (*k)++);
        if (a < 0.0) a = 0.0;
    }
    *acc = a;
    *thr = th;
    *nscat = ns;
    return sb;
}

// One chain on the host: x (nT) work array, on entry column n of Xc, on exit the total current; h (R) = AW[n, :, n];
// S (nT) out with stride sS.  Returns the exceptions.
PGL_CS_FN long long pgl_cs_chain(long long nT, int R, int nlin, double dt, double* x, const double* h, pgl_cs_u64 seed,
                                 pgl_cs_u64 r, pgl_cs_u64 n, unsigned char* S, long long sS, double* closest)
{
    const pgl_cs_u64 key = pgl_cs_key(seed, r, n);
    pgl_cs_u64 k = 1;
    double acc = 0.0, thr = pgl_cs_threshold(key, 0);
    long long nexc = 0;
    for (long long t = 0; t < nT; ++t) {
        int ns = 0;
        const int sb = pgl_cs_bin(x[t], nlin, dt, key, &k, &acc, &thr, &ns, &nexc, closest);
        S[t * sS] = (unsigned char)sb;
        const long long t_imp = (nT - t - 1 < R) ? nT - t - 1 : R;
        for (int c = 0; c < ns; ++c)
            for (long long tau = 0; tau < t_imp; ++tau) x[t + 1 + tau] += h[tau];
    }
    return nexc;
}

// fold the window counts of one replicate of one neuron: S (nT) with stride sS, obs / planes with stride N between windows
PGL_CS_FN void pgl_cs_fold(long long nT, long long win, const unsigned char* S, long long sS, const long long* obs,
                           long long* acc, long long plane, long long N)
{
    const long long n_win = pgl_cs_windows(nT, win);
    for (long long w = 0; w < n_win; ++w) {
        const long long t1 = ((w + 1) * win < nT) ? (w + 1) * win : nT;
        long long c = 0;
        for (long long t = w * win; t < t1; ++t) c += S[t * sS];
        long long* a = acc + w * N;
        a[0] += c;
        a[plane] += c * c;
        a[2 * plane] += (c < obs[w * N]) ? 1 : 0;
        a[3 * plane] += (c == obs[w * N]) ? 1 : 0;
        if (c < a[4 * plane]) a[4 * plane] = c;
        if (c > a[5 * plane]) a[5 * plane] = c;
    }
}

PGL_CS_FN void pgl_cs_acc_init(long long* acc, long long plane)
{
    for (long long i = 0; i < plane; ++i) {
        acc[i] = acc[plane + i] = acc[2 * plane + i] = acc[3 * plane + i] = acc[5 * plane + i] = 0;
        acc[4 * plane + i] = PGL_CS_MIN_INIT;
    }
}

#endif
