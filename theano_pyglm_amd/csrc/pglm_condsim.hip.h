// Clamped simulation on the device (the rules: pglm_condsim.h).
//   k_cond_currents   Xc from X0, AW and the recorded events: a gather per (t, q), a thread per element with the lanes over q,
//                     so the AW[p][tau][.] rows are read at full line width and the event lists of a bin are read by all the
//                     lanes of that bin at one address.  pgl_cs_current itself: the order of the rule, nothing races.
//   k_simulate_cond   ONE WAVE PER (neuron, 64 replicates): a lane owns one chain for all nT bins.  The lanes of a wave share
//                     the neuron, so what the chain reads is wave-uniform and lives in LDS: the self-history h_n (R doubles,
//                     gathered once) and a tile of 64 bins of Xc[., n] that lane i fetches for bin tile + i, one tile ahead.
//                     The time loop of a chain that stays on its queue has no global load in it (the memory counter of the
//                     wave is in order: a load inside the loop would wait for the prefetch of the next tile too).
//     self-history    a circular queue per lane of the own spike bins of the last R bins (PGL_CS_QUEUE entries of 32 bits in
//                     LDS: the bin's low 28 bits and the scattered rounds), evaluated oldest first onto Xc[t, n]: the order in
//                     which a ring would have received them, the same bits.
//     fallback        a push onto a full queue moves the chain to a ring of R doubles in the global workspace for the rest
//                     of its bins: the ring is built from Xc and the queue in the same order, then runs as k_simulate's does
//                     (slot t % R holds the total current of bin t, refilled with Xc[t + R]).  Nothing is dropped; flag bit 0
//                     starts every chain on the ring.
//     accumulators    at the end of a window the wave reduces its lanes' counts (sums, min, max) and lane 0 issues at most six
//                     int64 atomics; integers, so the order does not matter.  No f64 atomics.
// Every loop has a static bound: nT bins, at most 10 rounds per bin, at most PGL_CS_QUEUE queue entries, R taps.
#pragma once

#include "pglm_condsim.h"

#define PGL_CS_TMASK 0x0fffffffu

struct CondSimParams {
    const double* Xc;         // (nT, N)
    const double* AW;         // (N, R, N): only [n, :, n] is read
    const long long* obs;     // (n_win, N) recorded window counts
    double* ring;             // (N, R, n_rep) rings of the fallback
    long long* acc;           // (6, n_win, N)
    long long* exc;           // (N), added to
    long long* counts;        // (n_rep, N) or null
    unsigned char* S;         // (n_rep, nT, N) or null
    long long* fallbacks;     // (1), added to, or null
    long long nT, win, n_win;
    int N, R, n_rep, rep0, flags;
    unsigned long long seed;
    double dt;
};

__global__ __launch_bounds__(256) void k_cond_currents(const double* __restrict__ X0, const double* __restrict__ AW,
                                                       const int* __restrict__ ev_pre, const unsigned char* __restrict__ ev_cnt,
                                                       const long long* __restrict__ bin_off, double* __restrict__ Xc,
                                                       long long nT, int N, int R)
{
    const long long n = nT * N;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        Xc[i] = pgl_cs_current(i / N, (int)(i % N), N, R, X0, AW, ev_pre, ev_cnt, bin_off);
}

__global__ __launch_bounds__(256) void k_cond_acc_init(long long* __restrict__ acc, long long* __restrict__ exc,
                                                       long long* __restrict__ fallbacks, long long plane, int N)
{
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < plane) {
        acc[i] = acc[plane + i] = acc[2 * plane + i] = acc[3 * plane + i] = acc[5 * plane + i] = 0;
        acc[4 * plane + i] = PGL_CS_MIN_INIT;
    }
    if (i < N) exc[i] = 0;
    if (i == 0 && fallbacks) *fallbacks = 0;
}

__device__ __forceinline__ long long pgl_cs_wave_sum(long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int NLIN>
__global__ __launch_bounds__(64) void k_simulate_cond(const CondSimParams p)
{
    extern __shared__ double cs_h[];                           // (R) self-history of the wave's neuron
    __shared__ unsigned queue[PGL_CS_QUEUE * 64];              // entry j of lane l: queue[j * 64 + l]
    __shared__ double xt[2][64];                               // two tiles of Xc[., n]
    const int lane = threadIdx.x, N = p.N, R = p.R;
    const int groups = (p.n_rep + 63) >> 6;
    const int n = blockIdx.x / groups, r = (blockIdx.x % groups) * 64 + lane;
    const bool own = r < p.n_rep;
    const long long nT = p.nT;
    const double* __restrict__ Xn = p.Xc + n;
    for (int i = lane; i < R; i += 64) cs_h[i] = p.AW[((size_t)n * R + i) * N + n];
    xt[0][lane] = (lane < nT) ? Xn[(size_t)lane * N] : 0.0;
    const pgl_cs_u64 key = pgl_cs_key(p.seed, (pgl_cs_u64)p.rep0 + (pgl_cs_u64)r, (pgl_cs_u64)n);
    pgl_cs_u64 k = 1;
    double acc = 0.0, thr = pgl_cs_threshold(key, 0);
    long long count = 0, nexc = 0, wc = 0, w = 0, wleft = p.win;
    int qh = 0, qn = 0, slot = 0, cur = 0;
    bool ring = own && (p.flags & 1);
    double* __restrict__ rg = p.ring + (size_t)n * R * p.n_rep + (own ? r : 0);        // slot s: rg[s * n_rep]
    const size_t rs = (size_t)p.n_rep;
    if (ring)
        for (int u = 0; u < R; ++u) rg[u * rs] = (u < nT) ? Xn[(size_t)u * N] : 0.0;
    __syncthreads();
    for (long long tb = 0; tb < nT; tb += 64) {
        const long long tn = tb + 64 + lane;
        const double xnext = (tn < nT) ? Xn[(size_t)tn * N] : 0.0;                     // the next tile, in flight over this one
        const int len = (int)((nT - tb < 64) ? nT - tb : 64);
        for (int i = 0; i < len; ++i) {
            const long long t = tb + i;
            const unsigned tl = (unsigned)t & PGL_CS_TMASK;
            double x = xt[cur][i];
            if (ring) {
                x = rg[slot * rs];
                rg[slot * rs] = (t + R < nT) ? Xn[(size_t)(t + R) * N] : 0.0;
            } else {
                while (qn > 0 && ((tl - (queue[qh * 64 + lane] & PGL_CS_TMASK)) & PGL_CS_TMASK) > (unsigned)R) {
                    qh = (qh + 1 == PGL_CS_QUEUE) ? 0 : qh + 1;
                    --qn;
                }
                int j = qh;
                for (int e = 0; e < qn; ++e) {                                         // oldest first
                    const unsigned v = queue[j * 64 + lane];
                    const double hv = cs_h[((tl - (v & PGL_CS_TMASK)) & PGL_CS_TMASK) - 1];
                    for (int c = (int)(v >> 28); c > 0; --c) x += hv;
                    j = (j + 1 == PGL_CS_QUEUE) ? 0 : j + 1;
                }
            }
            int ns = 0, sb = 0;
            if (own) sb = pgl_cs_bin(x, NLIN, p.dt, key, &k, &acc, &thr, &ns, &nexc, (double*)nullptr);
            if (own && p.S) p.S[((size_t)r * nT + t) * N + n] = (unsigned char)sb;
            count += sb;
            wc += sb;
            if (ns > 0) {
                const int nel = (int)((nT - t - 1 < R) ? nT - t - 1 : R);
                if (!ring) {
                    if (qn < PGL_CS_QUEUE) {
                        int j = qh + qn;
                        if (j >= PGL_CS_QUEUE) j -= PGL_CS_QUEUE;
                        queue[j * 64 + lane] = tl | ((unsigned)ns << 28);
                        ++qn;
                    } else {                                                           // the ring of bins t + 1 .. t + R
                        ring = true;
                        if (p.fallbacks) atomicAdd((unsigned long long*)p.fallbacks, 1ULL);
                        for (int a = 0; a < nel; ++a) {
                            const long long u = t + 1 + a;
                            const unsigned ul = (unsigned)u & PGL_CS_TMASK;
                            double v = Xn[(size_t)u * N];
                            int j = qh;
                            for (int e = 0; e < PGL_CS_QUEUE; ++e) {
                                const unsigned qv = queue[j * 64 + lane];
                                const unsigned d = (ul - (qv & PGL_CS_TMASK)) & PGL_CS_TMASK;
                                if (d <= (unsigned)R) {
                                    const double hv = cs_h[d - 1];
                                    for (int c = (int)(qv >> 28); c > 0; --c) v += hv;
                                }
                                j = (j + 1 == PGL_CS_QUEUE) ? 0 : j + 1;
                            }
                            int sl = slot + 1 + a;
                            if (sl >= R) sl -= R;
                            rg[sl * rs] = v;
                        }
                        for (int a = nel; a < R; ++a) {                                // past the end of the recording
                            int sl = slot + 1 + a;
                            if (sl >= R) sl -= R;
                            rg[sl * rs] = 0.0;
                        }
                    }
                }
                if (ring) {
                    for (int a = 0; a < nel; ++a) {
                        int sl = slot + 1 + a;
                        if (sl >= R) sl -= R;
                        double v = rg[sl * rs];
                        const double hv = cs_h[a];
                        for (int c = ns; c > 0; --c) v += hv;
                        rg[sl * rs] = v;
                    }
                }
            }
            if (++slot == R) slot = 0;
            if (--wleft == 0 || t == nT - 1) {                                         // the end of window w: uniform in the wave
                const long long idx = w * N + n, plane = p.n_win * N;
                const long long ob = p.obs[idx];
                const long long s1 = pgl_cs_wave_sum(own ? wc : 0), s2 = pgl_cs_wave_sum(own ? wc * wc : 0);
                const long long lt = pgl_cs_wave_sum((own && wc < ob) ? 1 : 0), eq = pgl_cs_wave_sum((own && wc == ob) ? 1 : 0);
                long long mn = own ? wc : PGL_CS_MIN_INIT, mx = own ? wc : 0;
                for (int o = 32; o > 0; o >>= 1) {
                    const long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
                    mn = (a < mn) ? a : mn;
                    mx = (b > mx) ? b : mx;
                }
                if (lane == 0) {
                    long long* A = p.acc + idx;
                    if (s1) atomicAdd((unsigned long long*)A, (unsigned long long)s1);
                    if (s2) atomicAdd((unsigned long long*)(A + plane), (unsigned long long)s2);
                    if (lt) atomicAdd((unsigned long long*)(A + 2 * plane), (unsigned long long)lt);
                    if (eq) atomicAdd((unsigned long long*)(A + 3 * plane), (unsigned long long)eq);
                    atomicMin(A + 4 * plane, mn);
                    if (mx) atomicMax(A + 5 * plane, mx);
                }
                wc = 0;
                wleft = p.win;
                ++w;
            }
        }
        __syncthreads();                                                               // every lane is done with tile cur ^ 1 ..
        xt[cur ^ 1][lane] = xnext;
        cur ^= 1;
        __syncthreads();                                                               // .. and sees the next one
    }
    if (own && p.counts) p.counts[(size_t)r * N + n] = count;
    const long long ne = pgl_cs_wave_sum(own ? nexc : 0);
    if (lane == 0 && ne) atomicAdd((unsigned long long*)(p.exc + n), (unsigned long long)ne);
}
