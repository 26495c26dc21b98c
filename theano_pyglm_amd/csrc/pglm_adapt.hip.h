// windowed diagonal mass adaptation: the state's view and the HMC row kernel k_hmc_mass_adapt
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// Mass adaptation during the warm-up of the lock-step samplers (mass='adapt'; the rules are pglm_adapt.h, compiled for the
// host by tests/csrc/adapt_host.c).  One workgroup of 256 threads per row; every element of a row belongs to one thread
// from the first read to the last write, so there are no reductions, no atomics and no scratch; the row's two scalars are
// tid 0's.  The state lives in ONE device block of doubles laid out by pgl_adapt_view.
//   HMC   k_hmc_mass_adapt, one small launch between the last leap of transition t and the begin of t + 1 (k_hmc_begin
//         reads minv at the start of each transition).
//   NUTS  rows are asynchronous: the same rules run inside the ADAPT variant of the step kernel (pglm_nuts.hip.h).
// ---------------------------------------------------------------------------
#include "pglm_adapt.h"

struct AdaptView {
    int R, P;
    double *mean, *m2;                        // (R, P): Welford mean and M2 of the running window
    double *count, *widx;                     // (R): PglAdapt, field-major
};
__host__ __device__ inline size_t pgl_adapt_doubles(int R, int P)
{
    return (size_t)R * P * PGL_ADAPT_NVEC + (size_t)R * PGL_ADAPT_NSCAL;
}
__host__ __device__ inline AdaptView pgl_adapt_view(double* st, int R, int P)
{
    AdaptView a;
    const size_t RP = (size_t)R * P;
    a.R = R; a.P = P;
    a.mean = st; a.m2 = st + RP;
    a.count = st + 2 * RP; a.widx = st + 2 * RP + R;
    return a;
}

// after the last leap of a transition (the state's t counts it already): the row's point enters the running window; at
// the window's end the row of minv (R, P) is rewritten and avg_accept restarts
__global__ __launch_bounds__(256) void k_hmc_mass_adapt(const HmcView v, const AdaptView a, const int* __restrict__ sched,
                                                        double* __restrict__ minv)
{
    __shared__ int sact;
    __shared__ double sn;
    const int r = blockIdx.x, tid = threadIdx.x, P = v.P;
    const size_t o = (size_t)r * P;
    if (tid == 0) {
        PglAdapt ad;
        ad.count = a.count[r]; ad.widx = a.widx[r];
        double n = 0.0;
        const int act = pgl_adapt_row(&ad, sched, (int)v.sc[(size_t)5 * v.M + r] - 1, &n);
        if (act) {
            a.count[r] = ad.count; a.widx[r] = ad.widx;
        }
        if (act & PGL_ADAPT_SWITCH) {
            PglHmc s;
            pgl_hmc_load(v, r, &s);
            pgl_adapt_restart_hmc(&s);
            pgl_hmc_store(v, r, &s);
        }
        sact = act; sn = n;
    }
    __syncthreads();
    const int act = sact;
    const double n = sn;
    if (!act) return;
    for (int c = tid; c < P; c += 256) {
        double mean = a.mean[o + c], m2 = a.m2[o + c];
        pgl_adapt_welford(v.q[o + c], n, &mean, &m2);
        if (act & PGL_ADAPT_SWITCH) {
            minv[o + c] = pgl_adapt_minv(m2, n);
            mean = 0.0; m2 = 0.0;
        }
        a.mean[o + c] = mean; a.m2[o + c] = m2;
    }
}
