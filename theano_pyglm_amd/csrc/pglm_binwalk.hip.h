// The walk the diagnostics kernels share (k_rescale_chunk of pglm_rescale.hip.h, k_pw_chunk of pglm_pointwise.hip.h, k_rw_piece
// of pglm_ratewin.hip.h): a thread per (time unit, neuron) goes over about 256 consecutive bins of its column of the bias-free
// total currents the forward-only pass leaves in GX (rows [t][n], row stride xs), in time order, next to the neuron's event
// list.  Consecutive lanes hold consecutive neurons, so the 16 lanes of a post tile read one 128-byte line of a row.  BinSource
// is what such a kernel reads; pgl_bin_walk is the walk; the kernels differ in their rate function and in what they do per bin.
#pragma once

#define PGL_RS_CHUNK 256      // bins per chunk (a multiple of 16: chunk starts lie on the tile grid of the window tables)
#define PGL_RS_UNROLL 8       // rows of GX a thread has in flight

struct BinSource {
    const double* GX;         // (nT, xs) bias-free total current
    const double* theta;      // (N, P): column 0 is the bias
    const int2* spk;          // event lists (bin, count >= 1), neuron after neuron, time-sorted
    const int* wlo;           // wlo[n] = first event of neuron n (tile 0 of the window table)
    const int* whi;           // whi[tile * N + n] = first event of neuron n in bin >= 16 tile + 15
    long long t_lo, t_hi;
    int N, xs, P, nnz;
    double dt;
};

// first event of neuron n in a bin >= t, 0 <= t <= nT (index into spk; the neuron's list ends at `end`)
__device__ __forceinline__ int pgl_rs_first_event(const BinSource& s, const int n, const long long t, int& end)
{
    end = (n + 1 < s.N) ? s.wlo[n + 1] : s.nnz;
    const long long tile = t >> 4;
    int i = (tile == 0) ? s.wlo[n] : s.whi[(size_t)(tile - 1) * s.N + n];       // first event in a bin >= 16 tile - 1
    while (i < end && s.spk[i].x < t) ++i;
    return i;
}

// The bins t0 .. t0 + span of column j, PGL_RS_UNROLL rows of GX in flight.  rate(xv) is the rate at the current xv = bias + x;
// body(k, live, xv, lam, event, count, ei) gets bin t0 + k: whether an event lies in it, its spike count (0: no event) and its
// index in spk.
// Every lane evaluates every row of a group of PGL_RS_UNROLL, the rows past the span at x = 0 and with live = false: a rate
// function may pick its series by a vote of the wave (pgl_lambda_only), so its call stays in code all lanes reach.  The
// event cursor moves on live bins only: a dead row never reports an event (what a body did with one was dropped anyway --
// the sum of k_pw_chunk by its select, and the pre[] entry k_rescale_chunk wrote for an event in a bin >= t_hi is one
// k_rescale_finish never reads, its events end at the first one in a bin >= t_hi).
template <class Rate, class Body>
__device__ __forceinline__ void pgl_bin_walk(const BinSource& s, const int j, const long long t0, const int span, Rate&& rate,
                                             Body&& body)
{
    const double bias = s.theta[(size_t)j * s.P];
    int eend;
    int ei = pgl_rs_first_event(s, j, t0, eend);
    int2 nx = (ei < eend) ? s.spk[ei] : make_int2(-1, 0);       // the next event: (bin, count)
    const double* __restrict__ gx = s.GX + (size_t)t0 * s.xs + j;
    for (int k = 0; k < span; k += PGL_RS_UNROLL) {
        double x[PGL_RS_UNROLL];
#pragma unroll
        for (int u = 0; u < PGL_RS_UNROLL; ++u) x[u] = (k + u < span) ? gx[(size_t)(k + u) * s.xs] : 0.0;
#pragma unroll
        for (int u = 0; u < PGL_RS_UNROLL; ++u) {
            const bool live = k + u < span;
            const double xv = bias + x[u];
            const double lam = rate(xv);
            const bool event = live && t0 + k + u == nx.x;
            body(k + u, live, xv, lam, event, event ? nx.y : 0, ei);
            if (event) {
                ++ei;
                nx = (ei < eend) ? s.spk[ei] : make_int2(-1, 0);
            }
        }
    }
}
