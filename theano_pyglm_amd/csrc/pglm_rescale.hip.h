// Time-rescaling goodness of fit (Brown et al. 2002): the integrated rate between consecutive events of every neuron,
//     tau_k = dt * sum_{s = t_{k-1}+1 .. t_k} lam_s,     lam_t = nlin(bias_n + GX[t][n]),
// from the bias-free total currents the forward-only pass leaves in GX (rows [t][n], row stride xs) and the per-neuron event
// lists.  A segmented sum over time, memory-bound with ONE read of GX and no (nT, N) rate array, in three launches:
//   k_rescale_chunk   time chunks of PGL_RS_CHUNK bins x columns of GX, a thread per (chunk, neuron) on the walk of
//                     pglm_binwalk.hip.h (which has the geometry, the source struct and the chunk length): rate (all f64:
//                     pgl_lambda_only), running sum, the sum so far at every event bin of the chunk (pre[event]), and the
//                     chunk total;
//   k_rescale_scan    exclusive prefix of the chunk totals of every neuron, in chunk order (64 segments of consecutive
//                     chunks per neuron, each summed in order, the segment sums scanned in order);
//   k_rescale_finish  tau_k from the two in-chunk sums and whole-chunk totals (events in the same or in neighbouring chunks
//                     never see the difference of two long prefixes), expected count, event count, multi-spike bins.
// Every sum has a fixed order: the results are bit-reproducible from run to run.
#pragma once

#define PGL_RS_SEGS 64        // segments of the scan (k_rescale_scan runs 16 neurons x 64 segments per workgroup)

struct RescaleParams {
    BinSource src;            // currents, biases, event lists, time range (pglm_binwalk.hip.h)
    double* pre;              // (nnz) sum of the rate over the event's chunk up to and including its bin
    double* tot;              // (nchunks, xs) chunk totals
    double* cum;              // (nchunks + 1, xs) exclusive prefix of the chunk totals; row nchunks = the whole range
    const long long* off;     // (N + 1) interval offsets of the caller
    double* tau;              // concatenated intervals
    double* stats;            // (N, 4): expected count, events, multi-spike bins, reserved
    int nchunks;
};

template <int NLIN>
__global__ __launch_bounds__(256) void k_rescale_chunk(const RescaleParams p)
{
    const BinSource& s = p.src;
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int j = (int)(g % s.xs);
    const long long c = g / s.xs;
    if (c >= p.nchunks || j >= s.N) return;
    const long long t0 = s.t_lo + c * PGL_RS_CHUNK;
    const int len = (int)((s.t_hi - t0 < PGL_RS_CHUNK) ? s.t_hi - t0 : PGL_RS_CHUNK);
    double acc = 0.0;
    pgl_bin_walk(
        s, j, t0, len, [](const double xv) { return pgl_lambda_only(xv, NLIN, PGL_C); },
        [&](int, const bool live, double, const double lam, const bool event, int, const int ei) {
            acc += live ? lam : 0.0;
            if (event) p.pre[ei] = acc;
        });
    p.tot[(size_t)c * s.xs + j] = acc;
}

// one workgroup per 16 columns: thread = (segment, column)
__global__ __launch_bounds__(16 * PGL_RS_SEGS) void k_rescale_scan(const RescaleParams p)
{
    __shared__ double seg[PGL_RS_SEGS][16];
    const int j = blockIdx.x * 16 + (threadIdx.x & 15);
    const int s = threadIdx.x >> 4;
    const int per = (p.nchunks + PGL_RS_SEGS - 1) / PGL_RS_SEGS;
    const int c0 = (s * per < p.nchunks) ? s * per : p.nchunks;
    const int c1 = (c0 + per < p.nchunks) ? c0 + per : p.nchunks;
    const bool live = j < p.src.N;
    double sum = 0.0;
    if (live)
        for (int c = c0; c < c1; ++c) sum += p.tot[(size_t)c * p.src.xs + j];
    seg[s][threadIdx.x & 15] = sum;
    __syncthreads();
    if (s == 0) {
        double run = 0.0;
        for (int i = 0; i < PGL_RS_SEGS; ++i) {
            const double v = seg[i][threadIdx.x];
            seg[i][threadIdx.x] = run;
            run += v;
        }
    }
    __syncthreads();
    if (!live) return;
    double run = seg[s][threadIdx.x & 15];
    for (int c = c0; c < c1; ++c) {
        p.cum[(size_t)c * p.src.xs + j] = run;
        run += p.tot[(size_t)c * p.src.xs + j];
    }
    if (s == PGL_RS_SEGS - 1) p.cum[(size_t)p.nchunks * p.src.xs + j] = run;     // (an empty last segment starts at the total)
}

// one workgroup per neuron
__global__ __launch_bounds__(256) void k_rescale_finish(const RescaleParams p)
{
    __shared__ int multi[4];
    const int n = blockIdx.x;
    int end;
    const int e0 = pgl_rs_first_event(p.src, n, p.src.t_lo, end);
    const int e1 = pgl_rs_first_event(p.src, n, p.src.t_hi, end);
    const long long o0 = p.off[n];
    const long long room = p.off[n + 1] - o0;
    int nm = 0;
    for (int i = e0 + threadIdx.x; i < e1; i += 256) {
        const int2 b = p.src.spk[i];
        nm += b.y > 1;
        if (i == e0 || i - e0 - 1 >= room) continue;            // the interval before the first event is censored
        const int2 a = p.src.spk[i - 1];
        const long long ca = (a.x - p.src.t_lo) / PGL_RS_CHUNK, cb = (b.x - p.src.t_lo) / PGL_RS_CHUNK;
        const double pa = p.pre[i - 1], pb = p.pre[i];
        double s;
        if (ca == cb) {
            s = pb - pa;
        } else {
            s = p.tot[(size_t)ca * p.src.xs + n] - pa;
            if (cb > ca + 1) s += p.cum[(size_t)cb * p.src.xs + n] - p.cum[(size_t)(ca + 1) * p.src.xs + n];
            s += pb;
        }
        p.tau[o0 + (i - e0 - 1)] = p.src.dt * s;
    }
    for (int o = 32; o > 0; o >>= 1) nm += __shfl_down(nm, o, 64);
    if ((threadIdx.x & 63) == 0) multi[threadIdx.x >> 6] = nm;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* st = p.stats + (size_t)n * 4;
        st[0] = p.src.dt * p.cum[(size_t)p.nchunks * p.src.xs + n];
        st[1] = (double)(e1 - e0);
        st[2] = (double)(multi[0] + multi[1] + multi[2] + multi[3]);
        st[3] = 0.0;
    }
}
