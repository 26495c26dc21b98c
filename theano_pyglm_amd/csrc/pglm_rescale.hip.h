// Time-rescaling goodness of fit (Brown et al. 2002): the integrated rate between consecutive events of every neuron,
//     tau_k = dt * sum_{s = t_{k-1}+1 .. t_k} lam_s,     lam_t = nlin(bias_n + GX[t][n]),
// from the bias-free total currents the forward-only pass leaves in GX (rows [t][n], row stride xs) and the per-neuron event
// lists.  A segmented sum over time, memory-bound with ONE read of GX and no (nT, N) rate array, in three launches:
//   k_rescale_chunk   time chunks of PGL_RS_CHUNK bins x columns of GX; consecutive lanes hold consecutive neurons, so the 16
//                     lanes of a post tile read one 128-byte line of a row.  A thread walks its chunk in time order: rate
//                     (all f64: pgl_lambda_only), running sum, the sum so far at every event bin of the chunk (pre[event]),
//                     and the chunk total;
//   k_rescale_scan    exclusive prefix of the chunk totals of every neuron, in chunk order (64 segments of consecutive
//                     chunks per neuron, each summed in order, the segment sums scanned in order);
//   k_rescale_finish  tau_k from the two in-chunk sums and whole-chunk totals (events in the same or in neighbouring chunks
//                     never see the difference of two long prefixes), expected count, event count, multi-spike bins.
// Every sum has a fixed order: the results are bit-reproducible from run to run.
#pragma once

#define PGL_RS_CHUNK 256      // bins per chunk (a multiple of 16: chunk starts lie on the tile grid of the window tables)
#define PGL_RS_SEGS 64        // segments of the scan (k_rescale_scan runs 16 neurons x 64 segments per workgroup)
#define PGL_RS_UNROLL 8       // rows of GX a thread has in flight

struct RescaleParams {
    const double* GX;         // (nT, xs) bias-free total current
    const double* theta;      // (N, P): column 0 is the bias
    const int2* spk;          // event lists (bin, count), neuron after neuron, time-sorted
    const int* wlo;           // wlo[n] = first event of neuron n (tile 0 of the window table)
    const int* whi;           // whi[tile * N + n] = first event of neuron n in bin >= 16 tile + 15
    double* pre;              // (nnz) sum of the rate over the event's chunk up to and including its bin
    double* tot;              // (nchunks, xs) chunk totals
    double* cum;              // (nchunks + 1, xs) exclusive prefix of the chunk totals; row nchunks = the whole range
    const long long* off;     // (N + 1) interval offsets of the caller
    double* tau;              // concatenated intervals
    double* stats;            // (N, 4): expected count, events, multi-spike bins, reserved
    long long t_lo, t_hi;
    int N, xs, P, nnz, nchunks;
    double dt;
};

// first event of neuron n in a bin >= t, 0 <= t <= nT (index into spk; the neuron's list ends at `end`); Prm: RescaleParams,
// or the PointwiseParams of pglm_pointwise.hip.h (spk, wlo, whi, N, nnz)
template <class Prm>
__device__ __forceinline__ int pgl_rs_first_event(const Prm& p, const int n, const long long t, int& end)
{
    end = (n + 1 < p.N) ? p.wlo[n + 1] : p.nnz;
    const long long tile = t >> 4;
    int i = (tile == 0) ? p.wlo[n] : p.whi[(size_t)(tile - 1) * p.N + n];       // first event in a bin >= 16 tile - 1
    while (i < end && p.spk[i].x < t) ++i;
    return i;
}

template <int NLIN>
__global__ __launch_bounds__(256) void k_rescale_chunk(const RescaleParams p)
{
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int j = (int)(g % p.xs);
    const long long c = g / p.xs;
    if (c >= p.nchunks || j >= p.N) return;
    const long long t0 = p.t_lo + c * PGL_RS_CHUNK;
    const int len = (int)((p.t_hi - t0 < PGL_RS_CHUNK) ? p.t_hi - t0 : PGL_RS_CHUNK);
    const double bias = p.theta[(size_t)j * p.P];
    int eend;
    int ei = pgl_rs_first_event(p, j, t0, eend);
    long long tn = (ei < eend) ? p.spk[ei].x : -1;
    const double* __restrict__ gx = p.GX + (size_t)t0 * p.xs + j;
    double acc = 0.0;
    for (int k = 0; k < len; k += PGL_RS_UNROLL) {
        double x[PGL_RS_UNROLL];
#pragma unroll
        for (int u = 0; u < PGL_RS_UNROLL; ++u) x[u] = (k + u < len) ? gx[(size_t)(k + u) * p.xs] : 0.0;
#pragma unroll
        for (int u = 0; u < PGL_RS_UNROLL; ++u) {
            // (every lane evaluates every row, rows past the chunk's end at x = 0 and dropped: pgl_lambda_only picks its
            // series by a vote of the wave)
            const double lam = pgl_lambda_only(bias + x[u], NLIN, PGL_C);
            acc += (k + u < len) ? lam : 0.0;
            if (t0 + k + u == tn) {
                p.pre[ei] = acc;
                ++ei;
                tn = (ei < eend) ? p.spk[ei].x : -1;
            }
        }
    }
    p.tot[(size_t)c * p.xs + j] = acc;
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
    const bool live = j < p.N;
    double sum = 0.0;
    if (live)
        for (int c = c0; c < c1; ++c) sum += p.tot[(size_t)c * p.xs + j];
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
        p.cum[(size_t)c * p.xs + j] = run;
        run += p.tot[(size_t)c * p.xs + j];
    }
    if (s == PGL_RS_SEGS - 1) p.cum[(size_t)p.nchunks * p.xs + j] = run;     // (an empty last segment starts at the total)
}

// one workgroup per neuron
__global__ __launch_bounds__(256) void k_rescale_finish(const RescaleParams p)
{
    __shared__ int multi[4];
    const int n = blockIdx.x;
    int end;
    const int e0 = pgl_rs_first_event(p, n, p.t_lo, end);
    const int e1 = pgl_rs_first_event(p, n, p.t_hi, end);
    const long long o0 = p.off[n];
    const long long room = p.off[n + 1] - o0;
    int nm = 0;
    for (int i = e0 + threadIdx.x; i < e1; i += 256) {
        const int2 b = p.spk[i];
        nm += b.y > 1;
        if (i == e0 || i - e0 - 1 >= room) continue;            // the interval before the first event is censored
        const int2 a = p.spk[i - 1];
        const long long ca = (a.x - p.t_lo) / PGL_RS_CHUNK, cb = (b.x - p.t_lo) / PGL_RS_CHUNK;
        const double pa = p.pre[i - 1], pb = p.pre[i];
        double s;
        if (ca == cb) {
            s = pb - pa;
        } else {
            s = p.tot[(size_t)ca * p.xs + n] - pa;
            if (cb > ca + 1) s += p.cum[(size_t)cb * p.xs + n] - p.cum[(size_t)(ca + 1) * p.xs + n];
            s += pb;
        }
        p.tau[o0 + (i - e0 - 1)] = p.dt * s;
    }
    for (int o = 32; o > 0; o >>= 1) nm += __shfl_down(nm, o, 64);
    if ((threadIdx.x & 63) == 0) multi[threadIdx.x >> 6] = nm;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* st = p.stats + (size_t)n * 4;
        st[0] = p.dt * p.cum[(size_t)p.nchunks * p.xs + n];
        st[1] = (double)(e1 - e0);
        st[2] = (double)(multi[0] + multi[1] + multi[2] + multi[3]);
        st[3] = 0.0;
    }
}
