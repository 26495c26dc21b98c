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
// The bodies are templates over CORR: false is the above; true is the discrete-time correction of pglm_gof.h, launched as
// k_rcorr_chunk / k_rcorr_finish (pglm_gof.hip.h) around the same k_rescale_scan.  The corrected variant's chunks lie on the
// ABSOLUTE grid of PGL_RS_CHUNK bins (the first and the last chunk of a range may be partial) and its in-chunk sums start
// anew behind every event: the sum an interval is made of -- behind the earlier event to the end of its chunk, the whole
// chunks between, the later event's chunk up to its bin -- never starts before the earlier event and is added in the same
// order in every time range that holds the interval: the same bits whatever pgl_set_time_range says.
// The rate: pgl_lambda_only picks the series of log1p by a vote of the wave, so the last bit of a lane's rate can depend on
// its wave-mates -- other neurons, other chunks, and WHICH chunks share a wave changes with t_lo.  The corrected intervals
// must not see that: their pieces (pre, qev, tail) take pgl_lambda_only's arithmetic with the series chosen per lane
// (pgl_rw_lambda of pglm_ratewin.hip.h, made for the same reason).  The chunk totals behind stats keep the voted rate: on a
// range that starts on the chunk grid the waves are those of k_rescale_chunk, and the expected count is that kernel's bits.
#pragma once
#include "pglm_gof.h"
#include "pglm_ratewin.hip.h"

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
    // the corrected variant only (CORR): pre holds the sum BEFORE the event bin's term -- since the previous event of the
    // chunk, or since the chunk's start --, qev the term itself
    double* qev;              // (nnz) rate of the event's bin
    double* tail;             // (nchunks_abs, xs) sum behind the last event of the chunk (no event: the chunk's total)
    const double* lam_row;    // (xs) sum of the rate over the range, for stats: the row of cum that a scan over the chunks
                              // from t_lo left (pgl_rescale_dev's own sum: the same bits)
    long long c0;             // first absolute chunk: t_lo / PGL_RS_CHUNK
    int nchunks_abs;          // chunks of the absolute grid that the range touches
    unsigned long long seed;
    long long draw;
};

template <int NLIN, bool CORR>
__device__ __forceinline__ void pgl_rescale_chunk_body(const RescaleParams& p)
{
    const BinSource& s = p.src;
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int j = (int)(g % s.xs);
    const long long c = g / s.xs;
    if (c >= (CORR ? p.nchunks_abs : p.nchunks) || j >= s.N) return;
    long long t0 = s.t_lo + c * PGL_RS_CHUNK, t1 = t0 + PGL_RS_CHUNK;
    if (CORR) {
        t0 = (p.c0 + c) * PGL_RS_CHUNK;
        t1 = t0 + PGL_RS_CHUNK;
        t0 = t0 < s.t_lo ? s.t_lo : t0;
    }
    const int len = (int)((s.t_hi < t1 ? s.t_hi : t1) - t0);
    double acc = 0.0, since = 0.0;
    pgl_bin_walk(
        s, j, t0, len, [](const double xv) { return pgl_lambda_only(xv, NLIN, PGL_C); },
        [&](int, const bool live, const double xv, const double lam, const bool event, int, const int ei) {
            if (CORR) {
                const double own = pgl_rw_lambda(xv, NLIN, PGL_C);         // no vote: the same bits in every range
                if (event) {
                    p.pre[ei] = since;
                    p.qev[ei] = own;
                }
                since = event ? 0.0 : since + (live ? own : 0.0);
            }
            acc += live ? lam : 0.0;
            if (!CORR && event) p.pre[ei] = acc;
        });
    p.tot[(size_t)c * s.xs + j] = acc;
    if (CORR) p.tail[(size_t)c * s.xs + j] = since;
}

template <int NLIN>
__global__ __launch_bounds__(256) void k_rescale_chunk(const RescaleParams p)
{
    pgl_rescale_chunk_body<NLIN, false>(p);
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

// one workgroup per neuron.  CORR: same chunk: the sum since the earlier event IS pre of the later one; else the tail of the
// earlier event's chunk, the chunks strictly between the two events total by total in chunk order (they hold no event:
// tail = total; a serial loop of the thread, one strided load per chunk -- about 2 300 for a neuron with two events at the
// ends of 600 000 bins, a few for any neuron that fires; cum serves the stats only), the later event's pre.  No difference
// of sums anywhere.  The later event's bin enters by pgl_gof_event_term at the uniform of (seed, draw, neuron, index of the
// event in the neuron's whole list).
template <bool CORR>
__device__ __forceinline__ void pgl_rescale_finish_body(const RescaleParams& p)
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
        const long long ca = CORR ? a.x / PGL_RS_CHUNK - p.c0 : (a.x - p.src.t_lo) / PGL_RS_CHUNK;
        const long long cb = CORR ? b.x / PGL_RS_CHUNK - p.c0 : (b.x - p.src.t_lo) / PGL_RS_CHUNK;
        const double pb = p.pre[i];
        double s;
        if (CORR) {
            s = pb;
            if (ca != cb) {
                s = p.tail[(size_t)ca * p.src.xs + n];
                for (long long c = ca + 1; c < cb; ++c) s += p.tail[(size_t)c * p.src.xs + n];
                s += pb;
            }
        } else if (ca == cb) {
            s = pb - p.pre[i - 1];
        } else {
            s = p.tot[(size_t)ca * p.src.xs + n] - p.pre[i - 1];
            if (cb > ca + 1) s += p.cum[(size_t)cb * p.src.xs + n] - p.cum[(size_t)(ca + 1) * p.src.xs + n];
            s += pb;
        }
        if (CORR) {
            const double u = pgl_gof_uniform(p.seed, (pgl_hmc_u64)p.draw, (pgl_hmc_u64)n, (pgl_hmc_u64)(i - p.src.wlo[n]));
            p.tau[o0 + (i - e0 - 1)] = pgl_gof_corrected(p.src.dt * s, p.src.dt * p.qev[i], u);
        } else {
            p.tau[o0 + (i - e0 - 1)] = p.src.dt * s;
        }
    }
    for (int o = 32; o > 0; o >>= 1) nm += __shfl_down(nm, o, 64);
    if ((threadIdx.x & 63) == 0) multi[threadIdx.x >> 6] = nm;
    __syncthreads();
    if (threadIdx.x == 0) {
        double* st = p.stats + (size_t)n * 4;
        st[0] = p.src.dt * (CORR ? p.lam_row[n] : p.cum[(size_t)p.nchunks * p.src.xs + n]);
        st[1] = (double)(e1 - e0);
        st[2] = (double)(multi[0] + multi[1] + multi[2] + multi[3]);
        st[3] = 0.0;
    }
}

__global__ __launch_bounds__(256) void k_rescale_finish(const RescaleParams p)
{
    pgl_rescale_finish_body<false>(p);
}
