// Batched spike-train simulation (pgl_simulate_batch): the integrate-and-fire thinning of pgl_simulate (population.py:233-389)
// for many independent replicates of one model, ONE WORKGROUP PER REPLICATE running the whole time loop.  Time is serial
// (a spike at t changes the currents of t + 1 ..), replicates are not: they are the parallel axis.
//   state across bins   acc, thr and the stream counter k of a neuron live in the registers of the thread that owns the
//                       neuron (thread n = neuron n, N <= 1024); the currents of the next R bins live in a ring of R x N
//                       doubles -- LDS when it fits (RING_LDS), else a per-replicate global workspace (which stays in
//                       L2 / MALL: 200 KiB per replicate at N = 128, R = 200).
//   ring                slot t % R holds X[t, :]: the bias + stimulus current X0[t, :] plus what the spikes so far added.  Bin
//                       t consumes its slot and refills it with X0[t + R, :] (X0 is read once per bin), so the currents
//                       are summed in the order pgl_simulate sums them: same spikes, same bits of X.
//   spike rounds        the decision of a round is workgroup-uniform: every wave ballots its spiking neurons (and the
//                       neurons at the cap) into LDS, one barrier, every thread reads all the masks.  No barrier sits in
//                       divergent code.  A spiking neuron's AW[n_pre, :, :] (read only then) is added to the ring by all
//                       threads, each thread owning the elements i = tid (mod blockDim) of the (tau, n) plane, spiking
//                       neurons in ascending n_pre: no atomics, a fixed order, the same bits from run to run.
//   thresholds          thr = -log(u(seed, replicate, neuron, k)), stateless (the formula: include/pyglm_hip.h).
// Every loop has a static bound: nT bins; at most 10 N + 1 rounds per bin (a round that is not the last increments S[t, n] of
// at least one neuron, and a count that reaches 10 ends the bin: the cap of population.py:345-349), N neurons per round, R N
// ring elements per neuron.  The kernel cannot spin.
// All arithmetic is f64 with the all-f64 rate function of the rescale kernels (pgl_lambda_only): a threshold comparison is
// a discontinuity, there is no single-precision exp shortcut here.
#pragma once

#define PGL_SIM_MAXN 1024                       // thread n owns neuron n
#define PGL_SIM_MAXW (PGL_SIM_MAXN / 64)
#define PGL_SIM_G 0x9e3779b97f4a7c15ULL
#define PGL_SIM_LDS_MAX (160 * 1024 - 1024)     // ring bytes that fit beside the ballot masks

struct SimParams {
    const double* X0;         // (nT, N) bias + stimulus current, shared by the replicates
    const double* AW;         // (N, R, N) [n_pre][tau][n_post]
    double* ws;               // (n_rep, R, N) rings of the global placement
    unsigned char* S;         // (n_rep, nT, N) out, may be null
    double* X;                // (n_rep, nT, N) out, may be null
    long long* counts;        // (n_rep, N) out
    long long* exc;           // (n_rep) out
    long long nT;
    int N, R, rep0;
    unsigned long long seed;
    double dt;
};

__host__ __device__ __forceinline__ unsigned long long pgl_sim_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
// the stream key of neuron n in replicate r, and its k-th uniform
__host__ __device__ __forceinline__ unsigned long long pgl_sim_key(unsigned long long seed, unsigned long long r, unsigned long long n)
{
    return pgl_sim_mix(pgl_sim_mix(pgl_sim_mix(seed + PGL_SIM_G) + PGL_SIM_G * (r + 1)) + PGL_SIM_G * (n + 1));
}
__host__ __device__ __forceinline__ double pgl_sim_uniform(unsigned long long key, unsigned long long k)
{
    const unsigned long long z = pgl_sim_mix(key + PGL_SIM_G * (k + 1));
    return ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

template <int NLIN, bool RING_LDS>
__global__ __launch_bounds__(PGL_SIM_MAXN) void k_simulate(const SimParams p)
{
    extern __shared__ double sim_ring[];
    __shared__ unsigned long long mask[2][2][PGL_SIM_MAXW];       // [parity][spiking | at the cap][wave]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, nthr = blockDim.x;
    const int N = p.N, R = p.R, RN = R * N;
    const long long nT = p.nT;
    const size_t rep = blockIdx.x;
    double* __restrict__ ring = RING_LDS ? sim_ring : p.ws + rep * (size_t)RN;
    const double* __restrict__ X0 = p.X0;
    for (int i = tid; i < RN; i += nthr) ring[i] = ((long long)i < nT * N) ? X0[i] : 0.0;
    const bool own = tid < N;
    const unsigned long long key = pgl_sim_key(p.seed, (unsigned long long)p.rep0 + rep, (unsigned long long)tid);
    unsigned long long k = 1;
    double acc = 0.0, thr = -pgl_log(pgl_sim_uniform(key, 0), PGL_C);
    long long count = 0, nexc = 0;
    int slot = 0, par = 0;
    __syncthreads();
    for (long long t = 0; t < nT; ++t) {
        const int so = slot * N;
        double x = 0.0;
        if (own) {
            x = ring[so + tid];
            if (p.X) p.X[(rep * nT + t) * N + tid] = x;
            ring[so + tid] = (t + R < nT) ? X0[(size_t)(t + R) * N + tid] : 0.0;
        }
        // (every lane evaluates the rate, lanes without a neuron at x = 0: pgl_lambda_only picks its series by a vote of the wave)
        const double lam = pgl_lambda_only(x, NLIN, PGL_C);
        acc += lam * p.dt;
        bool spk = own && acc > thr;
        int sb = spk ? 1 : 0;
        const int nel = (int)((nT - t - 1 < R) ? nT - t - 1 : R) * N;      // population.py:326: the end truncates the impulse
        int base = so + N;                                                 // ring position of (t + 1, neuron 0)
        if (base >= RN) base -= RN;
        for (int round = 0; round <= 10 * N; ++round) {
            const unsigned long long ms = __ballot(spk), mc = __ballot(sb >= 10);
            if (lane == 0) {
                mask[par][0][wave] = ms;
                mask[par][1][wave] = mc;
            }
            __syncthreads();
            const unsigned long long* mk = mask[par][0];
            const unsigned long long* mcap = mask[par][1];
            par ^= 1;
            unsigned long long any = 0, cap = 0;
            for (int w = 0; w < nw; ++w) {
                any |= mk[w];
                cap |= mcap[w];
            }
            // (the same value in every lane of every wave; through an SGPR, so that the branches around the barrier are scalar)
            const int flag = __builtin_amdgcn_readfirstlane((any != 0 ? 1 : 0) | (cap != 0 ? 2 : 0));
            if ((flag & 1) == 0) break;
            if (flag & 2) {                                                // population.py:345-349: the round is dropped
                ++nexc;
                break;
            }
            for (int w = 0; w < nw; ++w) {                                 // population.py:351-353, ascending n_pre
                const unsigned long long m = mk[w];
                unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m);
                unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
                for (int half = 0; half < 2; ++half) {
                    unsigned bits = half ? hi : lo;
                    while (bits) {
                        const int npre = w * 64 + half * 32 + __builtin_ctz(bits);
                        bits &= bits - 1;
                        const double* __restrict__ aw = p.AW + (size_t)npre * RN;
                        for (int i = tid; i < nel; i += nthr) {
                            int q = base + i;
                            if (q >= RN) q -= RN;
                            ring[q] += aw[i];
                        }
                    }
                }
            }
            if (spk) {                                                     // population.py:355-360
                acc -= thr;
                thr = -pgl_log(pgl_sim_uniform(key, k), PGL_C);
                ++k;
            }
            acc = (acc < 0.0) ? 0.0 : acc;
            spk = own && acc > thr;
            sb += spk ? 1 : 0;
        }
        if (own && p.S) p.S[(rep * nT + t) * N + tid] = (unsigned char)sb;
        count += sb;
        if (++slot == R) slot = 0;
    }
    if (own) p.counts[rep * N + tid] = count;
    if (tid == 0) p.exc[rep] = nexc;
}
