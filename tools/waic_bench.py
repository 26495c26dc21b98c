"""The pointwise log-likelihood of posterior draws on the device (inference/model_compare.py: pointwise_ll_draws over
pgl_pointwise_dev) at C2 (N = 32, nT = 300 000) and C3 (N = 128, nT = 600 000), S = 100 draws.  No figure is a pass / fail
gate.

  (a) wall time per draw of pointwise_ll_draws (upload of the draws, S x (row copy + forward launches + k_pw_chunk +
      k_pw_block), one synchronisation, the accumulator back) and of queued pgl_pointwise_dev calls (device pointers, no
      synchronisation between them; a host clock around a window of --window-ms that ends in a stream synchronisation),
      against the floor: the kernel time of the forward launches of one call, from a kernel trace;
  (b) the two new launches alone: their kernel times from the same trace, and the bandwidth k_pw_chunk reaches on its one
      read of the currents GX;
  (c) the route the library had before: forward pass + N x pgl_gibbs_currents ((nT) doubles over PCIe each) + the rate, the
      terms and the block sums in numpy, timed on 3 draws, and the largest difference of the two routes.

Kernel times come from rocprofv3 in runs of their own, one per configuration, of this script's --trace-loop mode (set-up,
then nothing but queued pgl_pointwise_dev calls), summarised by tools/rocprof_summary.py:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/waic_bench.py --trace-loop --configs C3
    python tools/rocprof_summary.py stats DIR/.../*results.db profiles/waic_bench_kernel_stats_C3.csv
    python tools/waic_bench.py --kernel-stats C2=profiles/waic_bench_kernel_stats_C2.csv,C3=... --out profiles/waic_bench.json

pgl_gibbs_prepare_all itself is no floor for queued calls: it takes host arrays, uploads them and synchronises the stream
on every call.  Without --kernel-stats the figures that need kernel times are left out.  Prints one JSON line."""
import argparse, csv, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import model_compare as MC
from theano_pyglm_amd.models.model_factory import make_model
from theano_pyglm_amd.population import Population

BLOCK_CHUNKS = 40
SHAPES = {'C2': (32, 300000), 'C3': (128, 600000)}


def host_blocks(x, S, kind, dt, bc):
    """block sums of -dt lam + S log lam over blocks of 256 bc bins, float64 numpy"""
    if kind == 'exp':
        lam, loglam = np.exp(x), x
    else:
        lam = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
        loglam = np.log(lam)
    term = -dt * lam + np.where(S > 0, S * np.where(S > 0, loglam, 0.0), 0.0)
    return np.add.reduceat(term, np.arange(0, term.shape[0], 256 * bc), axis=0)


def kernel_times(path):
    """{kernel name: (dispatches, total us)} of a tools/rocprof_summary.py stats file"""
    with open(path) as f:
        rows = list(csv.reader(ln for ln in f if not ln.startswith('#')))
    return dict((r[0], (int(r[1]), float(r[2]))) for r in rows[1:])


def setup(N, nT):
    import torch
    rng = np.random.default_rng(1234)
    dt = 0.001
    popn = Population(make_model('standard_glm', N=N, dt=dt))
    S = np.minimum(rng.poisson(20.0 * dt, size=(nT, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': dt, 'T': nT * dt, 'stim': None, 'dt_stim': 0.1})
    x = popn.sample(np.random.RandomState(7))
    theta, Weff = popn.theta_matrix(x), popn.W_eff(x)
    d = popn._handle(popn.data_sequences[0])
    nb = d.pointwise_count(BLOCK_CHUNKS)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    d_th, d_W = t(theta), t(Weff)
    d_ll = torch.empty((nb, N), dtype=torch.float64, device='cuda')
    d_acc = torch.empty((4, nb, N), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    d.pointwise_dev(d_th.data_ptr(), d_W.data_ptr(), BLOCK_CHUNKS, d_ll.data_ptr(), d_acc.data_ptr(), 0)
    d.sync()
    call = lambda: d.pointwise_dev(d_th.data_ptr(), d_W.data_ptr(), BLOCK_CHUNKS, d_ll.data_ptr(), d_acc.data_ptr(), 1)
    return popn, x, S, theta, Weff, d, nb, rng, t, (d_th, d_W, d_ll, d_acc), call


def trace_loop(name, N, nT, calls):
    """what the kernel trace is taken of: queued pgl_pointwise_dev calls and nothing else after the set-up"""
    popn, x, S, theta, Weff, d, nb, rng, t, keep, call = setup(N, nT)
    d.set_option(_lib.OPT_RECORD_KERNELS, 1)
    call()
    d.sync()
    names = d.last_kernels()
    d.set_option(_lib.OPT_RECORD_KERNELS, 0)
    for _ in range(calls):
        call()
    d.sync()
    popn.release_data()
    return {'config': name, 'calls': calls + 2, 'kernels_of_a_call': names}


def run(name, N, nT, n_draws, window_ms, stats, traced):
    popn, x, S, theta, Weff, d, nb, rng, t, (d_th, d_W, d_ll, d_acc), call = setup(N, nT)
    dt = 0.001
    P = theta.shape[1]
    kind = popn.glm.nlin_model.kind
    draws = theta[None] + 0.01 * rng.standard_normal((n_draws, N, P))
    out = {'config': name, 'N': N, 'nT': nT, 'P': P, 'nlin': kind, 'draws': n_draws, 'block_chunks': BLOCK_CHUNKS,
           'block_bins': 256 * BLOCK_CHUNKS, 'n_blocks': nb}
    # (a) the whole route, warmed by one short run, twice
    MC.pointwise_ll_draws(popn, x, draws[:3], BLOCK_CHUNKS)
    per_draw = []
    for _ in range(2):
        t0 = time.perf_counter()
        r = MC.pointwise_ll_draws(popn, x, draws, BLOCK_CHUNKS)
        per_draw.append((time.perf_counter() - t0) / n_draws * 1e3)
    out['pointwise_ll_draws_ms_per_draw'] = per_draw
    res = MC.waic_from_accumulators(r['acc'], n_draws)
    out['elpd_waic_total'] = float(np.sum(res['elpd_waic']))
    out['p_waic_total'] = float(np.sum(res['p_waic']))
    out['blocks_above_variance_warning'] = int(np.sum(res['n_high_var']))

    def timed(calls):
        d.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        d.sync()
        return (time.perf_counter() - t0) / calls * 1e3

    calls = max(20, int(np.ceil(window_ms / timed(20))))      # (the pilot is the warm-up)
    out['calls_per_window'] = calls
    out['pointwise_dev_ms'] = [timed(calls) for _ in range(3)]
    d.set_option(_lib.OPT_RECORD_KERNELS, 1)
    call()
    d.sync()
    names = d.last_kernels()
    d.set_option(_lib.OPT_RECORD_KERNELS, 0)
    out['kernels_of_a_call'] = names
    out['gx_bytes'] = float(nT) * 16 * ((N + 15) // 16) * 8
    if stats is not None:
        # the kernels of a call: every row of the trace with at least one dispatch per traced call (the set-up launches nothing
        # that often); mean time per call = total / traced calls
        per_call = dict((k, tot / traced * 1e-3) for k, (n, tot) in kernel_times(stats).items() if n >= traced)
        is_named = lambda k, n: k == n or k.startswith(n + '(') or k.startswith('void ' + n + '(')
        pick = lambda n: [k for k in per_call if is_named(k, n)]
        chunk, block = pick(names[-2]), pick(names[-1])
        out['kernel_trace_ms_per_call'] = per_call
        if len(chunk) != 1 or len(block) != 1 or any(not pick(n) for n in names[:-2]):
            out['kernel_trace_error'] = "the kernels of a call are not rows of %s" % stats
        else:
            copies = [k for k in per_call if 'copyBuffer' in k]
            forward = [k for k in per_call if k not in chunk + block + copies]
            out['traced_calls'] = traced
            fw = sum(per_call[k] for k in forward)
            out['forward_kernels_ms'] = fw
            out['copy_kernels_ms'] = sum(per_call[k] for k in copies)
            out['pw_chunk_kernel_ms'] = per_call[chunk[0]]
            out['pw_block_kernel_ms'] = per_call[block[0]]
            out['pw_kernels_ms'] = out['pw_chunk_kernel_ms'] + out['pw_block_kernel_ms']
            out['pw_chunk_gx_read_gbps'] = out['gx_bytes'] / out['pw_chunk_kernel_ms'] * 1e-6
            out['pw_kernels_over_forward_kernels'] = out['pw_kernels_ms'] / fw
            out['pointwise_dev_over_forward_kernels'] = min(out['pointwise_dev_ms']) / fw
            out['draw_over_forward_kernels'] = min(per_draw) / fw
            # what a queued call spends outside its kernels: the gaps between launches
            out['pointwise_dev_outside_kernels_ms'] = min(out['pointwise_dev_ms']) - fw - out['pw_kernels_ms'] - out['copy_kernels_ms']
    # (c) the route of the parent commit, on 3 draws
    dev_ll = []
    for i in range(3):
        d.pointwise_dev(t(draws[i]).data_ptr(), d_W.data_ptr(), BLOCK_CHUNKS, d_ll.data_ptr())
        d.sync()
        dev_ll.append(d_ll.cpu().numpy().copy())
    t0 = time.perf_counter()
    host_ll = []
    for i in range(3):
        d.gibbs_prepare_all(draws[i], Weff)
        xcur = np.empty((nT, N))
        for n in range(N):
            xcur[:, n] = d.gibbs_currents(n) + draws[i][n, 0]
        host_ll.append(host_blocks(xcur, S, kind, dt, BLOCK_CHUNKS))
    out['currents_numpy_ms_per_draw'] = (time.perf_counter() - t0) / 3 * 1e3
    out['pcie_bytes_per_draw_of_that_route'] = float(nT) * N * 8
    out['max_rel_difference_of_the_two_routes'] = float(max(np.max(np.abs(a - b) / np.abs(b)) for a, b in zip(dev_ll, host_ll)))
    out['speedup'] = out['currents_numpy_ms_per_draw'] / min(per_draw)
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--draws', type=int, default=100)
    ap.add_argument('--window-ms', type=float, default=500.0, help='length of a timed window of queued calls')
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--kernel-stats', default=None, metavar='C2=CSV,C3=CSV',
                    help='tools/rocprof_summary.py stats files of --trace-loop runs under rocprofv3 --kernel-trace --stats')
    ap.add_argument('--trace-loop', action='store_true', help='set-up, then --calls queued pgl_pointwise_dev calls (to be traced)')
    ap.add_argument('--calls', type=int, default=300, help='calls of --trace-loop (the same value when its trace is read with --kernel-stats)')
    ap.add_argument('--scale', type=float, default=1.0, help='dev: shrink nT (a rehearsal, not a measurement)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("waic_bench: no GPU visible; nothing is measured without one")
    stats = dict(kv.split('=', 1) for kv in a.kernel_stats.split(',')) if a.kernel_stats else {}
    res = {'bench': 'waic_trace_loop' if a.trace_loop else 'waic'}
    for k in a.configs.split(','):
        N, nT = SHAPES[k]
        nT = int(nT * a.scale)
        res[k] = trace_loop(k, N, nT, a.calls) if a.trace_loop else run(k, N, nT, a.draws, a.window_ms, stats.get(k), a.calls + 2)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
