"""Expected counts over time windows of posterior draws on the device (pgl_rate_windows_dev, inference/predictive.py:
rate_bands) at C2 (N = 32, nT = 300 000) and C3 (N = 128, nT = 600 000), S = 100 draws, win = 50 bins.  No figure is a pass /
fail gate.

  (a) wall time per queued pgl_rate_windows_dev call (device pointers, accumulator on, no synchronisation between the calls; a
      host clock around a window of --window-ms that ends in a stream synchronisation, three windows), and per draw of
      rate_bands;
  (b) the two new launches alone: their kernel times from a kernel trace, the bandwidth k_rw_piece reaches on its one read of
      the currents GX, and the ratio to k_pw_chunk at the same configuration (profiles/waic_bench.json);
  (c) the route the library had before: per draw N x pgl_state (three (nT) host arrays each, as Population.eval_state does it)
      plus the window sums in numpy, timed on 3 draws in the same process, and the largest difference of the two routes.

Kernel times come from rocprofv3 in runs of their own, one per configuration, of this script's --trace-loop mode (set-up,
then nothing but queued pgl_rate_windows_dev calls), summarised by tools/rocprof_summary.py:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rate_bench.py --trace-loop --configs C3
    python tools/rocprof_summary.py stats DIR/.../*results.db profiles/rate_bench_kernel_stats_C3.csv
    python tools/rate_bench.py --kernel-stats C2=profiles/rate_bench_kernel_stats_C2.csv,C3=... --out profiles/rate_bench.json

Without --kernel-stats the figures that need kernel times are left out.  Prints one JSON line."""
import argparse, csv, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import predictive as PP
from theano_pyglm_amd.models.model_factory import make_model
from theano_pyglm_amd.population import Population

WIN = 50
SHAPES = {'C2': (32, 300000), 'C3': (128, 600000)}


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
    nw = d.rate_windows_count(WIN)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    d_th, d_W = t(theta), t(Weff)
    d_lam = torch.empty((nw, N), dtype=torch.float64, device='cuda')
    d_acc = torch.empty((_lib.RW_NACC, nw, N), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    d.rate_windows_dev(d_th.data_ptr(), d_W.data_ptr(), WIN, d_lam.data_ptr(), 0, d_acc.data_ptr(), 0)
    d.sync()
    call = lambda: d.rate_windows_dev(d_th.data_ptr(), d_W.data_ptr(), WIN, 0, 0, d_acc.data_ptr(), 1)
    return popn, x, S, theta, Weff, d, nw, rng, t, (d_th, d_W, d_lam, d_acc), call


def trace_loop(name, N, nT, calls):
    """what the kernel trace is taken of: queued pgl_rate_windows_dev calls and nothing else after the set-up"""
    popn, x, S, theta, Weff, d, nw, rng, t, keep, call = setup(N, nT)
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


def run(name, N, nT, n_draws, window_ms, stats, traced, waic):
    popn, x, S, theta, Weff, d, nw, rng, t, (d_th, d_W, d_lam, d_acc), call = setup(N, nT)
    dt = 0.001
    P = theta.shape[1]
    draws = theta[None] + 0.01 * rng.standard_normal((n_draws, N, P))
    out = {'config': name, 'N': N, 'nT': nT, 'P': P, 'nlin': popn.glm.nlin_model.kind, 'draws': n_draws, 'win': WIN, 'n_win': nw}
    # (a) the whole route, warmed by one short run, twice
    PP.rate_bands(popn, x, draws[:3], win=WIN)
    per_draw = []
    for _ in range(2):
        t0 = time.perf_counter()
        r = PP.rate_bands(popn, x, draws, win=WIN)
        per_draw.append((time.perf_counter() - t0) / n_draws * 1e3)
    out['rate_bands_ms_per_draw'] = per_draw
    out['max_abs_pearson'] = float(np.nanmax(np.abs(r['pearson'])))
    out['pit_ks_median'] = float(np.median(r['pit_ks']))
    out['pit_nan'] = int(np.sum(r['n_pit_nan']))

    def timed(calls):
        d.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        d.sync()
        return (time.perf_counter() - t0) / calls * 1e3

    calls = max(20, int(np.ceil(window_ms / timed(20))))      # (the pilot is the warm-up)
    out['calls_per_window'] = calls
    out['rate_windows_dev_ms'] = [timed(calls) for _ in range(3)]
    d.set_option(_lib.OPT_RECORD_KERNELS, 1)
    call()
    d.sync()
    names = d.last_kernels()
    d.set_option(_lib.OPT_RECORD_KERNELS, 0)
    out['kernels_of_a_call'] = names
    out['gx_bytes'] = float(nT) * 16 * ((N + 15) // 16) * 8
    if stats is not None:
        per_call = dict((k, tot / traced * 1e-3) for k, (n, tot) in kernel_times(stats).items() if n >= traced)
        is_named = lambda k, n: k == n or k.startswith(n + '(') or k.startswith('void ' + n + '(')
        pick = lambda n: [k for k in per_call if is_named(k, n)]
        piece, window = pick(names[-2]), pick(names[-1])
        out['kernel_trace_ms_per_call'] = per_call
        if len(piece) != 1 or len(window) != 1 or any(not pick(n) for n in names[:-2]):
            out['kernel_trace_error'] = "the kernels of a call are not rows of %s" % stats
        else:
            copies = [k for k in per_call if 'copyBuffer' in k]
            forward = [k for k in per_call if k not in piece + window + copies]
            fw = sum(per_call[k] for k in forward)
            out['traced_calls'] = traced
            out['forward_kernels_ms'] = fw
            out['rw_piece_kernel_ms'] = per_call[piece[0]]
            out['rw_window_kernel_ms'] = per_call[window[0]]
            out['rw_kernels_ms'] = out['rw_piece_kernel_ms'] + out['rw_window_kernel_ms']
            out['rw_piece_gx_read_gbps'] = out['gx_bytes'] / out['rw_piece_kernel_ms'] * 1e-6
            out['rw_kernels_over_forward_kernels'] = out['rw_kernels_ms'] / fw
            out['rate_windows_dev_over_forward_kernels'] = min(out['rate_windows_dev_ms']) / fw
            if waic and name in waic and 'pw_chunk_kernel_ms' in waic[name]:
                out['pw_chunk_kernel_ms_of_waic_bench'] = waic[name]['pw_chunk_kernel_ms']
                out['rw_piece_over_pw_chunk'] = out['rw_piece_kernel_ms'] / waic[name]['pw_chunk_kernel_ms']
    # (c) the route this replaces, on 3 draws: N x pgl_state per draw and the window sums in numpy
    dev = []
    for i in range(3):
        d.rate_windows_dev(t(draws[i]).data_ptr(), d_W.data_ptr(), WIN, d_lam.data_ptr())
        d.sync()
        dev.append(d_lam.cpu().numpy().copy())
    starts = np.arange(0, nT, WIN)
    t0 = time.perf_counter()
    host = []
    for i in range(3):
        lam = np.empty((nT, N))
        for n in range(N):
            lam[:, n] = d.state(n, draws[i][n], Weff[:, n])[0]
        host.append(dt * np.add.reduceat(lam, starts, axis=0))
    out['state_numpy_ms_per_draw'] = (time.perf_counter() - t0) / 3 * 1e3
    out['pcie_bytes_per_draw_of_that_route'] = 3.0 * nT * N * 8
    out['max_rel_difference_of_the_two_routes'] = float(max(np.max(np.abs(a - b) / np.abs(b)) for a, b in zip(dev, host)))
    out['speedup'] = out['state_numpy_ms_per_draw'] / min(per_draw)
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--draws', type=int, default=100)
    ap.add_argument('--window-ms', type=float, default=500.0, help='length of a timed window of queued calls')
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--kernel-stats', default=None, metavar='C2=CSV,C3=CSV',
                    help='tools/rocprof_summary.py stats files of --trace-loop runs under rocprofv3 --kernel-trace --stats')
    ap.add_argument('--trace-loop', action='store_true', help='set-up, then --calls queued pgl_rate_windows_dev calls (to be traced)')
    ap.add_argument('--calls', type=int, default=300, help='calls of --trace-loop (the same value when its trace is read with --kernel-stats)')
    ap.add_argument('--waic-json', default=os.path.join(ROOT, 'profiles', 'waic_bench.json'),
                    help='profiles/waic_bench.json: the k_pw_chunk kernel times the new piece kernel is set beside')
    ap.add_argument('--scale', type=float, default=1.0, help='dev: shrink nT (a rehearsal, not a measurement)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("rate_bench: no GPU visible; nothing is measured without one")
    stats = dict(kv.split('=', 1) for kv in a.kernel_stats.split(',')) if a.kernel_stats else {}
    waic = None
    if a.waic_json and os.path.exists(a.waic_json):
        with open(a.waic_json) as f:
            waic = json.load(f)
    res = {'bench': 'rate_trace_loop' if a.trace_loop else 'rate'}
    for k in a.configs.split(','):
        N, nT = SHAPES[k]
        nT = int(nT * a.scale)
        res[k] = trace_loop(k, N, nT, a.calls) if a.trace_loop else run(k, N, nT, a.draws, a.window_ms, stats.get(k), a.calls + 2, waic)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
