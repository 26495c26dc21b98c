"""PSIS-LOO on the device (inference/model_compare.py: loo_glms over pgl_psis_loo_dev) at C2 (N = 32, nT = 300 000) and C3
(N = 128, nT = 600 000), S = 1000 draws jittered around one parameter point (theta + 0.01 z: NOT a fitted posterior -- the
khat figures below describe this jitter).  No figure is a pass / fail bar.  Per configuration:
  (a) pgl_psis_loo_dev on the resident matrix ll (S, n_blocks, N): wall time per call of queued calls with one
      synchronisation inside the clock, three windows (the spread); and, from a kernel trace taken in a run of its own
      (nothing else is collected in that run), the time of k_psis_column per call;
  (b) psis_loo_from_pointwise (numpy) on the same matrix in the same process, and the device-to-host copy of the matrix,
      timed separately;
  (c) one whole loo_glms call and the share of it that (a) is;
  (d) what the numbers mean: the distribution of khat over blocks, neurons flagged by n_khat_bad and by WAIC's n_high_var.
The kernel time comes from
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/loo_bench.py --trace-loop --configs C3
    python tools/rocprof_summary.py stats DIR/.../*results.db profiles/loo_bench_kernel_stats_C3.csv
    python tools/loo_bench.py --kernel-stats C2=...,C3=... --out profiles/loo_bench.json
Without --kernel-stats the kernel time is left out.  Prints one JSON line."""
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


def setup(N, nT, n_draws):
    """the population, a parameter point, the draws and their matrix ll (S, n_blocks, N) resident on the device"""
    import torch
    rng = np.random.default_rng(1234)
    dt = 0.001
    popn = Population(make_model('standard_glm', N=N, dt=dt))
    S = np.minimum(rng.poisson(20.0 * dt, size=(nT, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': dt, 'T': nT * dt, 'stim': None, 'dt_stim': 0.1})
    x = popn.sample(np.random.RandomState(7))
    theta = popn.theta_matrix(x)
    draws = theta[None] + 0.01 * rng.standard_normal((n_draws,) + theta.shape)
    d = popn._handle(popn.data_sequences[0])
    nb = d.pointwise_count(BLOCK_CHUNKS)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    d_W, d_draws = t(popn.W_eff(x)), t(draws)
    d_ll = torch.empty((n_draws, nb, N), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    for i in range(n_draws):
        d.pointwise_dev(d_draws[i].data_ptr(), d_W.data_ptr(), BLOCK_CHUNKS, d_ll[i].data_ptr())
    d.sync()
    d_out = torch.empty((4, nb, N), dtype=torch.float64, device='cuda')
    call = lambda: d.psis_loo(d_ll, out=d_out)
    return popn, x, draws, d, nb, d_ll, d_out, call


def trace_loop(name, N, nT, n_draws, calls):
    """what the kernel trace is taken of: the set-up, then queued pgl_psis_loo_dev calls and nothing else"""
    popn, x, draws, d, nb, d_ll, d_out, call = setup(N, nT, n_draws)
    for _ in range(calls):
        call()
    d.sync()
    popn.release_data()
    return {'config': name, 'calls': calls}


def kernel_times(path):
    with open(path) as f:
        rows = list(csv.reader(ln for ln in f if not ln.startswith('#')))
    return dict((r[0], (int(r[1]), float(r[2]))) for r in rows[1:])


def run(name, N, nT, n_draws, window_ms, stats):
    import torch
    popn, x, draws, d, nb, d_ll, d_out, call = setup(N, nT, n_draws)
    out = {'config': name, 'N': N, 'nT': nT, 'draws': n_draws, 'block_chunks': BLOCK_CHUNKS, 'n_blocks': nb, 'columns': nb * N,
           'matrix_bytes': float(n_draws) * nb * N * 8, 'draws_are': 'theta + 0.01 z around one parameter point, not a fit'}

    def timed(calls):
        d.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        d.sync()
        return (time.perf_counter() - t0) / calls * 1e3

    calls = max(20, int(np.ceil(window_ms / timed(20))))      # (the pilot is the warm-up)
    out['calls_per_window'] = calls
    out['psis_loo_dev_ms'] = [timed(calls) for _ in range(3)]
    if stats is not None:
        rows = [(k, v) for k, v in kernel_times(stats).items() if 'k_psis_column' in k]
        if len(rows) == 1:
            out['k_psis_column_kernel_ms'] = rows[0][1][1] / rows[0][1][0] * 1e-3
            out['k_psis_column_traced_dispatches'] = rows[0][1][0]
        else:
            out['kernel_trace_error'] = "k_psis_column is not one row of %s" % stats
    dev = d_out.cpu().numpy().copy()
    # (b) the host route on the same matrix
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ll = d_ll.cpu().numpy()
    out['matrix_copy_ms'] = (time.perf_counter() - t0) * 1e3
    cols = min(nb * N, 512)                                     # numpy on a sample of the columns, scaled to all of them
    flat = ll.reshape(n_draws, -1)
    pick = np.linspace(0, nb * N - 1, cols).astype(int)
    t0 = time.perf_counter()
    host = MC.psis_loo_from_pointwise(flat[:, pick])
    out['numpy_ms_per_column'] = (time.perf_counter() - t0) / cols * 1e3
    out['numpy_columns_timed'] = cols
    out['numpy_ms_all_columns_extrapolated'] = out['numpy_ms_per_column'] * nb * N
    devp = dev.reshape(4, -1)[:, pick]
    with np.errstate(invalid='ignore'):
        out['max_abs_khat_difference_device_numpy'] = float(np.nanmax(np.abs(np.where(np.isfinite(host[1]), devp[1] - host[1], 0.0))))
        out['max_rel_elpd_difference_device_numpy'] = float(np.nanmax(np.abs(devp[0] - host[0]) / np.maximum(1.0, np.abs(host[0]))))
    out['speedup_over_numpy_and_copy'] = (out['numpy_ms_all_columns_extrapolated'] + out['matrix_copy_ms']) / min(out['psis_loo_dev_ms'])
    # (c) the whole call
    MC.loo_glms(popn, x, draws[:3], BLOCK_CHUNKS)
    t0 = time.perf_counter()
    res = MC.loo_glms(popn, x, draws, BLOCK_CHUNKS)
    out['loo_glms_ms'] = (time.perf_counter() - t0) * 1e3
    out['psis_share_of_loo_glms'] = min(out['psis_loo_dev_ms']) / out['loo_glms_ms']
    out['route'] = res['route']
    # (d) what it means
    wa = MC.waic_glms(popn, x, draws, BLOCK_CHUNKS)
    kh = res['khat_b']
    out['khat_quantiles_0_25_50_75_100'] = [float(q) for q in np.quantile(kh[np.isfinite(kh)], [0, 0.25, 0.5, 0.75, 1.0])]
    out['khat_threshold'] = res['khat_threshold']
    out['blocks_above_khat_threshold'] = int(np.sum(res['n_khat_bad']))
    out['blocks_above_waic_variance_warning'] = int(np.sum(wa['n_high_var']))
    out['neurons_flagged_by_khat'] = int(np.sum(res['n_khat_bad'] > 0))
    out['neurons_flagged_by_waic_variance'] = int(np.sum(wa['n_high_var'] > 0))
    out['elpd_loo_total'] = float(np.sum(res['elpd_loo']))
    out['elpd_waic_total'] = float(np.sum(wa['elpd_waic']))
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--draws', type=int, default=1000)
    ap.add_argument('--window-ms', type=float, default=500.0, help='length of a timed window of queued calls')
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--kernel-stats', default=None, metavar='C2=CSV,C3=CSV',
                    help='tools/rocprof_summary.py stats files of --trace-loop runs under rocprofv3 --kernel-trace --stats')
    ap.add_argument('--trace-loop', action='store_true', help='set-up, then --calls queued pgl_psis_loo_dev calls (to be traced)')
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--scale', type=float, default=1.0, help='dev: shrink nT (a rehearsal, not a measurement)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("loo_bench: no GPU visible; nothing is measured without one")
    stats = dict(kv.split('=', 1) for kv in a.kernel_stats.split(',')) if a.kernel_stats else {}
    res = {'bench': 'loo_trace_loop' if a.trace_loop else 'loo'}
    for k in a.configs.split(','):
        N, nT = SHAPES[k]
        nT = int(nT * a.scale)
        res[k] = trace_loop(k, N, nT, a.draws, a.calls) if a.trace_loop else run(k, N, nT, a.draws, a.window_ms, stats.get(k))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")
