"""Convergence diagnostics on the device (DeviceGlm.chain_diag over pgl_chain_diag_dev) on the samplers' tensor (n, C, K) at
the column counts of C2 (32 neurons x 161 parameters) and C3 (128 x 641), for C = 4 chains of n = 1000 draws and for one chain
of 200.  The draws are SYNTHETIC: independent AR(1) series (rho = 0.5, unit variance) generated on the device, not the output
of a sampler -- the figures time the summary, they say nothing about a posterior.  No figure is a pass / fail bar.  Per
configuration and chain shape:
  (a) pgl_chain_diag_dev on the resident tensor: wall time per call of queued calls with one synchronisation inside the
      clock, three windows (the spread); and, from a kernel trace taken in a run of its own (nothing else is collected in that
      run), the time of k_diag_column per call;
  (b) the device-to-host copy of the tensor;
  (c) batched_hmc.summarize(..., chains=True) -- the summary before this kernel -- on a timed subset of the columns, scaled to
      all of them;
  (d) diagnostics.chain_diagnostics (numpy) timed the same way, and its largest difference from the device on that subset.
The kernel time comes from
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/diag_bench.py --trace-loop --configs C3 --chains 4x1000
    python tools/rocprof_summary.py stats DIR/.../*results.db profiles/diag_bench_kernel_stats_C3_4x1000.csv
    python tools/diag_bench.py --kernel-stats C3_4x1000=...,... --out profiles/diag_bench.json
Without --kernel-stats the kernel time is left out.  Prints one JSON line."""
import argparse, csv, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import diagnostics as D
from theano_pyglm_amd.inference.batched_hmc import summarize

SHAPES = {'C2': (32, 161), 'C3': (128, 641)}
RHO = 0.5


def setup(M, P, C, n):
    """a handle (it supplies the stream only) and the synthetic draws (n, C * M, P) resident on the device"""
    import torch
    d = _lib.DeviceGlm(4, 100, 5, 200, 'explinear', 0.001)
    g = torch.Generator(device='cuda')
    g.manual_seed(1234)
    x = torch.empty((n, C * M, P), dtype=torch.float64, device='cuda')
    x[0] = torch.randn((C * M, P), dtype=torch.float64, device='cuda', generator=g)
    for i in range(1, n):
        x[i] = RHO * x[i - 1] + np.sqrt(1.0 - RHO * RHO) * torch.randn((C * M, P), dtype=torch.float64, device='cuda', generator=g)
    out = torch.empty((_lib.DIAG_NOUT, M, P), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    return d, x, out, (lambda: d.chain_diag(x, n_chains=C, out=out))


def trace_loop(M, P, C, n, calls):
    """what the kernel trace is taken of: the set-up, then queued pgl_chain_diag_dev calls and nothing else"""
    d, x, out, call = setup(M, P, C, n)
    for _ in range(calls):
        call()
    d.sync()
    d.close()
    return {'calls': calls}


def kernel_times(path):
    with open(path) as f:
        rows = list(csv.reader(ln for ln in f if not ln.startswith('#')))
    return dict((r[0], (int(r[1]), float(r[2]))) for r in rows[1:])


def run(M, P, C, n, window_ms, stats, subset):
    import torch
    d, x, out_d, call = setup(M, P, C, n)
    K = M * P
    out = {'neurons': M, 'parameters': P, 'columns': K, 'chains': C, 'draws_per_chain': n, 'tensor_bytes': float(n) * C * K * 8,
           'draws_are': 'synthetic AR(1), rho = %.1f, generated on the device; not a sampler\'s output' % RHO}

    def timed(calls):
        d.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        d.sync()
        return (time.perf_counter() - t0) / calls * 1e3

    calls = max(2, int(np.ceil(window_ms / timed(2))))           # (the pilot is the warm-up)
    out['calls_per_window'] = calls
    out['chain_diag_dev_ms'] = [timed(calls) for _ in range(3)]
    if stats is not None:
        rows = [(k, v) for k, v in kernel_times(stats).items() if 'k_diag_column' in k]
        if len(rows) == 1:
            out['k_diag_column_kernel_ms'] = rows[0][1][1] / rows[0][1][0] * 1e-3
            out['k_diag_column_traced_dispatches'] = rows[0][1][0]
        else:
            out['kernel_trace_error'] = "k_diag_column is not one row of %s" % stats
    dev = out_d.cpu().numpy().reshape(_lib.DIAG_NOUT, K).copy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = x.cpu().numpy()
    out['tensor_copy_ms'] = (time.perf_counter() - t0) * 1e3
    cols = min(K, subset)
    pick = np.linspace(0, K - 1, cols).astype(int)
    sub = np.ascontiguousarray(host.reshape(n, C, K)[:, :, pick].transpose(1, 0, 2))       # (C, n, cols)
    t0 = time.perf_counter()
    summarize(sub, chains=True) if C > 1 else summarize(sub[0])
    out['summarize_ms_per_column'] = (time.perf_counter() - t0) / cols * 1e3
    out['summarize_ms_all_columns_extrapolated'] = out['summarize_ms_per_column'] * K
    t0 = time.perf_counter()
    ref = D.chain_diagnostics(sub)
    out['numpy_ms_per_column'] = (time.perf_counter() - t0) / cols * 1e3
    out['numpy_ms_all_columns_extrapolated'] = out['numpy_ms_per_column'] * K
    out['host_columns_timed'] = cols
    for k in ('rhat', 'ess_bulk', 'ess_tail', 'mcse_mean'):
        a, b = dev[_lib.DIAG_ROWS.index(k), pick], ref[k]
        out['max_rel_difference_device_numpy_' + k] = float(np.max(np.abs(a - b) / np.abs(b)))
    out['lags_equal_device_numpy'] = bool(all(np.array_equal(dev[_lib.DIAG_ROWS.index(k), pick], ref[k]) for k in _lib.DIAG_ROWS[11:]))
    best = min(out['chain_diag_dev_ms'])
    out['speedup_over_summarize_and_copy'] = (out['summarize_ms_all_columns_extrapolated'] + out['tensor_copy_ms']) / best
    out['speedup_over_numpy_and_copy'] = (out['numpy_ms_all_columns_extrapolated'] + out['tensor_copy_ms']) / best
    full = dev
    out['rhat_max'] = float(np.max(full[_lib.DIAG_ROWS.index('rhat')]))
    out['ess_bulk_over_S_median'] = float(np.median(full[_lib.DIAG_ROWS.index('ess_bulk')]) / (C * n))
    out['ess_law_(1-rho)/(1+rho)'] = (1.0 - RHO) / (1.0 + RHO)
    d.close()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=500.0, help='length of a timed window of queued calls')
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--chains', default='4x1000,1x200', help='chain shapes C x n')
    ap.add_argument('--subset', type=int, default=64, help='columns the host routes are timed on')
    ap.add_argument('--kernel-stats', default=None, metavar='C2_4x1000=CSV,...',
                    help='tools/rocprof_summary.py stats files of --trace-loop runs under rocprofv3 --kernel-trace --stats')
    ap.add_argument('--trace-loop', action='store_true', help='set-up, then --calls queued pgl_chain_diag_dev calls (to be traced)')
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("diag_bench: no GPU visible; nothing is measured without one")
    stats = dict(kv.split('=', 1) for kv in a.kernel_stats.split(',')) if a.kernel_stats else {}
    res = {'bench': 'diag_trace_loop' if a.trace_loop else 'diag'}
    for k in a.configs.split(','):
        M, P = SHAPES[k]
        for ch in a.chains.split(','):
            C, n = [int(v) for v in ch.split('x')]
            key = '%s_%s' % (k, ch)
            res[key] = trace_loop(M, P, C, n, a.calls) if a.trace_loop else run(M, P, C, n, a.window_ms, stats.get(key), a.subset)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")
