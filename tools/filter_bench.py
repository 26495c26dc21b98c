"""Posterior bands of the filters on the device (DeviceGlm.filter_bands over pgl_filter_bands_dev) on the samplers' tensor
(n, C M, P) at the shapes of C2 (32 neurons, P = 161) and C3 (128 neurons, P = 641): the N groups of B = 5 impulse weights of
every row against a basis of R = 200 lags, for C = 4 chains of n = 1000 draws and for one chain of 200.  The draws are
SYNTHETIC: independent AR(1) series (rho = 0.5, unit variance) generated on the device, the basis is random -- the figures time
the reduction, they say nothing about a posterior.  No figure is a pass / fail bar.  Per configuration and chain shape:
  (a) pgl_filter_bands_dev on the resident tensor: wall time per call of queued calls with one synchronisation inside the
      clock, three windows of --window-ms (the spread); and, from a kernel trace taken in a run of its own (nothing else is
      collected in that run), the time of k_filter_bands per call;
  (b) the device-to-host copy of the tensor;
  (c) filters.filter_bands_numpy timed on a subset of the groups of row 0, scaled to all M N groups, and whether its bits
      equal the device's on that subset.
The kernel time comes from
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/filter_bench.py --trace-loop --configs C3 --chains 4x1000
    python tools/rocprof_summary.py stats DIR/.../*results.db profiles/filter_bench_kernel_stats_C3_4x1000.csv
    python tools/filter_bench.py --kernel-stats C3_4x1000=...,... --out profiles/filter_bench.json
Without --kernel-stats the kernel time is left out.  Prints one JSON line."""
import argparse, csv, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import filters as F

SHAPES = {'C2': (32, 161), 'C3': (128, 641)}
B, R, LEVEL, RHO, DT = 5, 200, 0.95, 0.5, 0.001


def setup(M, P, C, n):
    """a handle (it supplies the stream only), the synthetic draws (n, C * M, P) resident on the device, basis and contrast"""
    import torch
    d = _lib.DeviceGlm(4, 100, 5, 200, 'explinear', 0.001)
    g = torch.Generator(device='cuda')
    g.manual_seed(1234)
    x = torch.empty((n, C * M, P), dtype=torch.float64, device='cuda')
    x[0] = torch.randn((C * M, P), dtype=torch.float64, device='cuda', generator=g)
    for i in range(1, n):
        x[i] = RHO * x[i - 1] + np.sqrt(1.0 - RHO * RHO) * torch.randn((C * M, P), dtype=torch.float64, device='cuda', generator=g)
    basis = np.random.default_rng(7).normal(size=(R, B))
    c = DT * basis.sum(axis=0)
    G = (P - 1) // B
    bd, cd = (torch.tensor(a, dtype=torch.float64, device='cuda') for a in (basis, c))
    out = torch.empty((M, G, R, 5), dtype=torch.float64, device='cuda')
    grp = torch.empty((M, G, 8), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    return d, x, basis, c, G, out, grp, (lambda: d.filter_bands(x, C, 1, G, bd, cd, LEVEL, out=out, grp=grp))


def trace_loop(M, P, C, n, calls):
    """what the kernel trace is taken of: the set-up, then queued pgl_filter_bands_dev calls and nothing else"""
    d, call = setup(M, P, C, n)[::7]
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
    d, x, basis, c, G, out_d, grp_d, call = setup(M, P, C, n)
    out = {'neurons': M, 'parameters': P, 'groups': M * G, 'weights_per_group': B, 'lags': R, 'chains': C, 'draws_per_chain': n,
           'level': LEVEL, 'tensor_bytes': float(n) * C * M * P * 8, 'curves_bytes_if_materialised': float(n) * C * M * G * R * 8,
           'weights_resident_in_lds': bool((n * C * B + (1 << max(1, int(np.ceil(np.log2(n * C)))))) * 8 <= 144 * 1024),
           'draws_are': 'synthetic AR(1), rho = %.1f, generated on the device; not a sampler\'s output' % RHO}

    def timed(calls):
        d.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        d.sync()
        return (time.perf_counter() - t0) / calls * 1e3

    timed(1)                                                     # (warm-up)
    calls = max(1, int(np.ceil(window_ms / timed(1))))
    out['calls_per_window'] = calls
    out['filter_bands_dev_ms'] = [timed(calls) for _ in range(3)]
    if stats is not None:
        rows = [(k, v) for k, v in kernel_times(stats).items() if 'k_filter_bands' in k]
        if len(rows) == 1:
            out['k_filter_bands_kernel_ms'] = rows[0][1][1] / rows[0][1][0] * 1e-3
            out['k_filter_bands_traced_dispatches'] = rows[0][1][0]
        else:
            out['kernel_trace_error'] = "k_filter_bands is not one row of %s" % stats
    dev_out, dev_grp = out_d[0].cpu().numpy(), grp_d[0].cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = x.cpu().numpy()
    out['tensor_copy_ms'] = (time.perf_counter() - t0) * 1e3
    gs = min(G, subset)
    row0 = np.ascontiguousarray(host.reshape(n, C, M, P)[:, :, 0, :])                   # (n, C, P): row 0 of every chain
    t0 = time.perf_counter()
    ref_out, ref_grp = F.filter_bands_numpy(row0, C, 1, gs, basis, c, LEVEL)
    out['numpy_ms_per_group'] = (time.perf_counter() - t0) / gs * 1e3
    out['numpy_ms_all_groups_extrapolated'] = out['numpy_ms_per_group'] * M * G
    out['host_groups_timed'] = gs
    same = lambda a, b: bool(np.array_equal(np.isnan(a), np.isnan(b)) and
                             np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64)))
    out['bits_equal_device_numpy'] = same(np.ascontiguousarray(dev_out[:gs]), ref_out[0]) and \
        same(np.ascontiguousarray(dev_grp[:gs]), ref_grp[0])
    out['speedup_over_numpy_and_copy'] = (out['numpy_ms_all_groups_extrapolated'] + out['tensor_copy_ms']) / min(out['filter_bands_dev_ms'])
    out['c_sim_median'] = float(np.median(grp_d[..., 0].cpu().numpy()))
    d.close()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=500.0, help='length of a timed window of queued calls')
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--chains', default='4x1000,1x200', help='chain shapes C x n')
    ap.add_argument('--subset', type=int, default=64, help='groups the numpy statement is timed on')
    ap.add_argument('--kernel-stats', default=None, metavar='C2_4x1000=CSV,...',
                    help='tools/rocprof_summary.py stats files of --trace-loop runs under rocprofv3 --kernel-trace --stats')
    ap.add_argument('--trace-loop', action='store_true', help='set-up, then --calls queued pgl_filter_bands_dev calls (to be traced)')
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("filter_bench: no GPU visible; nothing is measured without one")
    stats = dict(kv.split('=', 1) for kv in a.kernel_stats.split(',')) if a.kernel_stats else {}
    res = {'bench': 'filter_trace_loop' if a.trace_loop else 'filter'}
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
