"""Coupling significance tests on the device (inference/connectivity.py: coupling_tests over pgl_wald_groups_dev) at C2
(N = 32, nT = 300 000, P = 161) and C3 (N = 128, nT = 600 000, P = 641), standard_glm with a Gaussian(0, 1) prior on the
impulse weights, at a parameter point drawn from the prior with the impulse weights scaled by 0.05 (NOT a fit: minus the
Hessian of a log-concave posterior is positive definite everywhere, which is all the timings need; lr1 - T at such a point
says nothing about a fit).  No figure is a pass / fail bar.  Per configuration:
  (a) pgl_wald_groups_dev on the resident factor W (N, P, P) of laplace_on_device, all N groups of all N rows, without and
      with d_u: wall time per call of queued calls with one synchronisation inside the clock, three windows (the spread),
      beside the bytes of the lower triangles (N P (P + 1) / 2 doubles: what one pass over W must read); and, from a kernel
      trace taken in a run of its own (nothing else is collected in that run), the time of k_wald_groups per call;
  (b) one whole coupling_tests(one_step_lr=True) call after a warm-up call, and its split into Hessian / factor / inverse /
      Wald / evaluations (coupling_tests' timings: each stage behind a synchronisation; the rest is host work).
The kernel time comes from
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/conn_bench.py --trace-loop --configs C3 [--with-u]
    python tools/rocprof_summary.py stats DIR/.../*results.db profiles/conn_bench_kernel_stats_C3.csv
    python tools/conn_bench.py --kernel-stats C2=...,C3=... [--kernel-stats-u C2=...,C3=...] --out profiles/conn_bench.json
Without --kernel-stats the kernel time is left out.  Prints one JSON line."""
import argparse, csv, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theano_pyglm_amd import _lib
from theano_pyglm_amd.inference import connectivity as CN
from theano_pyglm_amd.inference.laplace import laplace_on_device
from theano_pyglm_amd.models.model_factory import make_model
from theano_pyglm_amd.population import Population

SHAPES = {'C2': (32, 300000), 'C3': (128, 600000)}


def population(N, nT):
    rng = np.random.default_rng(1234)
    dt = 0.001
    model = make_model('standard_glm', N=N, dt=dt)
    model['impulse']['prior'] = {'type': 'gaussian', 'mu': 0.0, 'sigma': 1.0}
    popn = Population(model)
    S = np.minimum(rng.poisson(20.0 * dt, size=(nT, N)), 10).astype(np.uint8)
    popn.add_data({'S': S, 'N': N, 'dt': dt, 'T': nT * dt, 'stim': None, 'dt_stim': 0.1})
    x = popn.sample(np.random.RandomState(7))
    for g in x['glms']:                                        # (N(0, 1) weights of 128 inputs would saturate the rates)
        g['imp']['w_ir'] = 0.05 * np.asarray(g['imp']['w_ir'], dtype=float)
    return popn, x


def setup(N, nT):
    """the population, the point, the factor W resident on the device and the two calls (without / with d_u)"""
    import torch
    popn, x = population(N, nT)
    lap, A, pi, shapes = laplace_on_device(popn, x)
    del A
    W = lap['W'].contiguous()
    info = lap['info'].to(torch.int32).contiguous()
    B, first = int(popn.glm.imp_model.B), 1 + int(popn.glm.Dstim)
    theta = torch.tensor(popn.theta_matrix(x), dtype=torch.float64, device='cuda')
    c = torch.tensor(CN.effective_weight_contrast(popn), dtype=torch.float64, device='cuda')
    out = torch.empty((N, N, _lib.WALD_NOUT), dtype=torch.float64, device='cuda')
    u = torch.empty((N * N, pi.size), dtype=torch.float64, device='cuda')
    d = popn._handle(popn.data_sequences[0])
    torch.cuda.synchronize()                                   # (torch's stream filled what the handle's stream reads)
    plain = lambda: d.wald_groups(W, theta, first, N, B, c, info, out=out)
    with_u = lambda: d.wald_groups(W, theta, first, N, B, c, info, out=out, u=u)
    return popn, x, d, int(pi.size), B, int(info.count_nonzero().item()), plain, with_u


def trace_loop(name, N, nT, calls, with_u):
    """what the kernel trace is taken of: the set-up, then queued pgl_wald_groups_dev calls and nothing else"""
    popn, x, d, P, B, bad, plain, wu = setup(N, nT)
    for _ in range(calls):
        (wu if with_u else plain)()
    d.sync()
    popn.release_data()
    return {'config': name, 'calls': calls, 'with_u': bool(with_u)}


def kernel_times(path):
    with open(path) as f:
        rows = list(csv.reader(ln for ln in f if not ln.startswith('#')))
    return dict((r[0], (int(r[1]), float(r[2]))) for r in rows[1:])


def kernel_ms(out, key, stats_path, tri_bytes):
    rows = [(k, v) for k, v in kernel_times(stats_path).items() if 'k_wald_groups' in k]
    if len(rows) != 1:
        out[key + '_trace_error'] = "k_wald_groups is not one row of %s" % stats_path
        return
    ms = rows[0][1][1] / rows[0][1][0] * 1e-3
    out[key + '_kernel_ms'] = ms
    out[key + '_traced_dispatches'] = rows[0][1][0]
    out[key + '_lower_triangle_GB_per_s'] = tri_bytes / (ms * 1e-3) / 1e9


def run(name, N, nT, window_ms, stats, stats_u):
    popn, x, d, P, B, bad, plain, with_u = setup(N, nT)
    tri = float(N) * P * (P + 1) / 2 * 8
    out = {'config': name, 'N': N, 'nT': nT, 'P': P, 'B': B, 'groups': N * N, 'rows_not_positive_definite': bad,
           'lower_triangle_bytes': tri, 'W_bytes': float(N) * P * P * 8, 'u_bytes': float(N) * N * P * 8,
           'point_is': 'a draw from the prior with the impulse weights scaled by 0.05, not a fit'}

    def timed(call, calls):
        d.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        d.sync()
        return (time.perf_counter() - t0) / calls * 1e3

    for key, call in (('wald_groups_dev', plain), ('wald_groups_dev_with_u', with_u)):
        calls = max(20, int(np.ceil(window_ms / timed(call, 20))))       # (the pilot is the warm-up)
        out[key + '_calls_per_window'] = calls
        out[key + '_ms'] = [timed(call, calls) for _ in range(3)]
    if stats is not None:
        kernel_ms(out, 'k_wald_groups', stats, tri)
    if stats_u is not None:
        kernel_ms(out, 'k_wald_groups_with_u', stats_u, tri)
    # (b) the whole call
    CN.coupling_tests(popn, x, one_step_lr=True)
    t0 = time.perf_counter()
    res = CN.coupling_tests(popn, x, one_step_lr=True)
    out['coupling_tests_ms'] = (time.perf_counter() - t0) * 1e3
    tm = {}
    CN.coupling_tests(popn, x, one_step_lr=True, timings=tm)
    out['stages_ms'] = dict((k, v * 1e3) for k, v in tm.items())
    out['stages_ms_sum'] = sum(out['stages_ms'].values())
    ok = np.isfinite(res['lr1']) & np.isfinite(res['wald'])
    rel = np.abs(res['lr1_minus_wald'][ok]) / np.maximum(res['wald'][ok], 1.0)
    out['lr1_minus_wald_over_max_T_1_median_max'] = [float(np.median(rel)), float(np.max(rel))] if rel.size else None
    out['significant_pairs'] = int(np.sum(res['significant']))
    out['rows_pd'] = int(np.sum(res['pd']))
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--window-ms', type=float, default=500.0, help='length of a timed window of queued calls')
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--kernel-stats', default=None, metavar='C2=CSV,C3=CSV',
                    help='tools/rocprof_summary.py stats files of --trace-loop runs under rocprofv3 --kernel-trace --stats')
    ap.add_argument('--kernel-stats-u', default=None, metavar='C2=CSV,C3=CSV', help='the same of --trace-loop --with-u runs')
    ap.add_argument('--trace-loop', action='store_true', help='set-up, then --calls queued pgl_wald_groups_dev calls (to be traced)')
    ap.add_argument('--with-u', action='store_true', help='--trace-loop: the calls write d_u')
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--scale', type=float, default=1.0, help='dev: shrink nT (a rehearsal, not a measurement)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("conn_bench: no GPU visible; nothing is measured without one")
    split = lambda s: dict(kv.split('=', 1) for kv in s.split(',')) if s else {}
    stats, stats_u = split(a.kernel_stats), split(a.kernel_stats_u)
    res = {'bench': 'conn_trace_loop' if a.trace_loop else 'conn'}
    for k in a.configs.split(','):
        N, nT = SHAPES[k]
        nT = int(nT * a.scale)
        res[k] = trace_loop(k, N, nT, a.calls, a.with_u) if a.trace_loop else run(k, N, nT, a.window_ms, stats.get(k), stats_u.get(k))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")
