"""Stimulus decoding on the device (pgl_decode_eval_dev, pgl_decode_hvp_dev) against the only route the library had for the
objective: pgl_set_stimulus (the feature build) plus one forward-only pgl_ll_grad (grad_out = NULL) per trial stimulus -- a route
that gives no gradient at all.  C2 (N = 32, nT = 300 000) and C3 (N = 128, nT = 600 000) with a 'basis' stimulus of D = 1
dimension, B = 3 basis functions over Rt = 200 taps, q = 100 bins per frame; seeded spikes at 20 Hz.

Per configuration: wall time per call of queued calls in windows of at least 0.5 s that end in a synchronisation, three
windows; 2 nT N Rt D flops per convolution (eval with a gradient and hvp: two convolutions each) and the (nT, N) planes a call
must move at least once (eval: c in, r and cc out, r in again; hvp: cc in, y out and in) -- a floor, not the kernels' traffic.
The kernels' achieved bytes and flops per second are their own model (kernel_model: the staged K slabs and the rows of s or y
re-read per tap chunk included, about 16 planes for k_dec_backward at Rt = 200) over their traced mean times.  Kernel times come from
`rocprofv3 --kernel-trace --stats` in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/decode_bench.py --worker C3 --once
and are entered with --kernel-stats DIR/..._kernel_stats.csv --stats-config C3; without it the JSON says "not measured" for the
kernels.  No figure is asserted.

    python tools/decode_bench.py [--configs C2,C3] [--timeout 900] [--out profiles/decode_bench.json]"""
import argparse, csv, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {'C2': (32, 300000), 'C3': (128, 600000)}
WINDOW = 0.5
D, B_STIM, RT, Q = 1, 3, 200, 100


def windows(call, sync, min_windows=3):
    """mean seconds per call over windows of >= WINDOW s of queued calls, each ended by a synchronisation"""
    call(); sync()
    t0 = time.perf_counter(); call(); sync()
    one = time.perf_counter() - t0
    k = max(1, int(np.ceil(WINDOW / max(one, 1e-6))))
    per = []
    for _ in range(min_windows):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        sync()
        per.append((time.perf_counter() - t0) / k)
    return {'s_per_call': float(np.mean(per)), 'calls_per_window': k, 'windows': len(per), 'min': float(min(per)), 'max': float(max(per))}


def worker(name, once):
    import torch
    from tests import helpers as H
    from theano_pyglm_amd import _lib
    N, nT = CONFIGS[name]
    p = H.Problem(N, nT, H.std_ibasis(), seed=321)
    rng = np.random.default_rng(9)
    Tu = nT // Q
    stim = rng.standard_normal((Tu, D))
    basis_t = H.std_ibasis(RT)[:, :B_STIM]
    d = p.device(0)
    d.set_stimulus(stim, Q * p.dt, basis_t, None, layout=1)
    theta = np.concatenate([p.theta[:, :1], 0.5 * rng.standard_normal((N, D * B_STIM)), p.theta[:, 1:]], axis=1)
    out = {'config': name, 'N': N, 'nT': nT, 'Rt': RT, 'D': D, 'B': B_STIM, 'q': Q, 'Tu': Tu}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    d_theta, d_Weff, d_u, d_v = t(theta), t(p.Weff), t(stim), t(rng.standard_normal((Tu, D)))
    d_F = torch.empty(3, dtype=torch.float64, device='cuda')
    d_g, d_hv = torch.empty_like(d_u), torch.empty_like(d_u)
    d_ll = torch.empty(N, dtype=torch.float64, device='cuda')
    prior = (0.0, 1.0, np.inf)
    sync = d.sync
    d.decode_prepare_dev(d_theta, d_Weff)
    ev = lambda: d.decode_eval_dev(d_u, Tu, Q, prior, d_F, d_g)
    ev0 = lambda: d.decode_eval_dev(d_u, Tu, Q, prior, d_F, 0)
    hv = lambda: d.decode_hvp_dev(d_v, d_hv)

    def old():                                                 # the parent's route: rebuild the feature columns, forward-only ll
        d.set_stimulus(stim, Q * p.dt, basis_t, None, layout=1)
        d.ll_grad_dev(d_theta, d_Weff, d_ll, 0)
    sync()
    if once:
        ev(); hv(); old(); sync()
        return out
    t0 = time.perf_counter(); d.decode_prepare_dev(d_theta, d_Weff); sync()
    out['prepare_s'] = time.perf_counter() - t0
    out['eval_grad'] = windows(ev, sync)
    out['eval_only'] = windows(ev0, sync)
    out['hvp'] = windows(hv, sync)
    conv_flops = 2.0 * nT * N * RT * D
    plane = 8.0 * nT * N
    out['flops_per_call'] = {'eval_grad': 2 * conv_flops, 'eval_only': conv_flops, 'hvp': 2 * conv_flops}
    # the (nT, N) planes a call cannot avoid moving once: the floor of its traffic, NOT what the kernels fetch (kernel_model)
    out['min_plane_bytes_per_call'] = {'eval_grad': 4 * plane, 'eval_only': 3 * plane, 'hvp': 3 * plane}
    for k in ('eval_grad', 'eval_only', 'hvp'):
        out[k]['wall_flops_per_s'] = out['flops_per_call'][k] / out[k]['s_per_call']
        out[k]['wall_min_plane_bytes_per_s'] = out['min_plane_bytes_per_call'][k] / out[k]['s_per_call']
    F_new = d_F.cpu().numpy().copy()
    out['set_stimulus_plus_forward_ll'] = windows(old, sync)   # (last: it invalidates the prepare)
    out['ll_agreement'] = {'decode_log_lik': float(F_new[1]), 'sum_ll_grad': float(d_ll.sum().item())}
    out['ratio_old_over_eval_only'] = out['set_stimulus_plus_forward_ll']['s_per_call'] / out['eval_only']['s_per_call']
    d.close()
    return out


def kernel_model(name, N, nT):
    """(flops, bytes) one launch of a decoding kernel must execute and move at this shape, by the kernel's own tiling
    (csrc/pglm_decode.hip.h) -- the re-reads included, since they are what the memory system serves (L2 absorbs part of them;
    how much was not measured):
      k_dec_forward   per (64-bin sub-tile, slab of 64 neurons, dimension, 32 taps): a K slab of 32 x 64 doubles and 96 values of
                      s; per element of the plane: mode 0 reads c and writes r and cc, mode 1 reads cc and writes y;
      k_dec_backward  per (64-bin tile, dimension, slab, 16 taps): 80 rows x 64 of y and 16 x 64 of K; writes g_s."""
    conv = 2.0 * nT * N * RT * D
    plane = 8.0 * nT * N
    slabs = -(-N // 64)
    tiles = -(-nT // 64)
    if 'k_dec_forward' in name:
        staged = tiles * slabs * D * (-(-RT // 32)) * (32 * 64 + 96) * 8.0
        return conv, staged + (2 if ', 1>' in name else 3) * plane
    if 'k_dec_backward' in name:
        return conv, tiles * D * slabs * (-(-RT // 16)) * (80 * 64 + 16 * 64) * 8.0 + 8.0 * nT * D
    return None


def kernel_stats(path, config):
    """the k_dec_* rows of a rocprofv3 --kernel-trace --stats file of a `--worker CONFIG --once` run, with the achieved flops and
    bytes per second of the two convolution kernels: the model of kernel_model over the kernel's mean time"""
    if not path:
        return "not measured"
    N, nT = CONFIGS[config]
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get('Name', '')
            if 'k_dec_' not in name:
                continue
            mean_s = float(r['AverageNs']) * 1e-9
            row = {'calls': int(r['Calls']), 'total_ns': float(r.get('TotalDurationNs') or 0.0), 'mean_ns': float(r['AverageNs'])}
            model = kernel_model(name, N, nT)
            if model and mean_s > 0:
                row.update({'model_flops': model[0], 'model_bytes': model[1], 'flops_per_s': model[0] / mean_s,
                            'bytes_per_s': model[1] / mean_s})
            rows[name] = row
    return rows or "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--worker')
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--kernel-stats', default=None, help='the ..._kernel_stats.csv of a rocprofv3 run of --worker CONFIG --once')
    ap.add_argument('--stats-config', default='C3', help='the CONFIG of that run (default C3)')
    ap.add_argument('--timeout', type=int, default=900)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'decode_bench.json'))
    args = ap.parse_args()
    if args.worker:
        print('RESULT ' + json.dumps(worker(args.worker, args.once)))
        return
    import __graft_entry__ as g
    g.build()
    results = []
    for name in args.configs.split(','):                       # a fresh process per configuration
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', name], capture_output=True, text=True,
                           timeout=args.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        results.append(json.loads(line[-1][7:]) if line else {'config': name, 'status': 'not measured', 'stderr': r.stderr[-2000:]})
    doc = {'tool': 'tools/decode_bench.py', 'results': results, 'kernel_stats_config': args.stats_config if args.kernel_stats else None,
           'kernels': kernel_stats(args.kernel_stats, args.stats_config)}
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == '__main__':
    main()
