"""Clamped simulation on the device (pgl_cond_currents_dev + pgl_simulate_cond_dev, one wave per (neuron, 64 replicates))
against the route the library had for it: pgl_simulate_batch_dev on the same clamped currents with a diagonal-only AW (one
workgroup per replicate).  C2 (N = 32, nT = 300 000) and C3 (N = 128, nT = 600 000) on the seeded standard_glm draw of
tools/sim_bench.py; the recording is one replicate of the batched simulation of that draw.

Per configuration, for n_rep replicates (default 256): wall time of queued calls of each kernel in windows of at least 0.5 s that
end in a synchronisation (a call longer than the window is a window of one call; three windows, one where a call takes 5 s or
more); the same for pgl_simulate_batch_dev; the achieved rate of USEFUL reads of Xc (n_rep N nT 8 bytes per call: every chain reads its column once; the lines fetched are
wider); waves per SIMD the grid offers and the code object's registers and LDS; the chains that took the fallback ring; the
agreement of the two routes' counts.  Kernel times come from `rocprofv3 --kernel-trace --stats` in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/condsim_bench.py --worker C3 --once
and are entered with --kernel-stats DIR/..._kernel_stats.csv; without it the JSON says "not measured".
No speed-up is assumed: the ratio is reported as measured.

    python tools/condsim_bench.py [--configs C2,C3] [--n-rep 256] [--timeout 900] [--out profiles/condsim_bench.json]"""
import argparse, csv, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from sim_bench import CONFIGS, SEED, inputs  # noqa: E402

WINDOW = 0.5
WIN = 50


def windows(call, sync, min_windows=3):
    """mean seconds per call over windows of >= WINDOW s of queued calls, each ended by a synchronisation"""
    call(); sync()                                            # warm-up
    t0 = time.perf_counter(); call(); sync()
    one = time.perf_counter() - t0
    k = max(1, int(np.ceil(WINDOW / max(one, 1e-6))))
    per = []
    for _ in range(min_windows if one < 5.0 else 1):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        sync()
        per.append((time.perf_counter() - t0) / k)
    return {'s_per_call': float(np.mean(per)), 'calls_per_window': k, 'windows': len(per), 'min': float(min(per)), 'max': float(max(per))}


def worker(name, n_rep, once):
    import torch
    from theano_pyglm_amd import _lib
    N, nT = CONFIGS[name]
    X0, AW, kind, dt = inputs(N, nT)
    R = AW.shape[1]
    rec = _lib.simulate_batch(X0, AW, kind, dt, 1, seed=SEED, rep0=100000)
    S_obs = rec['S'][0]
    pre, cnt, off = _lib.spike_events(S_obs)
    obs = _lib.window_counts(S_obs, WIN)
    out = {'config': name, 'N': N, 'nT': nT, 'R': R, 'nlin': kind, 'n_rep': n_rep, 'win': WIN, 'events': int(pre.size),
           'recorded_rate_hz_mean': float(S_obs.sum() / (nT * dt) / N), 'recording_exceptions': int(rec['exceptions'][0])}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    D = np.zeros_like(AW)
    i = np.arange(N)
    D[i, :, i] = AW[i, :, i]
    d_X0, d_AW, d_D, d_pre, d_cnt, d_off, d_obs = t(X0), t(AW), t(D), t(pre), t(cnt), t(off), t(obs)
    d_Xc = torch.empty((nT, N), dtype=torch.float64, device='cuda')
    d_acc = torch.empty((_lib.CS_NACC,) + obs.shape, dtype=torch.int64, device='cuda')
    d_exc = torch.empty(N, dtype=torch.int64, device='cuda')
    d_fb = torch.empty(1, dtype=torch.int64, device='cuda')
    d_cc = torch.empty((n_rep, N), dtype=torch.int64, device='cuda')
    d_ws = torch.empty(_lib.simulate_cond_workspace(N, R, n_rep) // 8, dtype=torch.float64, device='cuda')
    sync = torch.cuda.synchronize
    cur = lambda: _lib.cond_currents_dev(N, nT, R, d_X0, d_AW, d_pre, d_cnt, d_off, d_Xc)
    sim = lambda: _lib.simulate_cond_dev(N, nT, R, kind, dt, d_Xc, d_AW, d_obs, WIN, n_rep, d_acc, d_exc, d_ws, seed=SEED,
                                         d_counts=d_cc, d_fallbacks=d_fb)
    in_lds, ws_bytes = _lib.simulate_batch_plan(N, R)
    d_bc = torch.empty((n_rep, N), dtype=torch.int64, device='cuda')
    d_be = torch.empty(n_rep, dtype=torch.int64, device='cuda')
    d_bws = None if in_lds else torch.empty(n_rep * ws_bytes // 8, dtype=torch.float64, device='cuda')
    old = lambda: _lib.simulate_batch_dev(N, nT, R, kind, dt, d_Xc, d_D, n_rep, d_bc, d_be, seed=SEED,
                                          d_workspace=0 if d_bws is None else d_bws)
    sync()
    if once:                                                  # under rocprofv3 --kernel-trace --stats: one launch of each
        cur(); sim(); old(); sync()
        return out
    out['k_cond_currents'] = windows(cur, sync)
    out['k_simulate_cond'] = windows(sim, sync)
    out['k_simulate_cond']['us_per_bin'] = out['k_simulate_cond']['s_per_call'] / nT * 1e6
    out['xc_useful_read_GBps'] = n_rep * N * nT * 8 / out['k_simulate_cond']['s_per_call'] / 1e9
    out['fallback_chains'] = int(d_fb.cpu().numpy()[0])
    out['chains'] = n_rep * N
    out['exceptions'] = int(d_exc.cpu().numpy().sum())
    out['pgl_simulate_batch_dev_diagonal'] = windows(old, sync)
    out['pgl_simulate_batch_dev_diagonal']['us_per_bin'] = out['pgl_simulate_batch_dev_diagonal']['s_per_call'] / nT * 1e6
    out['batch_exceptions'] = int(d_be.cpu().numpy().sum())
    out['counts_equal'] = bool(np.array_equal(d_cc.cpu().numpy(), d_bc.cpu().numpy()))
    out['batch_over_cond'] = out['pgl_simulate_batch_dev_diagonal']['s_per_call'] / out['k_simulate_cond']['s_per_call']
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = N * ((n_rep + 63) // 64)
    out['compute_units'] = cus
    out['waves'] = waves
    out['waves_per_simd_offered'] = waves / (4.0 * cus)
    return out


def resources():
    import reachable_kernels as RK
    built = RK.built_fused()
    return dict((n, dict((k, r[k]) for k in ('vgpr', 'sgpr', 'lds', 'scratch', 'spill_vgpr', 'spill_sgpr')))
                for n, r in built.items() if n.startswith(('k_cond_currents', 'k_simulate_cond<')))


def kernel_stats(path):
    """rows of a rocprofv3 kernel_stats.csv for the kernels of this bench"""
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            if any(k in r.get('Name', '') for k in ('k_cond_currents', 'k_simulate_cond', 'k_simulate<')):
                rows[r['Name']] = {'calls': int(r['Calls']), 'mean_ns': float(r['AverageNs'])}
    return rows


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--n-rep', type=int, default=256)
    ap.add_argument('--timeout', type=int, default=900, help='seconds a configuration may take (child process)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-stats', default=None, help='NAME=CSV[,NAME=CSV]: rocprofv3 kernel_stats.csv of --once runs')
    ap.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--once', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        print('RESULT ' + json.dumps(worker(a.worker, a.n_rep, a.once), sort_keys=True))
        sys.exit(0)
    import __graft_entry__ as ge
    ge.build_hip()
    res = {'bench': 'condsim', 'resources': resources(),
           'lds_note': 'k_simulate_cond: static LDS (queue + tiles) plus R * 8 bytes of dynamic LDS for the self-history'}
    stats = dict(kv.split('=', 1) for kv in a.kernel_stats.split(',')) if a.kernel_stats else {}
    for name in a.configs.split(','):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', name, '--n-rep', str(a.n_rep)],
                           stdout=subprocess.PIPE, timeout=a.timeout, check=True)
        res[name] = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith('RESULT ')][-1][7:])
        res[name]['kernel_trace'] = kernel_stats(stats[name]) if name in stats else 'not measured'
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
