"""The lock-step HMC chain (inference/batched_hmc.py) per configuration, next to its floor and to the route the library
had before it, in one process.  Seeded inputs as tools/ncg_bench.py makes them (Poisson spikes at 20 Hz), standard_glm,
started at the lock-step BFGS MAP fit.

    python tools/hmc_bench.py [--configs C2,C3] [--out profiles/hmc_bench.json]

C2: N = 32, nT = 300 000; C3: N = 128, nT = 600 000.  Per configuration:
  device_ms_per_transition   wall time of the device chain (mass='laplace') per transition, steady (second) call
  floor_ms_per_transition    n_leapfrog bare pgl_ll_grad_dev calls of all rows on the same stream
  host_ms_per_transition     inference/hmc.py: hmc_lockstep over Population.compute_lp_grad_packed, all neurons' full
                             packed vectors, state dicts packed and unpacked per evaluation, called the way the
                             Hmc*Update classes call it (n_leapfrog + 1 evaluations per transition)
  bias_sd / laplace_se       posterior sd of every neuron's bias from the kept draws against the Laplace standard error
  mass                       the diagonal ('laplace') and the dense ('laplace_dense') mass matrix from the same fit, same seed,
                             same lengths, each the steady (second) call: ms_per_transition (the chain: the call minus the
                             mass set-up), over_floor, setup_s (Hessian + host factorisation), accept rate, median frozen
                             step, median ESS of the kept draws (of the biases, and of all parameters) and ESS per second of
                             chain time; dense_over_diagonal_ms the ratio of the two chains
  tri_matvec                 the dense chain's product launches alone (pgl_tri_matvec_dev on the uploaded factors): ms and
                             achieved GB/s (the lower triangle's bytes) per product, on the (tile, row) grid the library uses
                             and on one workgroup per row (the rejected variant, dev option 90)
Records, sets no threshold.  Prints one JSON line."""
import argparse, copy, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from ncg_bench import CONFIGS, population


def host_route(popn, x, n_leapfrog, step_sz, n_transitions, seed=0):
    """hmc_lockstep over compute_lp_grad_packed: ms per transition."""
    from theano_pyglm_amd.inference.hmc import hmc_lockstep
    from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars, set_vars
    x = copy.deepcopy(x)
    syms = popn.glm_syms()
    glms = x['glms']
    Q, shapes = [], None
    for n in range(popn.N):
        q, shapes = packdict(get_vars(syms, glms[n]))
        Q.append(q)
    Q = np.array(Q)

    def UG(Qn):
        for n in range(popn.N):
            set_vars(syms, glms[n], unpackdict(Qn[n].copy(), shapes))
        lp, G = popn.compute_lp_grad_packed(x)
        return np.where(np.isfinite(lp), -lp, np.inf), -np.nan_to_num(G, nan=0.0, posinf=0.0, neginf=0.0)

    rng = np.random.RandomState(seed)
    n_acc = 0
    t0 = time.perf_counter()
    for _ in range(n_transitions):                             # as the Hmc*Update classes call it: n_leapfrog + 1 evaluations
        Q, acc, _ = hmc_lockstep(UG, step_sz, n_leapfrog, Q, rng=rng)
        n_acc += int(acc.sum())
    return (time.perf_counter() - t0) * 1e3 / n_transitions, n_acc / float(n_transitions * popn.N)


def mass_figures(popn, x, mass, n_samples, n_warmup, n_leapfrog, floor_ms):
    """One mass matrix: the steady (second) call of sample_glms_hmc and what its draws are worth."""
    import torch
    from theano_pyglm_amd.inference.batched_hmc import sample_glms_hmc, summarize
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sample_glms_hmc(popn, x, n_samples, n_warmup=n_warmup, n_leapfrog=n_leapfrog, step_sz=0.1, mass=mass, seed=1)
        wall = time.perf_counter() - t0
    st = popn.last_fit_stats
    chain_s = wall - st['mass_setup_s']
    ess_bias = summarize(res['samples'][:, :, 0])['ess']
    ess_all = summarize(res['samples'])['ess']
    out = {'ms_per_transition': chain_s * 1e3 / st['transitions'], 'setup_s': st['mass_setup_s'],
           'accept_rate': {'min': float(res['accept_rate'].min()), 'mean': float(res['accept_rate'].mean())},
           'step_sz_median': float(np.median(res['step_sz'])),
           'ess_median_bias': float(np.median(ess_bias)), 'ess_median_all': float(np.median(ess_all)),
           'ess_min_all': float(np.min(ess_all))}
    out['over_floor'] = out['ms_per_transition'] / floor_ms
    out['ess_per_s_bias'] = out['ess_median_bias'] / chain_s
    out['ess_per_s_all'] = out['ess_median_all'] / chain_s
    if 'dense_rows' in res:
        out['dense_rows'] = int(res['dense_rows'].sum())
    return out


def product_figures(popn, h, stream, N, P, reps=20):
    """pgl_tri_matvec_dev alone on (N, P, P) factors: ms and GB/s of the lower triangle per product, both grids."""
    import torch
    dev = torch.device('cuda', popn.device)
    W = torch.tril(torch.randn((N, P, P), dtype=torch.float64, device=dev))
    xv = torch.randn((N, P), dtype=torch.float64, device=dev)
    yv = torch.empty((N, P), dtype=torch.float64, device=dev)
    nbytes = N * (P * (P + 1) // 2) * 8.0
    out = {'bytes_per_product': nbytes}
    torch.cuda.synchronize()
    for label, rows in (('tile_grid', 0), ('row_grid', 1)):
        h.set_option(90, rows)
        for trans in (0, 1):
            for k in range(2):
                stream.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    h.tri_matvec_dev(W.data_ptr(), N, P, trans, xv.data_ptr(), yv.data_ptr())
                stream.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / reps
            out['%s_%s' % (label, 'Wt_x' if trans else 'W_x')] = {'ms': ms, 'GBps': nbytes / (ms * 1e-3) / 1e9}
    h.set_option(90, 0)
    return out


def run(name, n_samples, n_warmup, n_leapfrog, host_transitions):
    import torch
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch
    from theano_pyglm_amd.inference.batched_hmc import sample_glms_hmc, summarize, _laplace_minv
    from theano_pyglm_amd.inference.laplace import laplace_glms
    N, nT = CONFIGS[name]
    popn = population(N, nT)
    x = popn.sample(np.random.RandomState(4321))
    fit_glms_batched_torch(popn, x)
    out = {'config': name, 'N': N, 'nT': nT, 'n_samples': n_samples, 'n_warmup': n_warmup, 'n_leapfrog': n_leapfrog}
    t0 = time.perf_counter()
    minv = _laplace_minv(popn, x, 0, N, 1e-8)                   # what mass='laplace' computes: once, outside the clock
    out['laplace_mass_s'] = time.perf_counter() - t0
    for rep in range(2):                                       # the second call is the steady one
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sample_glms_hmc(popn, x, n_samples, n_warmup=n_warmup, n_leapfrog=n_leapfrog, step_sz=0.1, mass=minv, seed=1)
        wall = time.perf_counter() - t0
    st = popn.last_fit_stats
    # (the whole call: upload of the start, the chain, the copy of the samples)
    out['device_ms_per_transition'] = wall * 1e3 / st['transitions']
    out['device_accept_rate'] = {'min': float(res['accept_rate'].min()), 'mean': float(res['accept_rate'].mean())}
    out['device_step_sz'] = {'min': float(res['step_sz'].min()), 'median': float(np.median(res['step_sz'])),
                             'max': float(res['step_sz'].max())}
    out['launches'] = {k: st[k] for k in ('ll_grad_launches', 'row_launches', 'host_syncs_in_chain')}
    # the floor: n_leapfrog bare evaluations
    h = popn._handle(popn.data_sequences[0])
    dev = torch.device('cuda', popn.device)
    P = popn.glm.P
    th = torch.tensor(popn.theta_matrix(x), dtype=torch.float64, device=dev)
    We = torch.tensor(popn.W_eff(x), dtype=torch.float64, device=dev)
    buf = torch.empty(N * (1 + P), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    h.set_stream(stream.cuda_stream)
    try:
        reps = 20
        for k in range(2):
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps * n_leapfrog):
                h.ll_grad_dev(th.data_ptr(), We.data_ptr(), buf.data_ptr(), buf[N:].data_ptr(), 0, N)
            stream.synchronize()
            out['floor_ms_per_transition'] = (time.perf_counter() - t0) * 1e3 / reps
        out['tri_matvec'] = product_figures(popn, h, stream, N, P)
    finally:
        h.set_stream(None)
    out['device_over_floor'] = out['device_ms_per_transition'] / out['floor_ms_per_transition']
    out['mass'] = dict((m, mass_figures(popn, x, m, n_samples, n_warmup, n_leapfrog, out['floor_ms_per_transition']))
                       for m in ('laplace', 'laplace_dense'))
    out['mass']['dense_over_diagonal_ms'] = (out['mass']['laplace_dense']['ms_per_transition'] /
                                             out['mass']['laplace']['ms_per_transition'])
    host_route(popn, x, n_leapfrog, 1e-3, 1)                   # warm
    ms, acc = host_route(popn, x, n_leapfrog, 1e-3, host_transitions)
    out['host_ms_per_transition'] = ms
    out['host_step_sz'] = 1e-3                                 # (identity mass, one shared step: timing only)
    out['host_accept_rate'] = acc
    out['host_over_device'] = ms / out['device_ms_per_transition']
    # bias: posterior sd against the Laplace standard error
    s = summarize(res['samples'][:, :, 0])
    lap = laplace_glms(popn, x)
    se = np.array([r['stderr_vec'][0] if r['pd'] else np.nan for r in lap])
    # (the bias is the first entry of the packed vector of standard_glm as well as of the theta row)
    ratio = s['sd'] / se
    ok = np.isfinite(ratio)
    out['bias'] = {'laplace_pd_rows': int(ok.sum()), 'sd_over_laplace_se': {
        'min': float(np.min(ratio[ok])) if ok.any() else None, 'median': float(np.median(ratio[ok])) if ok.any() else None,
        'max': float(np.max(ratio[ok])) if ok.any() else None}, 'ess_median': float(np.median(s['ess'])),
        'sd_median': float(np.median(s['sd'])), 'laplace_se_median': float(np.nanmedian(se)) if ok.any() else None}
    popn.release_data()
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--samples', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--leapfrog', type=int, default=10)
    ap.add_argument('--host-transitions', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'bench': 'hmc'}
    for name in a.configs.split(','):
        res[name] = run(name, a.samples, a.warmup, a.leapfrog, a.host_transitions)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
