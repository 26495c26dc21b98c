"""Lock-step dense Newton (inference/batched_newton.py) next to lock-step Newton-CG and lock-step BFGS, in one process, from
two starts per configuration: the population.sample() start the sweeps use, and the BFGS fit.  Seeded inputs of
tools/ncg_bench.py (standard_glm, group-lasso impulse prior).

    python tools/newton_bench.py [--configs C2,C3] [--budget-s 900] [--out profiles/newton_bench.json]

Per configuration and start, for each optimiser: wall time, outer iterations, launch counts (Hessian / factor / solve /
evaluation for Newton with the seconds spent in each; prepare / apply / evaluation for Newton-CG; evaluations for BFGS),
the final max|g| from an independent Population.compute_lp_grad_packed, and f minus the BFGS f per neuron (min / median /
max; negative: below BFGS).  And pgl_chol_solve_dev alone against the route it replaces (pgl_tri_inverse_dev plus two
pgl_tri_matvec_dev) on the factor of the Hessians at the BFGS fit.  A wall budget bounds the whole: what no longer fits
is recorded as skipped, not guessed.  The file is rewritten after every measurement.  Records, sets no threshold."""
import argparse, copy, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from ncg_bench import CONFIGS, population


def q3(v):
    v = np.asarray(v, dtype=float)
    return {'min': float(v.min()), 'median': float(np.median(v)), 'max': float(v.max())}


def gmax(popn, x):
    lp, g = popn.compute_lp_grad_packed(x)
    return -lp, float(np.max(np.abs(g)))


def fit(kind, popn, x0):
    import torch
    from theano_pyglm_amd.inference.batched_bfgs import fit_glms_batched_torch
    from theano_pyglm_amd.inference.batched_newton import fit_glms_newton_torch
    from theano_pyglm_amd.inference.batched_newton_cg import fit_glms_newton_cg_torch
    x = copy.deepcopy(x0)
    tm = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == 'newton':
        fit_glms_newton_torch(popn, x, timings=tm)
    elif kind == 'newton_cg':
        fit_glms_newton_cg_torch(popn, x)
    else:
        fit_glms_batched_torch(popn, x)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    st = dict((k, v) for k, v in (popn.last_fit_stats or {}).items() if k not in ('per_neuron', 'cg_lengths', 'apply_kernels'))
    per = (popn.last_fit_stats or {}).get('per_neuron', {})
    rec = {'wall_s': wall, 'stats': st}
    if tm:
        rec['phase_s'] = tm
    if 'status' in per:
        u, c = np.unique(per['status'], return_counts=True)
        rec['status_counts'] = dict((str(int(a)), int(b)) for a, b in zip(u, c))
    if 'nit' in per:
        rec['nit'] = q3(per['nit'])
    f, g = gmax(popn, x)
    rec['max_abs_g'] = g
    return rec, x, f


def solve_alone(popn, x, reps=5):
    """seconds of pgl_chol_solve_dev and of tri_inverse + two tri_matvec on the factor of A at x, all rows"""
    import torch
    from theano_pyglm_amd.inference.batched_bfgs import _Packing
    from theano_pyglm_amd.inference.lockstep import session
    N = popn.N
    with session(popn) as (torch, dev, stream, handles):
        h = handles[0]
        pk = _Packing(popn, torch, handles, (0, N))
        P, prm = pk.Pp, pk.prior_params()
        f64 = torch.float64
        st = torch.zeros(h.newton_state_doubles(N, P), dtype=f64, device=dev)
        st[:N * P].copy_(torch.tensor(pk.pack(x, 0, N), dtype=f64, device=dev).view(-1))
        Weff = torch.tensor(popn.W_eff(x), dtype=f64, device=dev)
        A = torch.empty((N, P, P), dtype=f64, device=dev)
        h.hvp_prepare(st.data_ptr(), Weff.data_ptr(), 0, N)
        h.hess(A.data_ptr(), P)
        h.newton_assemble_dev(st.data_ptr(), N, P, 0, N, A.data_ptr(), P, prm)
        stream.synchronize()
        t0 = time.perf_counter()
        scale, _, info = h.chol_factor(A)
        stream.synchronize()
        out = {'P': int(P), 'rows': int(N), 'factor_s': time.perf_counter() - t0, 'failed_rows': int((info != 0).sum().item())}
        b = torch.randn((N, P), dtype=f64, device=dev)
        xs = torch.empty_like(b)
        ts = []
        for _ in range(reps):
            stream.synchronize()
            t0 = time.perf_counter()
            h.chol_solve(A, scale, info, b, out=xs)
            stream.synchronize()
            ts.append(time.perf_counter() - t0)
        out['chol_solve_s'] = float(np.median(ts))
        ts = []
        y, z = torch.empty_like(b), torch.empty_like(b)
        for _ in range(max(1, reps // 2)):
            Li = A.clone()
            stream.synchronize()
            t0 = time.perf_counter()
            h.tri_inverse(Li, info)
            bs = b / scale
            h.tri_matvec_dev(Li.data_ptr(), N, P, 0, bs.data_ptr(), y.data_ptr())
            h.tri_matvec_dev(Li.data_ptr(), N, P, 1, y.data_ptr(), z.data_ptr())
            zs = z / scale
            stream.synchronize()
            ts.append(time.perf_counter() - t0)
        out['inverse_route_s'] = float(np.median(ts))
        ok = (info == 0)
        d = (zs - xs)[ok]
        out['routes_differ_rel'] = float((d.abs().max() / xs[ok].abs().max()).item()) if bool(ok.any()) else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='C2,C3')
    ap.add_argument('--budget-s', type=float, default=900.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'newton_bench.json'))
    args = ap.parse_args()
    deadline = time.perf_counter() + args.budget_s
    res = {'tool': 'tools/newton_bench.py', 'configs': {}}

    def save():
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write('\n')

    for name in args.configs.split(','):
        N, nT = CONFIGS[name]
        popn = population(N, nT)
        out = res['configs'][name] = {'N': N, 'nT': nT, 'P': int(popn.glm.P) if hasattr(popn.glm, 'P') else None, 'starts': {}}
        try:
            x0 = popn.sample(np.random.RandomState(4321))
            fit('bfgs', popn, x0)                               # (warms the handle and the streams up)
            starts = {}
            for sname in ('sample', 'bfgs_fit'):
                srec = out['starts'][sname] = {}
                xs = x0 if sname == 'sample' else starts['bfgs_fit']
                fb = None
                for kind in ('bfgs', 'newton', 'newton_cg'):
                    if time.perf_counter() > deadline:
                        srec[kind] = 'skipped: wall budget'
                        continue
                    rec, xf, f = fit(kind, popn, xs)
                    if kind == 'bfgs':
                        fb = f
                        if sname == 'sample':
                            starts['bfgs_fit'] = xf
                    rec['f_minus_bfgs_f'] = q3(f - fb) if fb is not None else None
                    srec[kind] = rec
                    print(name, sname, kind, json.dumps(rec), flush=True)
                    save()
                if 'bfgs_fit' not in starts:
                    break
            if time.perf_counter() <= deadline and 'bfgs_fit' in starts:
                out['solve_alone'] = solve_alone(popn, starts['bfgs_fit'])
                print(name, 'solve_alone', json.dumps(out['solve_alone']), flush=True)
            else:
                out['solve_alone'] = 'skipped: wall budget'
            save()
        finally:
            popn.release_data()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
