"""Every kernel instantiation the Hessian-vector products can reach, run against a float64 reference.

tests/hvp_cases.json (tools/reachable_kernels.py --emit-hvp-cases; tests/test_hvp_cases.py keeps it complete) holds one
cheap case per reachable (prepare sequence, apply sequence) and, for every column pair of k_hvp5, one case per form of
call: `ring` (every workgroup walks three time tiles -- checked against the handle's own chunk count, pgl_info[2] -- on
a ragged sub-range), `list` (a permuted, non-contiguous neuron list), `trange` (t_lo > 0, t_hi not a multiple of 16),
`dstim` (dense stimulus columns, >= 65 neurons, automatic dispatch) -- the last three at no more than one tile per
workgroup -- and one `short` recording of 11 bins.

Per case, on the seeded data sets of tests/test_gpu_dispatch_sweep.py (explinear and exp in turn, a weighted Weff for
half of them, currents within 6 of the bias): prepare + apply through device pointers with kernel recording on -- the
launches of each must be the dry run's --, H v written over NaN, a second apply bit-identical, the one-shot pgl_hvp equal
to the two-step form.  Edge neurons of the evaluated rows: the first at bias 12 (explinear) / 3 (exp), the last at -20, and
in ranges of four or more one at -2 (spike data do not depend on theta: spiking bins meet all three explinear branches
of pgl_curvature, asserted from the reference currents over the sweep).  V: standard normal, one row zero, one row the unit
bias vector.

Reference: F^T (c o (F v)) in numpy float64 with tests/hvp_reference.curvature_stable (held to mpmath at 1e-12 per bin in
tests/test_hvp_reference.py; cross-checked here on the edge rows' own currents where mpmath is importable).  Bound: every
row's error against that row's own max|H v|: 1e-9 (the gradient's bound, README "Parity status"); with f32 feature tiles
(PGL_OPT_FEATURE_F32 = 1) the larger of 1e-9 and twice the first-order rounding bound of the stored features,
2 . 2^-24 max_k [|F|^T (|c| o (|F| |v|))]_k / max|H v|, from the reference alone."""
import json
import os
import time

import numpy as np
import pytest

from tests import hvp_reference as R
from tests.test_gpu_dispatch_sweep import _Data, _edge_biases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('N', 'B', 'R', 'Dstim', 'nT', 'n_lo', 'count', 'opt_kernel', 'opt_f32', 'list', 't_lo', 't_hi')
TOL = 1e-9


def _cases():
    with open(os.path.join(ROOT, 'tests', 'hvp_cases.json')) as f:
        return json.load(f)


def _label(c):
    return '%s: %s at %s' % (c['role'], ' + '.join(sorted(set(c['prepare'] + c['apply']))),
                             ' '.join('%s=%d' % (k, c[k]) for k in FIELDS))


def _family(c):
    k = c['apply'][0]
    fam = k.split('<')[0]
    if fam == 'k_fused2':
        fam += ' f32' if k.endswith('float>') else ''
        fam += ' (%s)' % ('one slice' if len(c['prepare']) == 1 else 'column slices')
    return fam


def _neurons(c, i):
    if not c['list']:
        return np.arange(c['n_lo'], c['n_lo'] + c['count'])
    ids = np.random.RandomState(900 + i).permutation(c['N'])[:c['count']]
    assert np.any(np.diff(ids) != 1)
    return ids


def _theta_rows(d, ids, i):
    """the rows of the evaluated neurons with their edge biases (module docstring), in the order of `ids`"""
    th = d.theta[ids].copy()
    pos = _edge_biases(np.zeros((len(ids), 1)) + np.nan, 0, len(ids), d.kind, i)[:, 0]     # by position in the call
    th[:, 0] = np.where(np.isnan(pos), th[:, 0], pos)
    if len(ids) >= 4:
        th[2, 0] = -2.0
    return th


def _vectors(count, P, i):
    V = np.random.RandomState(500 + i).standard_normal((count, P))
    if count >= 2:
        V[count // 2] = 0.0
    if count >= 3:
        V[count // 2 - 1] = 0.0
        V[count // 2 - 1, 0] = 1.0
    return V


def _tensor(torch, a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device='cuda')


def _run_case(c, i, d, stats, met):
    import torch
    from theano_pyglm_amd import _lib
    p, dev = d.p, d.dev
    ids = _neurons(c, i)
    th = _theta_rows(d, ids, i)
    V = _vectors(len(ids), th.shape[1], i)
    dev.set_option(_lib.OPT_KERNEL, c['opt_kernel'])
    dev.set_option(_lib.OPT_FEATURE_F32, c['opt_f32'])
    dev.set_time_range(c['t_lo'], c['t_hi'])
    ran = set()
    try:
        pair = [n for n in c['apply'] if n.startswith('k_hvp5<')]
        if pair:                                       # time tiles per workgroup from the handle's own plan
            tiles = (c['t_hi'] + 15) // 16 - c['t_lo'] // 16
            chunks = int(dev.info(int(ids.min()) if not c['list'] else 0,
                                  (int(ids.max()) + 1) if not c['list'] else len(ids))['chunks'])
            tpc = -(-tiles // chunks)
            per_wg = [min(tpc, tiles - k * tpc) for k in range(-(-tiles // tpc))]
            if c['role'] == 'ring':
                assert min(per_wg) >= 3, (_label(c), chunks, per_wg[-3:])
            elif c['role'] != 'base':
                assert max(per_wg) <= 1, (_label(c), chunks)
        d_th, d_W, d_v = _tensor(torch, th), _tensor(torch, p.Weff), _tensor(torch, V)
        d_hv = torch.full(V.shape, float('nan'), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        if c['list']:
            d_idx = _tensor(torch, ids, torch.int32)
            torch.cuda.synchronize()
            dev.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), d_idx=d_idx.data_ptr(), count=len(ids))
        else:
            dev.hvp_prepare(d_th.data_ptr(), d_W.data_ptr(), c['n_lo'], c['n_lo'] + c['count'])
        got_p = dev.last_kernels()
        dev.hvp_apply(d_v.data_ptr(), d_hv.data_ptr())
        dev.sync()
        got_a = dev.last_kernels()
        hv = d_hv.cpu().numpy().copy()
        ran.update(got_p + got_a)
        assert got_p == c['prepare'] and got_a == c['apply'], (_label(c), got_p, got_a)
        d_hv.fill_(float('nan'))
        torch.cuda.synchronize()
        dev.hvp_apply(d_v.data_ptr(), d_hv.data_ptr())
        dev.sync()
        assert np.array_equal(d_hv.cpu().numpy(), hv), _label(c) + ": a second apply differs"
        if not c['list']:
            one = dev.hvp(th, V, p.Weff, c['n_lo'], c['n_lo'] + c['count'])
            assert np.array_equal(one, hv), _label(c) + ": pgl_hvp differs from prepare + apply by %.2e" % np.max(np.abs(one - hv))
        ref, aref, xs, ss = R.ref_hvp(d.fS.reshape(p.nT, p.N, p.B), d.fstim, p.S, p.Weff, th, V, ids, d.kind, p.dt, c['t_lo'], c['t_hi'])
        if d.kind == 'explinear':
            for x, s in zip(xs, ss):
                xsp = x[s > 0]
                met['pos'] += int(np.sum(xsp >= 0.0))
                met['mid'] += int(np.sum((xsp < 0.0) & (np.exp(-np.abs(xsp)) >= 1.0e-2)))
                met['series'] += int(np.sum((xsp < 0.0) & (np.exp(-np.abs(xsp)) < 1.0e-2)))
        assert np.all(np.isfinite(hv)), _label(c) + ": not finite (NaN left in d_hv?)"
        scale = np.abs(ref).max(1)
        err = np.abs(hv - ref).max(1) / np.maximum(scale, 1e-300)
        tol = np.full(len(ids), TOL)
        if c['opt_f32'] == 1:
            tol = np.maximum(TOL, 2.0 * (2.0 * 2.0 ** -24 * aref.max(1) / np.maximum(scale, 1e-300)))
        fam = _family(c)
        stats[fam] = max(stats.get(fam, 0.0), float(np.max(err)))
        worst = int(np.argmax(err / tol))
        assert np.all(err <= tol), "%s (%s): row %d (neuron %d, bias %.1f): %.2e of its max|Hv| = %.2e (allowed %.1e); rows over: %s" % (
            _label(c), d.kind, worst, ids[worst], th[worst, 0], err[worst], scale[worst], tol[worst],
            np.nonzero(err > tol)[0].tolist())
    finally:
        dev.set_option(_lib.OPT_KERNEL, 0)
        dev.set_option(_lib.OPT_FEATURE_F32, 0)
        dev.set_time_range(0, p.nT)
    return ran, (xs, ss)


def _mp_crosscheck(kind, dt, xs, ss, n=40):
    """curvature_stable against mpmath on currents the sweep itself produced (skipped where mpmath is missing)"""
    try:
        import mpmath  # noqa: F401
    except ImportError:
        return None
    worst = 0.0
    for x, s in zip(xs, ss):
        sel = np.concatenate((np.nonzero(s > 0)[0][:n], np.arange(min(n, len(x)))))
        got = R.curvature_stable(x[sel], s[sel], kind, dt)
        for xi, si, g in zip(x[sel], s[sel], got):
            c = R.curvature_mp(xi, si, kind, dt, dps=80)
            worst = max(worst, float(abs((g - c) / c)))
    return worst


def test_every_hvp_instantiation_against_the_reference():
    cases = _cases()
    groups = {}
    for c in cases:
        groups.setdefault((c['N'], c['B'], c['R'], c['Dstim'], c['nT'], 0), []).append(c)
    ran, stats, failed = set(), {}, []
    met = {'pos': 0, 'mid': 0, 'series': 0}
    index = dict((id(c), i) for i, c in enumerate(cases))
    mp_worst, t0 = None, time.time()
    for g, key in enumerate(sorted(groups)):
        if g % 50 == 0:                               # (a sign of life: the sweep prints nothing else until its end)
            print("hvp sweep: data set %d of %d, %.0f s" % (g, len(groups), time.time() - t0), flush=True)
        d = _Data(key, g)
        try:
            for c in groups[key]:
                try:
                    r, (xs, ss) = _run_case(c, index[id(c)], d, stats, met)
                    ran |= r
                    if c['role'] == 'ring':          # edge rows (first, -2, last) of the long cases
                        w = _mp_crosscheck(d.kind, d.p.dt, [xs[0], xs[2], xs[-1]], [ss[0], ss[2], ss[-1]])
                        if w is not None:
                            mp_worst = max(mp_worst or 0.0, w)
                except AssertionError as e:          # (every failing case in one report)
                    failed.append(str(e))
        finally:
            d.close()
    table = set(n for c in cases for n in c['prepare'] + c['apply'])
    hvp5 = sorted(n for n in ran if n.startswith('k_hvp5<'))
    print("\nspiking explinear bins by branch of pgl_curvature: %s; curvature_stable against mpmath on the sweep's currents: %s"
          % (met, 'mpmath missing' if mp_worst is None else '%.2e' % mp_worst))
    for fam in sorted(stats):
        print("  %-34s worst row error (of the row's max|Hv|) %.2e" % (fam, stats[fam]))
    print("hvp sweep: %d cases in %.0f s, %d instantiations run (table: %d), k_hvp5: %d"
          % (len(cases), time.time() - t0, len(ran), len(table), len(hvp5)))
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(cases), "\n".join(failed))
    assert mp_worst is None or mp_worst <= 1e-12
    assert min(met.values()) > 0, met
    assert ran == table, "not run: %s; run but not in the table: %s" % (sorted(table - ran), sorted(ran - table))
    assert len(hvp5) == 14, hvp5
