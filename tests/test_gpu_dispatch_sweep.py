"""Every fused kernel instantiation the dispatcher can reach, run at least once against the oracle.

tests/dispatch_cases.json holds one cheap case per reachable instantiation (tools/reachable_kernels.py --emit-cases;
tests/test_dispatch_cases.py keeps it complete).  For each case: a seeded problem of that shape -- explinear and exp, a
weighted Weff for half of the data sets, dense / separable stimulus as the case says -- evaluated with kernel recording on
(PGL_OPT_RECORD_KERNELS): the launches the evaluation actually made must be the dry run's (pgl_plan_kernels), and the
results must match the C oracle at the suite's tolerances, the gradient row by row (each neuron's error against its own
largest gradient entry).  Edge neurons: the first evaluated neuron sits at a high bias -- 12 for explinear, where the
single-precision correction of the rate epilogue switches on for waves whose currents all exceed 12, so the regimes mix
inside a wave; 3 for exp, rates up to e^9 / s -- and, in ranges of two or more neurons, the last one far below rate 1
(bias -20).  A one-neuron range takes the high bias or -20 in turn along the table.  The impulse / stimulus weights are
scaled so that every current stays within 6 of its bias."""
import json
import os

import numpy as np
import pytest

from tests import helpers as H
from oracle import c_oracle as CO
from oracle import glm_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('N', 'B', 'R', 'Dstim', 'nT', 'stim', 'n_lo', 'count', 'path', 'opt_kernel', 'opt_f32')
THREADS = 16
BT, DT_STIM = 3, 0.1              # separable stimulus: three temporal bases, frames of 100 bins (Dstim = BT + spatial bases)
OPT_SEPF = 94                     # dev option: 2 = tap-rate kernels (stim 1), 3 = stimulus current through the slab (stim 3)


def _cases():
    with open(os.path.join(ROOT, 'tests', 'dispatch_cases.json')) as f:
        return json.load(f)


def _basis(R, B):
    """B distinct impulse bases of R taps: the standard basis and delayed copies of it."""
    std = H.std_ibasis(R)
    cols = []
    for j in range(B):
        c = np.roll(std[:, j % std.shape[1]], 11 * (j // std.shape[1]))
        c[:11 * (j // std.shape[1])] = 0.0
        cols.append(c)
    return np.ascontiguousarray(np.stack(cols, axis=1))


class _Data(object):
    """One seeded data set (spikes, basis, Weff, stimulus) shared by the cases of the same shape, its handle and its
    oracle features."""

    def __init__(self, key, g):
        from theano_pyglm_amd import _lib
        N, B, R, Dstim, nT, stim = key
        self.kind = 'explinear' if g % 2 == 0 else 'exp'
        self.stim = stim
        dense = Dstim if stim == 0 else 0
        p = H.Problem(N, nT, _basis(R, B), kind=self.kind, Dstim=dense, seed=7000 + g, weighted=(g // 2) % 2 == 1,
                      w_scale=0.1)
        self.p = p
        self.fS = CO.features(p.S, p.ibasis)
        rng = np.random.RandomState(g)
        theta = p.theta
        if stim:                                   # [bias, w_t, w_x, w_imp] on the device, the dense w_t (x) w_x for the oracle
            Bx = Dstim - BT
            ibt = np.ascontiguousarray(H.golden()['lr2d_ibasis_t'][:, :BT])
            self.stim_frames = rng.randn(int(np.ceil(nT * p.dt / DT_STIM)) + 2, Bx)
            self.ibt = ibt
            self.fstim = O.spatiotemporal_stim_features(self.stim_frames, DT_STIM, p.dt, nT, np.eye(Bx), ibt)
            w_t, w_x = 0.3 * rng.randn(N, BT), 0.3 * rng.randn(N, Bx)
            I_st = np.einsum('tk,nk->tn', self.fstim, np.einsum('nt,nx->ntx', w_t, w_x).reshape(N, -1))
            w_x *= np.minimum(1.0, 3.0 / np.maximum(np.abs(I_st).max(0), 1e-300))[:, None]
            self.w_t, self.w_x = w_t, w_x
            theta = np.concatenate((theta[:, :1], np.einsum('nt,nx->ntx', w_t, w_x).reshape(N, -1), theta[:, 1:]), axis=1)
        else:
            self.fstim = p.fstim
        D = theta.shape[1] - 1 - N * B
        # impulse currents of every neuron (one GEMM), weights scaled so that |I_net + I_stim| <= 6
        Wc = (theta[:, 1 + D:].reshape(N, N, B) * p.Weff.T[:, :, None]).reshape(N, N * B)
        I = self.fS.reshape(nT, N * B).dot(Wc.T)
        if D:
            I_s = self.fstim.dot(theta[:, 1:1 + D].T)
            s_st = np.minimum(1.0, 3.0 / np.maximum(np.abs(I_s).max(0), 1e-300))
            theta[:, 1:1 + D] *= s_st[:, None]
            if stim:
                self.w_x *= s_st[:, None]
        s_imp = np.minimum(1.0, 3.0 / np.maximum(np.abs(I).max(0), 1e-300))
        theta[:, 1 + D:] *= s_imp[:, None]
        self.theta = theta                           # dense layout (the oracle's)
        self.D = D
        self.dev = p.device()
        try:
            if stim:
                self.dev.set_stimulus_separable(self.stim_frames, DT_STIM, self.ibt)
            self.dev.set_option(_lib.OPT_RECORD_KERNELS, 1)
        except Exception:
            self.dev.close()
            raise

    def device_theta(self, th):
        """all N dense rows -> the handle's layout (separable: [bias, w_t, w_x, w_imp])"""
        if not self.stim:
            return th
        return np.concatenate((th[:, :1], self.w_t, self.w_x, th[:, 1 + self.D:]), axis=1)

    def chain(self, g, lo, hi):
        """oracle gradient (dense stimulus weights) -> the separable layout, rows [lo, hi)"""
        if not self.stim:
            return g
        Bx = self.w_x.shape[1]
        G = g[:, 1:1 + self.D].reshape(-1, BT, Bx)
        return np.concatenate((g[:, :1], np.einsum('ntx,nx->nt', G, self.w_x[lo:hi]),
                               np.einsum('ntx,nt->nx', G, self.w_t[lo:hi]), g[:, 1 + self.D:]), axis=1)

    def close(self):
        self.dev.close()


def _edge_biases(th, lo, hi, kind, i):
    """case i of the table evaluates [lo, hi): its edge neurons (see the module docstring)"""
    th = th.copy()
    high = (12.0, 11.5) if kind == 'explinear' else (3.0, 2.5)
    th[lo, 0] = high[0] if hi - lo >= 2 or i % 2 == 0 else -20.0
    if hi - lo >= 2:
        th[hi - 1, 0] = -20.0                      # rate far below 1
    if hi - lo >= 3:
        th[lo + 1, 0] = high[1]
    return th


def _row_err(g, g0):
    """largest gradient error of a row relative to the row's own largest entry, over the rows"""
    return float(np.max(np.abs(g - g0).max(1) / np.maximum(np.abs(g0).max(1), 1e-300)))


def _label(c):
    return ' + '.join(sorted(set(c['names']))) + ' at ' + ' '.join('%s=%d' % (k, c[k]) for k in FIELDS)


def _f32_ll_bound(d, th, lo, hi):
    """Per neuron of [lo, hi): the first-order bound of what storing the features in f32 can do to the ll,
    2^-24 sum_t |d ll / d x_t| sum_k |F_tk w_k|, relative to |ll|.  Above 1e-8 only where the ll is ill-conditioned
    (an exp neuron whose ll terms nearly cancel against 200 dense stimulus columns)."""
    p = d.p
    F = d.fS.reshape(p.nT, -1)
    out = []
    for n in range(lo, hi):
        w = (th[n, 1 + d.D:].reshape(p.N, p.B) * p.Weff[:, n][:, None]).ravel()
        x, a = F.dot(w) + th[n, 0], np.abs(F).dot(np.abs(w))
        if d.D:
            x, a = x + d.fstim.dot(th[n, 1:1 + d.D]), a + np.abs(d.fstim).dot(np.abs(th[n, 1:1 + d.D]))
        r = O.glm_resid(x, p.S[:, n].astype(float), p.dt, d.kind)
        out.append(2.0 ** -24 * np.sum(np.abs(r) * a) / abs(O.glm_ll_from_x(x, p.S[:, n], p.dt, d.kind)))
    return np.array(out)


def _run_case(c, i, d, stats):
    from theano_pyglm_amd import _lib
    p, dev = d.p, d.dev
    lo, hi = c['n_lo'], c['n_lo'] + c['count']
    th = _edge_biases(d.theta, lo, hi, d.kind, i)
    th_dev = d.device_theta(th)
    dev.set_option(_lib.OPT_KERNEL, c['opt_kernel'])
    dev.set_option(_lib.OPT_FEATURE_F32, c['opt_f32'])
    dev.set_option(OPT_SEPF, {0: 0, 1: 2, 2: 0, 3: 3}[c['stim']])
    fam = c['names'][0].split('<')[0]
    ran = set()
    try:
        if c['path'] == 2:
            dev.gibbs_prepare_all(th_dev, p.Weff)
            got = dev.last_kernels()
            ran.update(got)
            assert got == c['names'], (_label(c), got)
            err = 0.0
            for n in range(p.N):
                w = th[n, 1 + d.D:].reshape(p.N, p.B)
                x0, _, _ = O.glm_currents(n, d.fS, w, p.Weff[:, n], th[n, 0], d.fstim,
                                          th[n, 1:1 + d.D] if d.D else None)
                x = dev.gibbs_currents(n)
                err = max(err, float(np.max(np.abs(x - (x0 - th[n, 0])))))
            assert err < 1e-10, (_label(c), err)
            s = stats.setdefault(fam + ' (Gibbs)', [0.0, 0.0])
            s[1] = max(s[1], err)
            return ran
        ll, g = dev.ll_grad(th_dev[lo:hi], p.Weff, lo, hi)
        got = dev.last_kernels()
        ran.update(got)
        ll1, _ = dev.ll_grad(th_dev[lo:hi], p.Weff, lo, hi, want_grad=False)
        got1 = dev.last_kernels()
        ran.update(got1)
        assert (got if c['path'] == 0 else got1) == c['names'], (_label(c), got, got1)
        if c['stim'] >= 2:
            # (the frame-rate ll-only call runs another forward kernel: k_fused7<.., 2> instead of <.., 3>)
            assert np.allclose(ll1, ll, rtol=1e-13, atol=0), _label(c)
        else:
            assert np.array_equal(ll1, ll), _label(c)
        ll0, g0 = CO.ll_grad(p.S, d.fS, th[lo:hi], p.Weff, d.kind, p.dt, lo, hi, d.fstim, threads=THREADS)
        g0 = d.chain(g0, lo, hi)
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(g)), _label(c)
        ref_ll, ref_g = ll0, g0
        ll_tol, g_rtol = np.full(len(ll), 1e-10), 1e-9
        if c['opt_f32'] == 1:
            # f32 feature tiles: 1e-8 (test_f32_feature_staging), or twice the rounding bound of a neuron whose ll is
            # ill-conditioned beyond that -- each neuron against its own bound
            ll_tol, g_rtol = np.maximum(1e-8, 2.0 * _f32_ll_bound(d, th, lo, hi)), 1e-6
        if c['opt_f32'] == 2:
            # f32 resident blocks: 1e-6 from the f64 path of the same handle (which is held to the f64 bounds)
            dev.set_option(_lib.OPT_FEATURE_F32, 0)
            ref_ll, ref_g = dev.ll_grad(th_dev[lo:hi], p.Weff, lo, hi)
            assert np.allclose(ref_ll, ll0, rtol=1e-10, atol=0) and _row_err(ref_g, g0) < 1e-9, _label(c)
            ll_tol, g_rtol = np.full(len(ll), 1e-6), 1e-6
        rel_ll = np.abs(ll - ref_ll) / np.abs(ref_ll)
        e_ll, e_g = float(np.max(rel_ll)), _row_err(g, ref_g)
        blocks = [(0, 1), (1, g.shape[1] - p.N * p.B), (g.shape[1] - p.N * p.B, g.shape[1])]
        assert np.all(rel_ll <= ll_tol) and e_g < g_rtol, \
            "%s (%s): ll %.2e (allowed %.1e), gradient %.2e (bias / stimulus / impulse blocks %s)" % (
                _label(c), d.kind, e_ll, float(ll_tol[np.argmax(rel_ll / ll_tol)]), e_g,
                ['%.1e' % (_row_err(g[:, a:b], ref_g[:, a:b]) if b > a else 0.0) for a, b in blocks])
        if d.stim:                                 # each block of the separable layout on its own scale
            Bx = d.w_x.shape[1]
            for sl in (slice(0, 1), slice(1, 1 + BT), slice(1 + BT, 1 + BT + Bx), slice(1 + BT + Bx, None)):
                assert H.rel_err(g[:, sl], g0[:, sl]) < g_rtol, (_label(c), sl)
        key = fam + (' f32=%d' % c['opt_f32'] if c['opt_f32'] else '')
        s = stats.setdefault(key, [0.0, 0.0])
        s[0], s[1] = max(s[0], e_ll), max(s[1], e_g)
    finally:
        dev.set_option(_lib.OPT_KERNEL, 0)
        dev.set_option(_lib.OPT_FEATURE_F32, 0)
        dev.set_option(OPT_SEPF, 0)
    return ran


def test_every_dispatchable_instantiation_against_the_oracle():
    cases = _cases()
    groups = {}
    for c in cases:
        groups.setdefault(tuple(c[k] for k in ('N', 'B', 'R', 'Dstim', 'nT', 'stim')), []).append(c)
    ran, stats, failed = set(), {}, []
    index = dict((id(c), i) for i, c in enumerate(cases))
    for g, key in enumerate(sorted(groups)):
        d = _Data(key, g)
        try:
            for c in groups[key]:
                try:
                    ran |= _run_case(c, index[id(c)], d, stats)
                except AssertionError as e:          # (every failing case in one report)
                    failed.append(str(e))
        finally:
            d.close()
    table = set(n for c in cases for n in c['names'])
    print("\ndispatch sweep: %d cases, %d instantiations run (table: %d)" % (len(cases), len(ran), len(table)))
    for fam in sorted(stats):
        print("  %-18s worst ll rel err %.2e   worst grad err (of the row's max|g|; Gibbs: current abs) %.2e"
              % (fam, stats[fam][0], stats[fam][1]))
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(cases), "\n".join(failed))
    assert ran == table, "not run: %s; run but not in the table: %s" % (sorted(table - ran), sorted(ran - table))
