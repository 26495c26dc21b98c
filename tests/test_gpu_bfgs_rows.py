"""GPU tests of the lock-step BFGS row kernels (csrc/pglm_bfgs.hip.h) against the plain numpy reference of
tests/bfgs_reference.py, launch by launch.  pgl_bfgs_step_dev runs with prior kind < 0, so f and g come from numpy and
no ll+grad launch is involved; the handle only supplies the device and the stream.

A. One launch from an uploaded synthetic state (the cases of bfgs_reference.CASES), in the three forms the driver can
   choose -- one kernel (k_bfgs_step<1024>), split implicit (k_bfgs_hdots + k_bfgs_hcomb) and dense (k_bfgs_hmul) -- each
   against the reference, never against each other.  Every real number within its own derived rounding bound
   (8 n 2^-53 m, n terms, m the sum of their absolute values), alpha and the line-search block within the span the bound
   of dp allows, every flag and counter exactly, every entry the launch has no business with bit-identical.
B. Free-running fits of three convex objectives (P = 26, 71, 261; M = 3) from pgl_bfgs_init_dev to the end in the three
   forms: the decision record of every launch equals the reference's, the final X and f lie within 16 x the spread of the
   reference's own two orderings of the sums.
C. pgl_bfgs_init_dev and pgl_bfgs_trial_dev on their own."""
import numpy as np
import pytest

from tests import bfgs_reference as R
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(3, 200, H.std_ibasis()[:, :2], Dstim=2, seed=5).device(0)
    yield h
    h.close()


def _close(dev, ref, tol, what):
    """entries with tolerance 0 bit-identical, the others within their tolerance (inf: no contract)"""
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    tol = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)).reshape(-1)
    dev, ref = np.ascontiguousarray(dev, dtype=np.float64).reshape(-1), ref.reshape(-1)
    assert dev.size == ref.size
    exact = tol == 0
    same = dev.view(np.int64) == ref.view(np.int64)
    bad = np.nonzero(exact & ~same)[0]
    assert bad.size == 0, "%s: %d entries that must be bit-identical differ, first %d: %r != %r" % (
        what, bad.size, bad[0], dev[bad[0]], ref[bad[0]])
    k = ~exact & np.isfinite(tol)
    with np.errstate(all='ignore'):
        d = np.abs(dev[k] - ref[k])
        ratio = d / tol[k]
    worst = float(np.max(ratio)) if ratio.size else 0.0
    assert not np.any(np.isnan(d)) and worst <= 1.0, "%s: %.3g x its rounding bound (entry %d of the compared ones)" % (
        what, worst, int(np.argmax(ratio)) if ratio.size else -1)
    return worst


class Dev(object):
    """the device side of one optimiser: the state block, the history or the dense matrices, the launch arguments"""

    def __init__(self, handle, st, form):
        import torch
        self.t, self.h, self.form = torch, handle, form
        self.dev = torch.device('cuda', 0)
        self.M, self.P = st.M, st.P
        self.state = self.up(R.pack(st))
        self.Kmax, self.ld = st.Kmax, st.ld
        self.hist = self.coef = self.ab = self.Hd = None
        if form == 'dense':
            self.Hd = self.up(st.Hd)
        else:
            self.hist, self.coef = self.up(st.hist), self.up(st.coef)
            self.ab = self.up(np.full((st.M, st.Kmax, 2), 1e30))
        self.flags = torch.full((st.M,), -3.0, dtype=torch.float64).pin_memory()

    def up(self, a, dtype=None):
        return self.t.tensor(np.ascontiguousarray(a), dtype=dtype or self.t.float64, device=self.dev)

    def step(self, rows, Xt, f, g, hk_bound, max_trials, gtol, maxiter, init_scaling, pos_next=None, L_next=None,
             sentinel=np.nan, **_):
        t = self.t
        L = len(f)
        d_rows = self.up(rows, t.int32) if rows is not None else None
        d_pos = self.up(pos_next, t.int32) if pos_next is not None else None
        Xn = t.full((L if L_next is None else L_next, self.P), sentinel, dtype=t.float64, device=self.dev)
        Xd, fd, gd = self.up(Xt), self.up(f), self.up(g)
        t.cuda.synchronize()
        ptr = lambda x: x.data_ptr() if x is not None else 0
        self.h.bfgs_step_dev(self.state.data_ptr(), self.M, self.P, ptr(d_rows), L, Xd.data_ptr(), fd.data_ptr(), gd.data_ptr(),
                             None, max_trials, gtol, maxiter, init_scaling, ptr(self.hist), ptr(self.coef), self.Kmax,
                             ptr(self.ab), hk_bound, ptr(self.Hd), self.ld if self.Hd is not None else 0, ptr(d_pos),
                             Xn.data_ptr(), self.flags.data_ptr())
        self.h.sync()
        assert np.array_equal(fd.cpu().numpy(), f, equal_nan=True) and np.array_equal(gd.cpu().numpy(), g)   # final: not touched
        return Xn.cpu().numpy()


def _with_form(handle, form, fn):
    from theano_pyglm_amd import _lib
    if form != 'split':
        return fn()
    handle.set_option(_lib.OPT_BFGS_MERGE, 0)
    try:
        return fn()
    finally:
        handle.set_option(_lib.OPT_BFGS_MERGE, 65536)


# ---- A -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('name', [c['name'] for c in R.CASES])
def test_one_launch_from_an_uploaded_state(handle, name, form):
    st0, args, spec, st1, out = R.run_case(name, form)
    assert R.valid(out['decisions']), "the case is not valid: a decision hangs on rounding"
    for d, e in zip(out['decisions'], R.expected_decisions(spec)):
        assert all(d[k] == v for k, v in e.items()), (d, e)
    assert spec['hk_bound'] >= 1 and R.KMAX > spec['hk_bound']
    dv = Dev(handle, st0, form)
    Xn = _with_form(handle, form, lambda: dv.step(hk_bound=spec['hk_bound'], **args))
    got = dv.state.cpu().numpy()
    worst = {}
    ref, tol = R.pack(st1), R.pack_tol(st1)
    # field by field, so that a failure names its field
    o = 0
    M, P = st0.M, st0.P
    for nm, sz in [(n, M * P) for n in R.VEC] + [('U', 3 * M * P), ('V', 3 * M * P)] + [(n, M) for n in R.SCAL] + \
                  [('ls.' + n, M) for n in R.LSF]:
        worst[nm] = _close(got[o:o + sz], ref[o:o + sz], tol[o:o + sz], '%s/%s: %s' % (name, form, nm))
        o += sz
    assert o == got.size
    for nm in R.FLAGS + tuple('ls.' + n for n in R.LS_FLAGS):
        assert worst[nm] == 0.0                               # (compared bit for bit above: their tolerance is 0)
    if form == 'dense':
        worst['H'] = _close(dv.Hd.cpu().numpy(), st1.Hd, st1.tol['Hd'] if 'Hd' in st1.tol else 0.0, '%s/%s: dense H' % (name, form))
    else:
        for nm, d_, r_ in (('hist', dv.hist, st1.hist), ('coef', dv.coef, st1.coef)):
            worst[nm] = _close(d_.cpu().numpy(), r_, st1.tol[nm] if nm in st1.tol else 0.0, '%s/%s: %s' % (name, form, nm))
        ab, used = dv.ab.cpu().numpy(), np.zeros((M, R.KMAX), dtype=bool)
        for r, K in out['ab'].items():
            used[r, :K] = True
        assert np.all(np.isfinite(ab[used])) and np.all(ab[~used] == 1e30)       # the scratch: written where a product ran only
    worst['Xt_next'] = _close(Xn, out['Xt_next'], out['Xt_next_tol'], '%s/%s: Xt_next' % (name, form))
    flags = dv.flags.numpy()
    for r in range(M):
        assert flags[r] == (out['active'][r] if r in out['active'] else -3.0), (r, flags)
    print("%s/%s: worst fraction of the rounding bound: %s" % (
        name, form, ', '.join('%s %.2g' % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1])[:6])))


# ---- B -----------------------------------------------------------------------------------------------------------------
GTOL_B, MAXITER_B = 1e-4, 60


def _objective(P, seed):
    """M = 3 convex rows: a quadratic of three distinct curvatures in [1, 100] plus a quartic (no pure quadratic: its searches
    end on the exact minimiser, dp = 0 up to rounding), started at different distances so that they finish at different
    launches"""
    rng = np.random.default_rng(seed)
    D = rng.choice(np.array([1.0, 10.0, 100.0]), size=(3, P))
    c = rng.standard_normal((3, P))
    q = np.array([0.1, 0.3, 1.0])
    X0 = c + np.array([0.02, 0.1, 0.4])[:, None] * rng.standard_normal((3, P))

    def fun(r, x):
        d = x - c[r]
        return float(0.5 * np.sum(D[r] * d * d) + 0.25 * q[r] * np.sum(d ** 4)), D[r] * d + q[r] * d ** 3

    return fun, X0


SEEDS_B = {26: 2, 71: 1, 261: 1}             # chosen on the CPU: margins clear, both reference runs decide alike, <= 48 launches
_REF_FITS = {}


def _ref_fit(P, form):
    key = (P, 'dense' if form == 'dense' else 'hist')
    if key not in _REF_FITS:
        fun, X0 = _objective(P, SEEDS_B[P])
        kw = dict(gtol=GTOL_B, maxiter=MAXITER_B, init_scaling=0, form=key[1])
        _REF_FITS[key] = (fun, X0, R.fit(fun, X0, sums='ld', **kw), R.fit(fun, X0, sums='f64', **kw))
    return _REF_FITS[key]


def _device_fit(handle, fun, X0, form):
    """the same driver loop on the device: (X, f, record of every launch)"""
    M, P = X0.shape
    st = R.State(M, P, 'dense' if form == 'dense' else 'hist', MAXITER_B, P + (P & 1))
    st.X[:] = X0
    for r in range(M):
        st.f[r], st.g[r] = fun(r, X0[r])
    dv = Dev(handle, st, form)                                   # (the dense buffer goes up filled with NaN)
    handle.bfgs_init_dev(dv.state.data_ptr(), M, P, GTOL_B)
    handle.sync()
    st = R.unpack(dv.state.cpu().numpy(), M, P)
    rows = [r for r in range(M) if st.active[r] != 0]
    Xt = st.X[rows] + st.alpha[rows][:, None] * st.p[rows]
    record, launches = [], 0
    while rows:
        assert launches < 3 * MAXITER_B
        fg = [fun(r, Xt[j]) for j, r in enumerate(rows)]
        f, g = np.array([v[0] for v in fg]), np.stack([v[1] for v in fg])
        before = st
        Xn = _with_form(handle, form, lambda: dv.step(rows, Xt, f, g, hk_bound=launches, max_trials=100, gtol=GTOL_B,
                                                      maxiter=MAXITER_B, init_scaling=0))
        st = R.unpack(dv.state.cpu().numpy(), M, P)
        rec = []
        for j, r in enumerate(rows):
            # the return code that the device's own state before the launch and its own dp imply (host line search), and the
            # source of the point it holds now
            rc = R.ls_step(before.ls[:, r], f[j], float(np.dot(g[j], before.p[r])))[0]
            taken = st.iters[r] != before.iters[r]
            src = 0 if not taken else (1 if np.array_equal(st.X[r], Xt[j]) else (2 if np.array_equal(st.X[r], before.Xb[r]) else -1))
            assert (rc == R.EVALUATE) == (not taken), (launches, r, rc)
            assert float(dv.flags[r]) == st.active[r]
            rec.append((rc, src, int(st.active[r]), int(st.iters[r]), int(st.nfev[r]), int(st.hk[r])))
        record.append((tuple(rows), rec))
        keep = [j for j, r in enumerate(rows) if st.active[r] != 0]
        rows, Xt = [rows[j] for j in keep], Xn[keep]
        launches += 1
    return st.X.copy(), st.f.copy(), record


@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('P', [26, 71, 261])
def test_free_running_fit_follows_the_reference(handle, P, form):
    """Tolerance, measured on the reference alone: the spread between its run with longdouble sums and its run with plain
    float64 np.dot sums (the same decisions in both, asserted), times 16 -- 4 for the device's own reduction tree, 4 for the
    number of forms.  Measured spread of the final X: 6.7e-11 (P = 26, 27 launches; dense 2.3e-11), 1.0e-11 (P = 71, 28
    launches), 2.8e-9 (P = 261, 42 launches); of f: 2.6e-16, 4.5e-19 and 2.6e-16 (dense 8.8e-16).  Printed by the test."""
    fun, X0, (st1, _, log1, rec1), (st2, _, _, rec2) = _ref_fit(P, form)
    assert all(R.valid(decs) for decs in log1), "a decision of the reference's run hangs on rounding: choose another seed"
    assert rec1 == rec2, "the reference's own two runs decide differently: choose another seed"
    ends = [max(k for k, (rows, _) in enumerate(rec1) if r in rows) for r in range(3)]
    assert len(set(ends)) == 3 and len(rec1) <= 48, (ends, len(rec1))         # rows finish at different launches
    spread_X = float(np.max(np.abs(st1.X - st2.X)))
    spread_f = np.abs(st1.f - st2.f)
    Xd, fd, recd = _device_fit(handle, fun, X0, form)
    print("P %d %s: %d launches, spread of X %.3e (tolerance %.3e), of f %s; device: X off by %.3e, f by %s"
          % (P, form, len(rec1), spread_X, 16 * spread_X, spread_f, np.max(np.abs(Xd - st1.X)), np.abs(fd - st1.f)))
    assert recd == rec1
    assert np.max(np.abs(Xd - st1.X)) <= 16 * spread_X
    assert np.all(np.abs(fd - st1.f) <= 16 * spread_f)


# ---- C -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 65, 257])
def test_init_and_trial_on_their_own(handle, P):
    M, gtol = 4, 1e-3
    rng = np.random.default_rng(900 + P)
    st = R.State(M, P, 'hist', 0, 0)
    for n in R.VEC:
        getattr(st, n)[:] = rng.standard_normal((M, P))
    st.U[:], st.V[:] = rng.standard_normal((M, P, 3)), rng.standard_normal((M, P, 3))
    st.g *= np.array([30.0, 1.0, 0.05, 1.0])[:, None]           # |g| > 1.01 (a first step below 1), ~1, small
    st.g[3] *= gtol / np.max(np.abs(st.g[3]))                    # max|g| <= gtol: this row never starts
    assert np.max(np.abs(st.g[3])) <= gtol
    st.f[:] = rng.standard_normal(M)
    for n in R.SCAL[1:]:
        getattr(st, n)[:] = -5.0                                 # every scalar must be written by the init
    st.ls[:] = -5.0
    ref = R.init_phase(st.copy(), gtol)
    nrm = np.sqrt(np.sum(st.g.astype(R.LD) ** 2, axis=1)).astype(np.float64)
    assert np.allclose(ref.alpha, np.minimum(1.0, 1.01 / nrm), rtol=1e-13, atol=0)
    assert np.allclose(ref.fprev, st.f + nrm / 2, rtol=1e-13, atol=0)
    assert list(ref.active) == [1.0, 1.0, 1.0, 0.0] and ref.alpha[0] < 1.0 and (P == 1 or ref.alpha[2] == 1.0)
    dv = Dev(handle, st, 'merged')
    handle.bfgs_init_dev(dv.state.data_ptr(), M, P, gtol)
    handle.sync()
    got = dv.state.cpu().numpy()
    w = _close(got, R.pack(ref), R.pack_tol(ref), 'init P=%d' % P)
    dst = R.unpack(got, M, P)
    assert np.array_equal(dst.active, ref.active) and np.array_equal(dst.ident, np.ones(M)) and not dst.hk.any()
    rows = [2, 0, 3]
    Xt = dv.t.full((len(rows), P), -7.0, dtype=dv.t.float64, device=dv.dev)
    handle.bfgs_trial_dev(dv.state.data_ptr(), M, P, dv.up(rows, dv.t.int32).data_ptr(), len(rows), Xt.data_ptr())
    handle.sync()
    Xr, Xtol = R.trial_phase(dst, rows)                          # from the device's own state: exact inputs
    w2 = _close(Xt.cpu().numpy(), Xr, Xtol, 'trial P=%d' % P)
    print("init P=%d: worst fraction of the rounding bound %.2g, trial %.2g" % (P, w, w2))
