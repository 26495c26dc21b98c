"""Plain numpy reference of the lock-step BFGS row kernels (test infrastructure, no GPU).

The algorithm is restated from its description -- include/pyglm_hip.h (the block above pgl_bfgs_state_doubles) and the
comments of csrc/pglm_bfgs.hip.h -- for one row at a time, in the order a launch of pgl_bfgs_step_dev runs its phases:

  line search   phi'(alpha) = g_trial . p, one step of the More'-Thuente machine (the host build of pglm_linesearch.h,
                tests/csrc/ls_host.c, pinned to scipy's DCSRCH by tests/test_optimizer_host.py).  EVALUATE: next trial step,
                the trial is saved as the best point when it became the best step.  CONVERGED: the row takes the trial.
                WARNING (also: f or the slope not finite, max_trials steps used up): the trial is taken when it is a
                sufficient decrease and not worse than the saved best point, else the saved best point when that is a
                sufficient decrease, else the row stalls.  A taken point leaves s, y, rho = 1 / s.y and upd = (s.y > 0).
  t = H g_new   for the rows that took a point.  The reference keeps the inverse Hessian approximation of every row as a real
                (P, P) matrix H (longdouble) and multiplies by it; the device holds either the update history
                (H = hscale I + sum_j U_j V_j^T, U_j = (c0 s, -rho Hy, -rho s), V_j = (s, s, Hy)) or a dense matrix with a
                pending rank-3 update -- by algebra the same matrix.
  update        H_new = (I - rho s y^T) H (I - rho y s^T) + rho s s^T = H + U V^T, H_new g_new, the next direction, restart
                (once) / freeze of a stalled row, H = I when the direction is not a descent direction, convergence
                (max|g| <= gtol, iters == maxiter), the start of the next search with scipy's first step.
  trial         Xt_next[pos_next[r]] = X[r] + alpha[r] p[r] for every listed row.

Sums are formed in np.longdouble (sums='ld'; sums='f64' uses plain float64 np.dot, for measuring how far two orderings of
the same sums drift apart).  Every real output carries a rounding bound in the manner of tests/test_gpu_prior.py: the
number of terms n of the longest summation chain that forms it and the sum m of the absolute values of its terms, inner
sums replaced by their absolute sums; a device value may differ by 8 n 2^-53 m.  The three sums that decisions hang on --
dp = g_trial . p, s.y and sl = -Hg . g -- get margins: the line-search step is repeated with dp moved by its bound (the
decisions must not change; the span of the next step lengths, widened by 4 ulp, is the tolerance of alpha and of the
line-search block), and s.y and sl must lie 1000 bounds away from zero."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U53 = 2.0 ** -53
FTOL, GTOL, XTOL, STPMIN, STPMAX = 1e-4, 0.9, 1e-14, 1e-100, 1e100
EVALUATE, CONVERGED, WARNING = 0, 1, 2
MARGIN = 1000.0

VEC = ('X', 'g', 'p', 'Hg', 's', 'y', 't', 'Xb', 'gb')
SCAL = ('f', 'fprev', 'alpha', 'slope', 'rho', 'hscale', 'iters', 'restarts', 'active', 'frozen', 'acc', 'upd', 'stall',
        'ident', 'pend', 'fb', 'nfev', 'hk')
LSF = ('stp', 'finit', 'ginit', 'gtest', 'stx', 'fx', 'gx', 'sty', 'fy', 'gy', 'stmin', 'stmax', 'width', 'width1',
       'brackt', 'stage', 'nfev', 'moved')
LS = dict((n, k) for k, n in enumerate(LSF))
LS_FLAGS = ('brackt', 'stage', 'nfev', 'moved')
FLAGS = ('iters', 'restarts', 'active', 'frozen', 'acc', 'upd', 'stall', 'ident', 'pend', 'nfev', 'hk')

_LIB = None


def ls_lib():
    """The host build of the line search (tests/csrc/ls_host.c)."""
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix='ls_host_')
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, 'ls_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'ls_host.c')])
        lib = C.CDLL(so)
        lib.ls_step.restype = C.c_int
        lib.ls_step.argtypes = [C.c_void_p] + [C.c_double] * 7
        lib.ls_start.argtypes = [C.c_void_p] + [C.c_double] * 6
        lib.ls_first_step.restype = C.c_double
        lib.ls_first_step.argtypes = [C.c_double] * 3
        assert lib.ls_ndoubles() == len(LSF)
        _LIB = lib
    return _LIB


def ls_start(a0, f, slope):
    st = np.zeros(len(LSF))
    ls_lib().ls_start(st.ctypes.data, float(a0), float(f), float(slope), FTOL, STPMIN, STPMAX)
    return st


def ls_step(st, f, dp):
    st = np.array(st, dtype=np.float64)
    rc = ls_lib().ls_step(st.ctypes.data, float(f), float(dp), FTOL, GTOL, XTOL, STPMIN, STPMAX)
    return rc, st


def first_step(f, fprev, slope):
    return ls_lib().ls_first_step(float(f), float(fprev), float(slope))


# ---------------------------------------------------------------------------------------------------------------------
# values with a rounding bound
class B(object):
    """v: value(s); n: terms of the longest chain; m: sum of absolute values of the terms (>= |v|).  n = 0: exact.
    dt: the type the sums are formed in (given where a number enters; results keep the type of their operands)."""
    __slots__ = ('v', 'n', 'm')

    def __init__(self, v, n=0, m=None, dt=None):
        self.v = np.asarray(v, dtype=dt) if dt is not None else np.asarray(v)
        self.n = int(n)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=self.v.dtype)

    @staticmethod
    def with_err(v, err, dt=None):
        """a value known to the absolute error err -- an interval, or a number read back from memory with the bound it was
        stored under: the chain starts again from it (n = 1)"""
        v = np.asarray(v, dtype=dt) if dt is not None else np.asarray(v)
        return B(v, 1, np.maximum(np.abs(v), np.asarray(err, dtype=v.dtype) / (8 * U53)))

    def stored(self):
        """the number as it is written to memory (f64) and read back: one more rounding on its chain"""
        return B(self.f64().astype(self.v.dtype), self.n + 1, self.m)

    def tol(self):
        with np.errstate(all='ignore'):
            return np.asarray(8.0 * self.n * U53 * self.m, dtype=np.float64)

    def f64(self):
        return np.asarray(self.v, dtype=np.float64)

    def __neg__(self):
        return B(-self.v, self.n, self.m)

    def __add__(self, o):
        return B(self.v + o.v, max(self.n, o.n) + 1, self.m + o.m)

    def __sub__(self, o):
        return B(self.v - o.v, max(self.n, o.n) + 1, self.m + o.m)

    def __mul__(self, o):
        return B(self.v * o.v, self.n + o.n + 1, self.m * o.m)

    def __truediv__(self, o):
        with np.errstate(all='ignore'):
            return B(self.v / o.v, self.n + o.n + 1, self.m * o.m / (o.v * o.v))

    def sqrt(self):
        with np.errstate(all='ignore'):
            r = np.sqrt(self.v)
            return B(r, self.n + 1, np.where(r > 0, self.m / np.where(r > 0, r, 1), 0))


def dot(a, b):
    """sum over the last axis of a * b (plain np.dot when the sums are formed in float64)"""
    if a.v.dtype == np.float64 and b.v.dtype == np.float64 and a.v.ndim == 1 and b.v.ndim == 1:
        v = np.dot(a.v, b.v)
    else:
        v = np.sum(a.v * b.v, axis=-1)
    return B(v, a.v.shape[-1] + a.n + b.n + 1, np.sum(a.m * b.m, axis=-1))


def matvec(A, x):
    """A (P, Q) . x (Q): one dot per row"""
    if A.v.dtype == np.float64 and x.v.dtype == np.float64:
        v = np.dot(A.v, x.v)
    else:
        v = np.sum(A.v * x.v[None, :], axis=1)
    return B(v, A.v.shape[1] + A.n + x.n + 1, np.sum(A.m * x.m[None, :], axis=1))


def ulp_widen(lo, hi, k=4):
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------------
# the state
class State(object):
    """The device block under its documented field names, plus what lives beside it: the update history (form 'hist':
    hist [M][Kmax][2][P], coef [M][Kmax][2]) or the dense matrices (form 'dense': Hd (M, P, ld)), and the reference's own
    real matrices H (M, P, P).  tol: field name -> tolerance of every entry after the last step (absent: bit-identical)."""

    def __init__(self, M, P, form='hist', Kmax=0, ld=0):
        self.M, self.P, self.form, self.Kmax, self.ld = M, P, form, Kmax, ld
        for n in VEC:
            setattr(self, n, np.zeros((M, P)))
        self.U, self.V = np.zeros((M, P, 3)), np.zeros((M, P, 3))
        for n in SCAL:
            setattr(self, n, np.zeros(M))
        self.ls = np.zeros((len(LSF), M))
        self.H = np.zeros((M, P, P), dtype=LD)
        for r in range(M):
            self.H[r] = np.eye(P, dtype=LD)
        self.hist = np.full((M, Kmax, 2, P), 1e30) if form == 'hist' else None
        self.coef = np.full((M, Kmax, 2), 1e30) if form == 'hist' else None
        self.Hd = np.full((M, P, ld), np.nan) if form == 'dense' else None
        self.tol = {}

    def copy(self):
        o = State.__new__(State)
        for k, v in self.__dict__.items():
            o.__dict__[k] = v.copy() if isinstance(v, np.ndarray) else (dict(v) if isinstance(v, dict) else v)
        return o


def state_doubles(M, P):
    return M * P * (len(VEC) + 6) + M * (len(SCAL) + len(LSF))


def _layout(st, get):
    parts = [get(n, (st.M, st.P)) for n in VEC] + [get('U', (st.M, st.P, 3)), get('V', (st.M, st.P, 3))]
    parts += [get(n, (st.M,)) for n in SCAL] + [get('ls', (len(LSF), st.M))]
    return np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in parts])


def pack(st):
    """the device block: (M,P) X g p Hg s y t Xb gb | (M,P,3) U V | (M) the 18 scalars | (18,M) line search"""
    return _layout(st, lambda n, shp: getattr(st, n))


def pack_tol(st):
    """tolerances in the layout of pack(); 0 = the entry must be bit-identical"""
    return _layout(st, lambda n, shp: st.tol[n] if n in st.tol else np.zeros(shp))


def unpack(a, M, P, form='hist', Kmax=0, ld=0):
    a = np.asarray(a, dtype=np.float64)
    assert a.size == state_doubles(M, P)
    st = State(M, P, form, Kmax, ld)
    o = 0
    for n in VEC:
        setattr(st, n, a[o:o + M * P].reshape(M, P).copy())
        o += M * P
    for n in ('U', 'V'):
        setattr(st, n, a[o:o + 3 * M * P].reshape(M, P, 3).copy())
        o += 3 * M * P
    for n in SCAL:
        setattr(st, n, a[o:o + M].copy())
        o += M
    st.ls = a[o:o + len(LSF) * M].reshape(len(LSF), M).copy()
    return st


def history_matrix(st, r):
    """hscale I + sum_j U_j V_j^T of row r from the history buffers (longdouble)"""
    P = st.P
    Hm = np.eye(P, dtype=LD) * LD(st.hscale[r])
    for j in range(int(st.hk[r])):
        s, Hy = st.hist[r, j, 0].astype(LD), st.hist[r, j, 1].astype(LD)
        c0, rho = LD(st.coef[r, j, 0]), LD(st.coef[r, j, 1])
        Hm += np.outer(c0 * s - rho * Hy, s) + np.outer(-rho * s, Hy)
    return Hm


def dense_matrix(st, r):
    """the matrix a dense row stands for: (hscale I | Hd) + pending U V^T (longdouble)"""
    P = st.P
    Hm = np.eye(P, dtype=LD) * LD(st.hscale[r]) if st.ident[r] != 0 else st.Hd[r, :, :P].astype(LD)
    if st.pend[r] != 0:
        Hm = Hm + st.U[r].astype(LD) @ st.V[r].astype(LD).T
    return Hm


def _settol(st, name, r, tol):
    if name not in st.tol:
        st.tol[name] = np.zeros(getattr(st, name).shape)
    st.tol[name][r] = tol


def _setls(st, r, lsv, lstol):
    st.ls[:, r] = lsv
    if 'ls' not in st.tol:
        st.tol['ls'] = np.zeros(st.ls.shape)
    st.tol['ls'][:, r] = lstol


def _span(mid, alts):
    """tolerance of every field of `mid` from the runs `alts`: the span of the values, widened by 4 ulp"""
    allv = np.stack([mid] + list(alts))
    with np.errstate(all='ignore'):
        lo, hi = ulp_widen(np.min(allv, axis=0), np.max(allv, axis=0))
        tol = np.maximum(hi - mid, mid - lo)
    tol = np.where(np.isfinite(tol), tol, 0.0)
    for n in LS_FLAGS:
        tol[LS[n]] = 0.0
    return tol


# ---------------------------------------------------------------------------------------------------------------------
# the phases, one row at a time
def _dt(sums):
    return LD if sums == 'ld' else np.float64


def init_phase(st, gtol, sums='ld'):
    """start of a fit from X, f, g: H = I, p = -g, first step min(1, 1.01 / |g|) through fprev = f + |g| / 2; a row with
    max|g| <= gtol never starts"""
    dt = _dt(sums)
    for r in range(st.M):
        g = B(st.g[r], dt=dt)
        st.Hg[r] = st.g[r]
        st.p[r] = -st.g[r]
        gg = dot(g, g)
        fprev = B(st.f[r], dt=dt) + gg.sqrt() * B(0.5)
        slope = -gg
        st.fprev[r], st.slope[r] = fprev.f64(), slope.f64()
        _settol(st, 'fprev', r, fprev.tol())
        _settol(st, 'slope', r, slope.tol())
        for n in ('rho', 'iters', 'restarts', 'frozen', 'acc', 'upd', 'stall', 'pend', 'nfev', 'hk'):
            getattr(st, n)[r] = 0.0
        st.hscale[r] = st.ident[r] = 1.0
        st.fb[r] = st.f[r]
        st.active[r] = 1.0 if np.max(np.abs(st.g[r])) > gtol else 0.0
        st.H[r] = np.eye(st.P, dtype=LD)
        _start_search(st, r, fprev, slope)
    return st


def _start_search(st, r, fprev, slope):
    f = st.f[r]
    fv, sv = [float(fprev.f64())], [float(slope.f64())]
    ft, stl = float(fprev.tol()), float(slope.tol())
    if ft > 0:
        fv += [fv[0] - ft, fv[0] + ft]
    if stl > 0:
        sv += [sv[0] - stl, sv[0] + stl]
    runs = []
    for a in fv:
        for b in sv:
            a0 = first_step(f, a, b)
            runs.append(ls_start(a0, f, b))
    _setls(st, r, runs[0], _span(runs[0], runs[1:]))
    st.alpha[r] = runs[0][LS['stp']]
    _settol(st, 'alpha', r, st.tol['ls'][LS['stp'], r])


def _ls_decide(st, r, ft, dp, max_trials):
    """(rc, src, moved, line-search block after the step): the documented outcome rules"""
    ls0 = st.ls[:, r].copy()
    stp, stx_prev, finit, gtest = ls0[LS['stp']], ls0[LS['stx']], ls0[LS['finit']], ls0[LS['gtest']]
    if np.isfinite(ft) and np.isfinite(dp):
        rc, ls1 = ls_step(ls0, ft, dp)
    else:
        rc, ls1 = WARNING, ls0.copy()
        ls1[LS['moved']] = 0.0
    if rc == EVALUATE and ls1[LS['nfev']] >= max_trials:
        rc = WARNING
    moved = int(ls1[LS['moved']] != 0.0)
    src = 0
    if rc == CONVERGED:
        src = 1
    elif rc == WARNING:
        fb = st.fb[r]
        okT = stp > 0.0 and ft <= finit + stp * gtest and ft < finit
        okB = stx_prev > 0.0 and fb <= finit + stx_prev * gtest and fb < finit
        if okT and (not okB or ft <= fb):
            src = 1
        elif okB:
            src = 2
    return rc, src, moved, ls1


def linesearch_phase(st, r, xt, ft, gt, max_trials, rec, work):
    if st.active[r] == 0.0:
        return
    dt = work['dt']
    dp = dot(B(gt, dt=dt), B(st.p[r], dt=dt))
    dpv, dpt = float(dp.f64()), float(dp.tol())
    rc, src, moved, ls1 = _ls_decide(st, r, ft, dpv, max_trials)
    alts = [_ls_decide(st, r, ft, dpv + sg * dpt, max_trials) for sg in (-1.0, 1.0)]
    key = lambda d: (d[0], d[1], d[2], d[3][LS['brackt']], d[3][LS['stage']])
    rec.update(rc=rc, src=src, moved=moved, dp=dpv, dp_tol=dpt,
               dp_stable=bool(all(key(a) == key((rc, src, moved, ls1)) for a in alts)))
    st.nfev[r] += 1.0
    if rc == EVALUATE:
        _setls(st, r, ls1, _span(ls1, [a[3] for a in alts]))
        st.alpha[r] = ls1[LS['stp']]
        _settol(st, 'alpha', r, st.tol['ls'][LS['stp'], r])
        rec['alpha_span'] = (st.alpha[r] - st.tol['alpha'][r], st.alpha[r] + st.tol['alpha'][r])
        if moved:
            st.fb[r] = ft
            st.Xb[r] = xt
            st.gb[r] = gt
        return
    if src == 0:
        st.stall[r] = 1.0
        return
    xs, gs = (xt, gt) if src == 1 else (st.Xb[r].copy(), st.gb[r].copy())
    # s and y are ONE IEEE subtraction each of numbers both sides hold bit for bit: the same bits on the device, exact inputs
    # of everything that follows
    st.s[r], st.y[r] = xs - st.X[r], gs - st.g[r]
    s, y = B(st.s[r], dt=dt), B(st.y[r], dt=dt)
    sy = dot(s, y)
    st.X[r], st.g[r] = xs, gs
    st.fprev[r] = st.f[r]
    st.f[r] = ft if src == 1 else st.fb[r]
    st.acc[r] = 1.0
    rho = B(1.0) / sy
    u = bool(sy.v > 0 and np.isfinite(rho.f64()))
    with np.errstate(all='ignore'):
        rec.update(sy=float(sy.f64()), sy_margin=float(abs(sy.f64()) / sy.tol()))
    st.upd[r] = 1.0 if u else 0.0
    st.rho[r] = rho.f64() if u else 0.0
    _settol(st, 'rho', r, rho.tol() if u else 0.0)
    work.update(s=s, y=y, rho=rho.stored() if u else B(0.0))


def hmul_phase(st, r, work):
    """t = H g for a row that has taken a point.  The value is the product with the reference's real matrix; the bound is
    that of the form the device holds (a row whose H is still hscale I is left alone: the update uses hscale g)."""
    if st.acc[r] == 0.0:
        return
    P, dt = st.P, work['dt']
    g = B(st.g[r], dt=dt)
    if st.form == 'hist':
        K = int(st.hk[r])
        if K == 0:
            return
        S, HY = B(st.hist[r, :K, 0], dt=dt), B(st.hist[r, :K, 1], dt=dt)
        c0, rho = B(st.coef[r, :K, 0], dt=dt), B(st.coef[r, :K, 1], dt=dt)
        a, b = dot(S, B(g.v[None, :])), dot(HY, B(g.v[None, :]))
        ab0, ab1 = c0 * a - rho * b, -(rho * a)
        terms = B(ab0.v[:, None], ab0.n, ab0.m[:, None]) * S + B(ab1.v[:, None], ab1.n, ab1.m[:, None]) * HY
        form = B(st.hscale[r], dt=dt) * g + B(np.sum(terms.v, axis=0), terms.n + K, np.sum(terms.m, axis=0))
        extra = K + 2                                        # the reference's matrix against the K stored, rounded updates
        work['ab'] = K                                       # the scratch coefficients the device leaves behind
    else:
        lazy = st.ident[r] != 0 and st.pend[r] == 0
        if lazy:
            return
        Hm = B(np.eye(P) * st.hscale[r], dt=dt) if st.ident[r] != 0 else B(st.Hd[r, :, :P], dt=dt)
        if st.pend[r] != 0:
            Uv, Vv = B(st.U[r], dt=dt), B(st.V[r], dt=dt)
            Hm = Hm + B(np.sum(Uv.v[:, None, :] * Vv.v[None, :, :], axis=2), 4,
                        np.sum(Uv.m[:, None, :] * Vv.m[None, :, :], axis=2))
            st.Hd[r, :, :P] = Hm.f64()
            if 'Hd' not in st.tol:
                st.tol['Hd'] = np.zeros(st.Hd.shape)
            st.tol['Hd'][r, :, :P] = Hm.tol()
            # pad columns go through the same pass with zero factors: 0 when the matrix is materialised here, else as they were
            if st.ident[r] != 0:
                st.Hd[r, :, P:] = 0.0
            st.ident[r], st.pend[r] = 0.0, 0.0               # (update_phase sets the flags of the NEW pending update)
        form = matvec(Hm, g)
        extra = 2
    if dt is LD:
        t = B(np.sum(st.H[r] * g.v[None, :], axis=1), form.n + extra, form.m)
    else:
        t = form
    st.t[r] = t.f64()
    _settol(st, 't', r, t.tol())
    work['t'] = t.stored()


def _product_update(Hm, s, y):
    """H_new = (I - rho s y^T) H (I - rho y s^T) + rho s s^T in longdouble, rho = 1 / s.y: the documented update as it
    stands (small P: the three matrix products literally; else the same products multiplied out, still O(P^2))"""
    rho = LD(1.0) / np.sum(s * y)
    P = s.size
    if P <= 129:
        A = np.eye(P, dtype=LD) - rho * np.outer(s, y)
        return np.dot(np.dot(A, Hm), A.T) + rho * np.outer(s, s)
    Hy, yH = np.sum(Hm * y[None, :], axis=1), np.sum(Hm * y[:, None], axis=0)
    yHy = np.sum(y * Hy)
    return Hm - rho * np.outer(s, yH) - rho * np.outer(Hy, s) + (rho * rho * yHy + rho) * np.outer(s, s)


def update_phase(st, r, gtol, maxiter, init_scaling, rec, work):
    act, a, u, stl = st.active[r] != 0, st.acc[r] != 0, st.upd[r] != 0, st.stall[r] != 0
    if not act or (not a and not stl):
        return
    P, dt = st.P, work['dt']
    g = B(st.g[r], dt=dt)
    hs = B(st.hscale[r], dt=dt)
    frozen = again = False
    Hg_old = B(st.Hg[r], dt=dt)
    if a:
        lazy = work['lazy']
        st.iters[r] += 1.0
        st.restarts[r] = 0.0
        if u:
            s, y, rho = work['s'], work['y'], work['rho']
            sc = B(1.0)
            if init_scaling and lazy:
                gam = (B(1.0) / rho) / dot(y, y)
                if gam.v > 0 and np.isfinite(gam.f64()):
                    sc, hs = gam / hs, gam
                    st.H[r] = np.eye(P, dtype=LD) * LD(np.sum(s.v * y.v) / np.sum(y.v * y.v))
            tc = hs * g if lazy else work['t']
            Hy = tc - sc * Hg_old
            yHy, vg0, vg2 = dot(y, Hy), dot(s, g), dot(Hy, g)
            c0 = (B(1.0) + rho * yHy) * rho
            u0, u1, u2 = c0 * s, -(rho * Hy), -(rho * s)
            Hg = tc + (u0 * vg0 + u1 * vg0 + u2 * vg2)        # the factored form: its terms give the bound
            rec['c0'] = float(c0.f64())
            if dt is LD:
                # the value: H_new g_new with the reference's own matrix, advanced by the documented product formula
                st.H[r] = _product_update(st.H[r], s.v, y.v)
                Hg = B(np.sum(st.H[r] * g.v[None, :], axis=1), Hg.n + 2, Hg.m)
            if st.form == 'hist':
                k = int(st.hk[r])
                st.hist[r, k, 0], st.hist[r, k, 1] = s.f64(), Hy.f64()
                st.coef[r, k] = (c0.f64(), st.rho[r])
                for nm, arr in (('hist', st.hist), ('coef', st.coef)):
                    if nm not in st.tol:
                        st.tol[nm] = np.zeros(arr.shape)
                st.tol['hist'][r, k, 0], st.tol['hist'][r, k, 1] = 0.0, Hy.tol()
                st.tol['coef'][r, k] = (c0.tol(), st.tol['rho'][r])
                st.ident[r], st.pend[r] = 0.0, 0.0
                st.hk[r] += 1.0
            else:
                st.U[r] = np.stack((u0.f64(), u1.f64(), u2.f64()), axis=1)
                st.V[r] = np.stack((s.f64(), s.f64(), Hy.f64()), axis=1)
                _settol(st, 'U', r, np.stack((u0.tol(), u1.tol(), u2.tol()), axis=1))
                _settol(st, 'V', r, np.stack((s.tol(), s.tol(), Hy.tol()), axis=1))
                st.ident[r], st.pend[r] = (1.0 if lazy else 0.0), 1.0
        else:
            Hg = hs * g if lazy else work['t']
            st.ident[r], st.pend[r] = (1.0 if lazy else 0.0), 0.0
        st.Hg[r] = Hg.f64()
        _settol(st, 'Hg', r, Hg.tol())
        Hg = Hg.stored() if Hg.n else Hg                     # read back from memory: the chain starts again
    else:
        Hg = Hg_old
        again = st.restarts[r] == 0.0
        if again:
            st.restarts[r] = 1.0
        else:
            frozen = True
    sl, gg = -dot(Hg, g), dot(g, g)
    gmax = float(np.max(np.abs(st.g[r])))
    newls = a or again
    descent = bool(sl.v < 0)
    reset = newls and (again or not descent)
    if newls and not again:
        with np.errstate(all='ignore'):
            rec.update(sl=float(sl.f64()), sl_margin=float(abs(sl.f64()) / sl.tol()))
    if newls:
        if reset:
            st.Hg[r] = st.g[r]
            _settol(st, 'Hg', r, 0.0)
            st.p[r] = -st.g[r]
            _settol(st, 'p', r, 0.0)
        else:
            st.p[r] = -st.Hg[r]
            _settol(st, 'p', r, st.tol['Hg'][r])
    if frozen:
        st.frozen[r] = 1.0
    if reset:
        st.ident[r], st.pend[r], hs = 1.0, 0.0, B(1.0)
        st.hk[r] = 0.0
        st.H[r] = np.eye(P, dtype=LD)
    st.hscale[r] = hs.f64()
    _settol(st, 'hscale', r, hs.tol())
    go = (not frozen) and gmax > gtol and st.iters[r] < maxiter
    if newls and go:
        slope = -gg if reset else sl
        fprev = B(st.f[r], dt=dt) + gg.sqrt() * B(0.5) if again else B(st.fprev[r])
        st.fprev[r], st.slope[r] = fprev.f64(), slope.f64()
        _settol(st, 'fprev', r, fprev.tol())
        _settol(st, 'slope', r, slope.tol())
        _start_search(st, r, fprev, slope)
        st.fb[r] = st.f[r]
    st.active[r] = 1.0 if go else 0.0
    st.acc[r] = st.upd[r] = st.stall[r] = 0.0
    rec.update(upd=int(u and a), reset=bool(reset), again=bool(again), frozen=bool(frozen), go=bool(go), gmax=gmax)


def trial_phase(st, rows, pos_next=None, L_next=None, sentinel=np.nan, sums='ld'):
    """Xt_next[pos_next[r]] = X[r] + alpha[r] p[r] for the listed rows (pos_next None: the same positions; < 0: dropped);
    rows of Xt_next that nobody writes keep the sentinel.  Returns (Xt_next, its tolerance)."""
    dt = _dt(sums)
    L = len(rows)
    L_next = L if L_next is None else L_next
    Xn = np.full((L_next, st.P), sentinel)
    Xtol = np.zeros((L_next, st.P))
    for j, r in enumerate(rows):
        jn = j if pos_next is None else int(pos_next[r])
        if jn < 0:
            continue
        al = B.with_err(st.alpha[r], st.tol['alpha'][r] if 'alpha' in st.tol else 0.0, dt=dt)
        pt = st.tol['p'][r] if 'p' in st.tol else 0.0
        pp = B.with_err(st.p[r], pt, dt=dt) if np.any(pt) else B(st.p[r], dt=dt)
        x = al * pp + B(st.X[r], dt=dt)
        Xn[jn], Xtol[jn] = x.f64(), x.tol()
    return Xn, Xtol


def step(state, rows, Xt, f, g, max_trials=100, gtol=1e-5, maxiter=225, init_scaling=0, pos_next=None, L_next=None,
         sentinel=np.nan, sums='ld'):
    """One launch of pgl_bfgs_step_dev with final f and g.  rows: the listed rows (None: 0 .. len(f) - 1); Xt, f, g by list
    position.  Returns (state', out) with out = dict(Xt_next, Xt_next_tol, pos_next, active (the flags of the listed rows,
    by row), ab (row -> number of scratch coefficient pairs the implicit forms leave behind), decisions (per listed row: rc,
    src, moved, upd, reset, again, frozen, go and the margins))."""
    st = state.copy()
    st.tol = {}
    rows = list(range(len(f))) if rows is None else [int(r) for r in rows]
    decisions, ab = [], {}
    for j, r in enumerate(rows):
        rec = dict(row=r, rc=None, src=0, moved=0, upd=0, reset=False, again=False, frozen=False,
                   go=bool(st.active[r] != 0), dp_stable=True, sy_margin=np.inf, sl_margin=np.inf)
        work = dict(lazy=bool(st.ident[r] != 0 and st.pend[r] == 0), dt=_dt(sums))
        linesearch_phase(st, r, np.asarray(Xt[j], dtype=np.float64), float(f[j]), np.asarray(g[j], dtype=np.float64),
                         max_trials, rec, work)
        hmul_phase(st, r, work)
        update_phase(st, r, gtol, maxiter, init_scaling, rec, work)
        rec.update(active=int(st.active[r]), iters=int(st.iters[r]), nfev=int(st.nfev[r]), hk=int(st.hk[r]))
        decisions.append(rec)
        if 'ab' in work:
            ab[r] = work['ab']
    Xn, Xtol = trial_phase(st, rows, pos_next, L_next, sentinel, sums)
    flags = dict((r, st.active[r]) for r in rows)
    return st, dict(Xt_next=Xn, Xt_next_tol=Xtol, pos_next=pos_next, active=flags, ab=ab, decisions=decisions)


def valid(decisions):
    """the margin condition: no decision of the launch hangs on the rounding of dp, s.y or sl"""
    return all(d['dp_stable'] and d['sy_margin'] >= MARGIN and d['sl_margin'] >= MARGIN for d in decisions)


# ---------------------------------------------------------------------------------------------------------------------
# synthetic single-launch cases (tests/test_bfgs_reference.py checks them on the CPU, tests/test_gpu_bfgs_rows.py runs them)
def R(hk, out, **kw):
    return dict(hk=hk, out=out, **kw)


KMAX, MAXITER, MAX_TRIALS = 40, 40, 20
EXPECT = dict(conv=dict(rc=1, src=1, upd=1), eval_moved=dict(rc=0, moved=1), eval_nomove=dict(rc=0, moved=0),
              warn_trial=dict(rc=2, src=1, upd=1), sy_neg=dict(rc=2, src=1, upd=0), warn_best=dict(rc=2, src=2, upd=1),
              stall=dict(rc=2, src=0), inf=dict(rc=2, src=0, again=True, reset=True), inf_best=dict(rc=2, src=2, upd=1))

CASES = [
    dict(name='p1', P=1, rows=[R(0, 'conv'), R(1, 'eval_moved'), R(3, 'conv')]),
    dict(name='p2_scaled', P=2, init_scaling=1, rows=[R(1, 'conv'), R(0, 'eval_nomove'), R(4, 'warn_trial')]),
    dict(name='p63_moved_list', P=63, list=[3, 0, 4, 1], pos_next=[-1, 1, -1, 0, 2], L_next=4,
         rows=[R(0, 'conv'), R(5, 'conv'), R(7, 'eval_moved'), R(8, 'warn_best'), R(9, 'conv')]),
    dict(name='p64_pad4', P=64, ldpad=4, rows=[R(15, 'conv'), R(16, 'conv'), R(17, 'conv')]),
    dict(name='p65_stalls', P=65, list=[4, 2, 0, 3, 1],
         rows=[R(24, 'conv'), R(25, 'sy_neg'), R(33, 'conv'), R(3, 'stall', expect=dict(again=True, reset=True, go=True)),
               R(0, 'stall', restarts=1, expect=dict(frozen=True, go=False))]),
    dict(name='p129_inf', P=129, list=[2, 0], rows=[R(33, 'conv'), R(9, 'inf'), R(1, 'inf_best')]),
    dict(name='p129_inf_listed', P=129, rows=[R(4, 'inf'), R(9, 'inf', restarts=1, expect=dict(frozen=True, again=False,
                                                                                             reset=False, go=False))]),
    dict(name='p255_indefinite', P=255, ldpad=4,
         rows=[R(8, 'conv', indef=True, expect=dict(reset=True)), R(16, 'conv', pend0=True),
               R(4, 'conv', inactive=True, expect=dict(rc=None, src=0, upd=0, go=False))]),
    dict(name='p256', P=256, init_scaling=1, rows=[R(17, 'conv')]),
    dict(name='p257_first_update', P=257, init_scaling=0,
         rows=[R(0, 'conv'), R(0, 'conv', restarts=1), R(25, 'conv', pre='bracket')]),
    dict(name='p257_first_update_scaled', P=257, init_scaling=1,
         rows=[R(0, 'conv'), R(0, 'conv', restarts=1), R(25, 'conv', pre='bracket')]),
    dict(name='p261_maxiter', P=261, list=[4, 1, 3, 2], pos_next=[-1, 0, 2, -1, 1], L_next=3,
         rows=[R(7, 'conv'), R(15, 'eval_moved'), R(24, 'conv', iters=MAXITER - 1, expect=dict(go=False)), R(33, 'conv'),
               R(5, 'eval_nomove')]),
    dict(name='p513', P=513, rows=[R(33, 'conv'), R(16, 'conv'), R(1, 'warn_trial')]),
    dict(name='p65_gmax_equals_gtol', P=65, gtol=('eq', 1),
         rows=[R(3, 'conv', expect=dict(go=True)), R(4, 'conv', gscale=0.05, expect=dict(go=False)), R(0, 'conv')]),
    dict(name='p65_gmax_ulp_above_gtol', P=65, gtol=('above', 1),
         rows=[R(3, 'conv', expect=dict(go=True)), R(4, 'conv', gscale=0.05, expect=dict(go=True)), R(0, 'conv')]),
]
FORMS = ('merged', 'split', 'dense')
_CASE_CACHE = {}


def _build_row(st, r, rs, seed):
    rng = np.random.default_rng([seed, r])
    P, hk, dense = st.P, rs['hk'], st.form == 'dense'
    sign = -1.0 if rs.get('indef') else 1.0
    # (a point of small entries beside a step of order one: s = x_new - X loses nothing to cancellation, so the bounds of
    #  everything built on s stay near the numbers themselves)
    X, g, A = 0.03 * rng.standard_normal(P), 0.5 * rng.standard_normal(P), rng.uniform(0.5, 4.0, P)
    hs = 1.0 if hk == 0 else 0.7
    Hm = np.eye(P, dtype=LD) * LD(hs)
    Hprev, Ul, Vl = None, rng.standard_normal((P, 3)), rng.standard_normal((P, 3))
    for j in range(hk):
        s = 0.3 * rng.standard_normal(P)
        y = A * s
        Hy = np.asarray(np.sum(Hm * y.astype(LD)[None, :], axis=1), dtype=np.float64)
        rho = float(1.0 / np.sum(s.astype(LD) * y.astype(LD)))
        c0 = float((1.0 + LD(rho) * np.sum(y.astype(LD) * Hy.astype(LD))) * LD(rho))
        Hprev = Hm.copy()
        Hm = _product_update(Hm, s.astype(LD), y.astype(LD))   # the reference's matrix: the documented product formula
        if not dense:
            st.hist[r, j, 0], st.hist[r, j, 1] = s, Hy
            st.coef[r, j] = (sign * c0, sign * rho)
        Ul = sign * np.stack((c0 * s, -rho * Hy, -rho * s), axis=1)
        Vl = np.stack((s, s, Hy), axis=1)
    hs, Hm = sign * hs, sign * Hm
    st.hscale[r] = hs
    st.U[r], st.V[r] = Ul, Vl
    if dense:
        st.hk[r] = 0.0
        st.Hd[r, :, P:] = 1e30
        if hk <= 1:
            st.ident[r], st.pend[r] = 1.0, float(hk)
        elif rs.get('pend0'):
            st.ident[r], st.pend[r] = 0.0, 0.0
            st.Hd[r, :, :P] = np.asarray(Hm, dtype=np.float64)
        else:
            st.ident[r], st.pend[r] = 0.0, 1.0
            st.Hd[r, :, :P] = np.asarray(sign * Hprev, dtype=np.float64)
        if hk <= 1:
            st.Hd[r] = np.nan                                # a matrix that is not materialised yet: never read
        st.H[r] = Hm
    else:
        st.hk[r], st.ident[r], st.pend[r] = float(hk), float(hk == 0), 0.0
        st.H[r] = Hm
    Hg = np.asarray(np.sum(st.H[r] * g.astype(LD)[None, :], axis=1), dtype=np.float64)
    p = -sign * Hg
    slope = float(np.sum(p.astype(LD) * g.astype(LD)))
    assert slope < 0
    f = 3.0 + rng.uniform()
    st.X[r], st.g[r], st.Hg[r], st.p[r] = X, g, Hg, p
    fprev = f - 0.5 * slope                                  # first step min(1, 1.01) = 1
    st.f[r], st.fprev[r], st.fb[r], st.slope[r] = f, fprev, f, slope
    for n in ('s', 'y', 't', 'Xb', 'gb'):
        getattr(st, n)[r] = rng.standard_normal(P)
    st.rho[r] = 0.0
    st.iters[r], st.restarts[r], st.nfev[r] = rs.get('iters', hk), rs.get('restarts', 0), 2 * hk
    st.active[r] = 0.0 if rs.get('inactive') else 1.0
    lsv = ls_start(first_step(f, fprev, slope), f, slope)
    pp = float(np.sum(p.astype(LD) ** 2))

    def mk_g(target):
        rv = rs.get('gscale', 1.0) * 0.5 * rng.standard_normal(P)
        return np.asarray(rv + ((target - np.sum(rv.astype(LD) * p.astype(LD))) / pp) * p.astype(LD), dtype=np.float64)

    out = rs['out']
    pre = rs.get('pre') or ('best' if out in ('warn_best', 'inf_best') else None)
    if pre:
        a = lsv[LS['stp']]
        f1, g1 = (f + 0.5 * a * slope, mk_g(0.97 * slope)) if pre == 'best' else (f - 0.3 * a * slope, mk_g(-0.5 * slope))
        rc, lsv = ls_step(lsv, f1, float(np.sum(g1.astype(LD) * p.astype(LD))))
        assert rc == EVALUATE and (lsv[LS['moved']] != 0) == (pre == 'best')
        if pre == 'best':
            st.fb[r], st.Xb[r], st.gb[r] = f1, X + a * p, g1
        st.nfev[r] += 1
    if out in ('warn_trial', 'sy_neg', 'warn_best', 'stall'):
        lsv[LS['nfev']] = MAX_TRIALS - 1
    st.ls[:, r] = lsv
    a = st.alpha[r] = lsv[LS['stp']]
    lower, higher = f + 0.5 * a * slope, f - 0.3 * a * slope
    ft, dpt = dict(conv=(lower, 0.2), eval_moved=(lower, 0.97), warn_trial=(lower, 0.97), sy_neg=(lower, 1.3),
                   eval_nomove=(higher, -0.5), warn_best=(higher, -0.5), stall=(higher, -0.5), inf=(np.inf, 0.5),
                   inf_best=(np.inf, 0.5))[out]
    return X + a * p, ft, mk_g(dpt * slope)


def build_case(name, form):
    """(state, step arguments, specification) of a single-launch case in one of the three forms; cached, never modified"""
    if (name, form) in _CASE_CACHE:
        return _CASE_CACHE[(name, form)]
    spec = [c for c in CASES if c['name'] == name][0]
    P, M = spec['P'], len(spec['rows'])
    ld = P + (P & 1) + (spec.get('ldpad', 0) if form == 'dense' else 0)
    st = State(M, P, 'dense' if form == 'dense' else 'hist', KMAX, ld)
    seed = 1000 + [c['name'] for c in CASES].index(name)
    ev = [_build_row(st, r, spec['rows'][r], seed) for r in range(M)]
    rows = spec.get('list')
    lst = list(range(M)) if rows is None else rows
    gtol = spec.get('gtol', 1e-5)
    if isinstance(gtol, tuple):
        gm = float(np.max(np.abs(ev[gtol[1]][2])))
        gtol = gm if gtol[0] == 'eq' else float(np.nextafter(gm, 0.0))
    args = dict(rows=rows, Xt=np.stack([ev[r][0] for r in lst]), f=np.array([ev[r][1] for r in lst]),
                g=np.stack([ev[r][2] for r in lst]), max_trials=MAX_TRIALS, gtol=gtol, maxiter=MAXITER,
                init_scaling=spec.get('init_scaling', 0), pos_next=spec.get('pos_next'), L_next=spec.get('L_next'),
                sentinel=-7.25e77)
    hk_bound = max(rs['hk'] for rs in spec['rows'])
    _CASE_CACHE[(name, form)] = (st, args, dict(spec, hk_bound=hk_bound, ld=ld, lst=lst))
    return _CASE_CACHE[(name, form)]


def run_case(name, form):
    """(state, arguments, specification, state after the launch, outputs) of the reference; cached"""
    key = (name, form, 'run')
    if key not in _CASE_CACHE:
        st, args, spec = build_case(name, form)
        _CASE_CACHE[key] = (st, args, spec) + step(st, **args)
    return _CASE_CACHE[key]


def expected_decisions(spec):
    """what every listed row of a case must decide, by list position"""
    exp = []
    for r in spec['lst']:
        rs = spec['rows'][r]
        e = dict(EXPECT[rs['out']])
        e.update(rs.get('expect', {}))
        exp.append(e)
    return exp


def fit(fun, X0, gtol=1e-5, maxiter=225, init_scaling=0, form='hist', sums='ld', max_trials=100):
    """The driver loop around step(): fun(r, x) -> (f, g).  Rows leave the list as they finish, as in the product's driver.
    Returns (state, iterates: per row the points taken, the decisions of every launch, record: per launch the list and per
    listed row (rc, src, active, iters, nfev, hk))."""
    M, P = X0.shape
    st = State(M, P, form, maxiter, P + (P & 1))
    st.X[:] = X0
    for r in range(M):
        st.f[r], st.g[r] = fun(r, X0[r])
    st = init_phase(st, gtol, sums)
    rows = [r for r in range(M) if st.active[r] != 0]
    Xt = trial_phase(st, rows, sums=sums)[0]
    iterates, log, record = [[] for _ in range(M)], [], []
    while rows:
        fg = [fun(r, Xt[j]) for j, r in enumerate(rows)]
        before = st.iters.copy()
        st, out = step(st, rows, Xt, np.array([v[0] for v in fg]), np.stack([v[1] for v in fg]), max_trials=max_trials,
                       gtol=gtol, maxiter=maxiter, init_scaling=init_scaling, sums=sums)
        for r in rows:
            if st.iters[r] != before[r]:
                iterates[r].append(st.X[r].copy())
        log.append(out['decisions'])
        record.append((tuple(rows), [(d['rc'], d['src'], d['active'], d['iters'], d['nfev'], d['hk']) for d in out['decisions']]))
        keep = [j for j, r in enumerate(rows) if st.active[r] != 0]
        rows, Xt = [rows[j] for j in keep], out['Xt_next'][keep]
    return st, iterates, log, record
