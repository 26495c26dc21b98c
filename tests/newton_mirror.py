"""The host mirror of the lock-step dense Newton fit: theano_pyglm_amd/csrc/pglm_newton.h compiled for the host with gcc
through tests/csrc/newton_host.c (the way tests/prox_mirror.py builds prox_host.c) and driven with numpy: the priors' part
of f, g and the Hessian (objective, prior_hessian, assemble), the factor from laplace.numpy_factor, the solve from
scipy.linalg.solve_triangular, the Hessian of ll from tests/hessian_reference.py.  Shared by tests/test_newton_host.py (no
GPU) and tests/test_gpu_newton.py (every row kernel launch against this mirror).  Test infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
from scipy.linalg import solve_triangular

from theano_pyglm_amd.inference.laplace import numpy_factor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('f', 'fprev', 'slope', 'alpha', 'shift', 'nit', 'nfev', 'nhess', 'nfact', 'status', 'phase')
SC = dict((n, i) for i, n in enumerate(FIELDS))
NLS = 18
VECS = ('X', 'g', 'p', 'Xb', 'gb')                             # the (M, P) arrays of the device block, in its order
PHASE_HESS, PHASE_SEARCH, PHASE_DONE, PHASE_REFACTOR = 0.0, 1.0, 2.0, 3.0
LADDER = (0.0, 1e-6, 1e-4, 1e-2, 1.0, 1e2)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='newton_host_'), 'newton_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'newton_host.c')])
        L = C.CDLL(so)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.newton_start.argtypes = [vp, vp, vp, i, i, d, d, vp]
        L.newton_feed_direction.argtypes = [vp, vp, vp, i, i, vp]
        L.newton_feed_fg.argtypes = [vp, vp, vp, i, i, d, d, vp]
        L.newton_next_shift.argtypes = [d]
        L.newton_next_shift.restype = d
        assert L.newton_nscal() == len(FIELDS) and L.newton_nls() == NLS
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the priors' part in numpy (prior: the 7-tuple of _Packing.prior_params(): kind, mu_b, sg_b, stim_sigma, mu, sigma, lam)
def objective(X, ll, grad, prior, N, B, Dstim):
    """f = -(ll + log prior) (M,), g = -(grad + prior gradient) (M, P) of theta rows X; no NaN rules (the machine's).
    prior None: no prior at all (the tests' quadratics)."""
    if prior is None:
        return -np.asarray(ll, dtype=float), -np.asarray(grad, dtype=float)
    kind, mu_b, sg_b, ss, mu, sigma, lam = prior
    X = np.asarray(X, dtype=float)
    M = X.shape[0]
    lp = -0.5 * ((X[:, 0] - mu_b) / sg_b) ** 2 - 0.5 * np.sum((X[:, 1:1 + Dstim] / ss) ** 2, axis=1)
    gp = np.zeros_like(X)
    gp[:, 0] = -(X[:, 0] - mu_b) / sg_b ** 2
    gp[:, 1:1 + Dstim] = -X[:, 1:1 + Dstim] / ss ** 2
    w = X[:, 1 + Dstim:].reshape(M, N, B)
    if kind == 1:
        z = (w - mu) / sigma
        nrm = np.sqrt(np.sum(z * z, axis=2))
        lp = lp - lam * np.sum(nrm, axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            gp[:, 1 + Dstim:] = (-lam * z / nrm[:, :, None] / sigma).reshape(M, N * B)
    else:
        lp = lp - 0.5 * np.sum(((w - mu) / sigma) ** 2, axis=(1, 2))
        gp[:, 1 + Dstim:] = (-(w - mu) / sigma ** 2).reshape(M, N * B)
    return -(np.asarray(ll, dtype=float) + lp), -(np.asarray(grad, dtype=float) + gp)


def prior_hessian(x, prior, N, B, Dstim):
    """(P, P): the Hessian of the log prior at the theta row x."""
    if prior is None:
        return np.zeros((x.size, x.size))
    kind, mu_b, sg_b, ss, mu, sigma, lam = prior
    P = x.size
    Hp = np.zeros((P, P))
    Hp[0, 0] = -1.0 / sg_b ** 2
    for c in range(1, 1 + Dstim):
        Hp[c, c] = -1.0 / ss ** 2
    for n in range(N):
        o = 1 + Dstim + n * B
        if kind == 1:
            z = (x[o:o + B] - mu) / sigma
            nrm = np.sqrt(np.sum(z * z))
            with np.errstate(invalid='ignore', divide='ignore'):
                Hp[o:o + B, o:o + B] = -lam / sigma ** 2 * (np.eye(B) / nrm - np.outer(z, z) / nrm ** 3)
        else:
            Hp[o:o + B, o:o + B] = -np.eye(B) / sigma ** 2
    return Hp


def assemble(H_ll, x, shift, prior, N, B, Dstim):
    """A = -H - H_prior(x) + shift diag(-H - H_prior): what pgl_newton_assemble_dev leaves in the lower triangle."""
    A = -(np.asarray(H_ll, dtype=float) + prior_hessian(x, prior, N, B, Dstim))
    i = np.arange(x.size)
    A[i, i] = A[i, i] + shift * A[i, i]
    return A


def factor_solve(A, g):
    """(info, sol): laplace.numpy_factor on A and sol = -A^-1 g by two triangular solves around the scales."""
    F, scale, _, info = numpy_factor(A[None])
    if info[0] != 0:
        return int(info[0]), np.full(g.size, np.nan)
    Ls = np.tril(F[0])
    y = solve_triangular(Ls, -g / scale[0], lower=True)
    return 0, solve_triangular(Ls, y, lower=True, trans='T') / scale[0]


class Mirror(object):
    """M rows of P = 1 + Dstim + N B parameters, each its own machine.  target(X (M, P)) -> (ll (M,), grad (M, P));
    hessian(X (L, P), rows) -> (L, P, P) Hessians of ll of the listed rows at their points."""

    def __init__(self, target, hessian, X0, N, B, Dstim, prior, gtol=1e-5, maxiter=50):
        self.lib = lib()
        self.target, self.hessian = target, hessian
        X0 = np.ascontiguousarray(X0, dtype=float)
        self.M, self.P = X0.shape
        assert self.P == 1 + Dstim + N * B
        self.NBD = (int(N), int(B), int(Dstim))
        self.prior = None if prior is None else tuple(prior)
        self.gtol, self.maxiter = float(gtol), int(maxiter)
        self.sc = np.zeros((self.M, len(FIELDS)))
        self.ls = np.zeros((self.M, NLS))
        self.vec = np.zeros((self.M, 6, self.P))               # x, g, p, xb, gb, xt
        self.vec[:, 0] = X0
        self.shifts = [[] for _ in range(self.M)]              # per row: the shifts of every factorisation, by outer iteration
        self.fallback = [0] * self.M                           # per row: searches along -g
        self.f_trace = [[] for _ in range(self.M)]
        self.H = {}                                            # row -> the Hessian of ll at its point (kept for a refactor)

    # -- the five launches, row by row ------------------------------------------------------------------------------
    def init(self, ll=None, grad=None):
        if ll is None:
            ll, grad = self.target(self.vec[:, 0].copy())
        f, g = objective(self.vec[:, 0], ll, grad, self.prior, *self.NBD)
        for r in range(self.M):
            gr = np.ascontiguousarray(g[r])
            self.lib.newton_start(_p(self.sc[r]), _p(self.ls[r]), _p(self.vec[r]), self.P, self.maxiter, self.gtol,
                                  float(f[r]), _p(gr))
            self.f_trace[r].append(self.sc[r, SC['f']])
        return self

    def field(self, name):
        return self.sc[:, SC[name]]

    def rows_in(self, *phases):
        return np.nonzero(np.isin(self.field('phase'), phases))[0]

    def assembled(self, r, H_ll):
        return assemble(H_ll, self.vec[r, 0], self.sc[r, SC['shift']], self.prior, *self.NBD)

    def direction(self, r, info, sol):
        fresh = self.sc[r, SC['phase']] == PHASE_HESS
        shift = self.sc[r, SC['shift']]
        sol = np.ascontiguousarray(sol, dtype=float)
        ph = self.lib.newton_feed_direction(_p(self.sc[r]), _p(self.ls[r]), _p(self.vec[r]), self.P, int(info), _p(sol))
        if fresh:
            self.shifts[r].append([])
        self.shifts[r][-1].append(shift)
        if ph == 1 and not np.array_equal(self.vec[r, 2], sol):        # the search runs, but not along the solve's output
            self.fallback[r] += 1
        return ph

    def feed(self, r, ll, grad, xt=None):
        """The evaluation (ll, grad of ll) of row r's trial point (xt: the point it was made at, default the mirror's)."""
        if xt is not None:
            self.vec[r, 5] = xt
        f, g = objective(self.vec[r, 5][None], np.array([ll]), np.asarray(grad)[None], self.prior, *self.NBD)
        g0 = np.ascontiguousarray(g[0])
        nit = self.sc[r, SC['nit']]
        ph = self.lib.newton_feed_fg(_p(self.sc[r]), _p(self.ls[r]), _p(self.vec[r]), self.P, self.maxiter, self.gtol,
                                     float(f[0]), _p(g0))
        if self.sc[r, SC['nit']] > nit:
            self.f_trace[r].append(self.sc[r, SC['f']])
        return ph

    # -- the driver: batched_newton.py's loop in numpy ----------------------------------------------------------------
    def outer(self):
        rows = self.rows_in(PHASE_HESS)
        if rows.size:
            Hs = self.hessian(self.vec[rows, 0].copy(), rows)
            for r, H in zip(rows, Hs):
                self.H[r] = H
        todo = rows
        while todo.size:
            for r in todo:
                info, sol = factor_solve(self.assembled(r, self.H[r]), self.vec[r, 1])
                self.direction(r, info, sol)
            todo = todo[self.field('phase')[todo] == PHASE_REFACTOR]
        rows = self.rows_in(PHASE_SEARCH)
        while rows.size:
            ll, grad = self.target_rows(self.vec[rows, 5].copy(), rows)
            for j, r in enumerate(rows):
                self.feed(r, ll[j], grad[j])
            rows = rows[self.field('phase')[rows] == PHASE_SEARCH]

    def target_rows(self, Xt, rows):
        X = self.vec[:, 0].copy()
        X[rows] = Xt
        ll, grad = self.target(X)
        return np.asarray(ll)[rows], np.asarray(grad)[rows]

    def run(self):
        k = 0
        while not np.all(self.field('phase') == PHASE_DONE):
            self.outer()
            k += 1
            assert k <= self.maxiter + 1
        return self

    # -- the device block ---------------------------------------------------------------------------------------------
    def block(self):
        """The state as the device lays it out (pgl_newton_state_doubles(M, P) doubles)."""
        return np.concatenate([self.vec[:, k].reshape(-1) for k in range(5)] + [self.sc.T.reshape(-1), self.ls.T.reshape(-1)])

    def load_block(self, st):
        M, P = self.M, self.P
        st = np.asarray(st, dtype=float)
        assert st.size == 5 * M * P + M * (len(FIELDS) + NLS)
        for k in range(5):
            self.vec[:, k] = st[k * M * P:(k + 1) * M * P].reshape(M, P)
        o = 5 * M * P
        self.sc[:] = st[o:o + len(FIELDS) * M].reshape(len(FIELDS), M).T
        self.ls[:] = st[o + len(FIELDS) * M:].reshape(NLS, M).T


def split_block(st, M, P):
    """{name: array} of a device block: the five (M, P) vectors, 'sc' (11, M), 'ls' (18, M)."""
    out = dict((n, st[k * M * P:(k + 1) * M * P].reshape(M, P)) for k, n in enumerate(VECS))
    o = 5 * M * P
    out['sc'] = st[o:o + len(FIELDS) * M].reshape(len(FIELDS), M)
    out['ls'] = st[o + len(FIELDS) * M:].reshape(NLS, M)
    return out
