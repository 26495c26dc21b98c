"""The host mirror of the lock-step proximal-gradient fit: theano_pyglm_amd/csrc/pglm_prox.h compiled for the host with gcc
through tests/csrc/prox_host.c (the way tests/hmc_mirror.py builds hmc_host.c) and driven with numpy supplying ll and its
gradient.  Shared by tests/test_prox_host.py (no GPU) and tests/test_gpu_prox.py (the device fit against this mirror fed by
the oracle).  Test infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('f_x', 'F_x', 'f_y', 't', 'tk', 'iters', 'nfev', 'nbt', 'restarts', 'phase', 'status', 'kkt', 'y_is_x', 'm_sd',
          'm_restart', 'm_zero', 'm_kkt')
SC = dict((n, i) for i, n in enumerate(FIELDS))
MARGINS = ('m_sd', 'm_restart', 'm_zero', 'm_kkt')
PHASE_Y, PHASE_TRIAL, PHASE_DONE = 0.0, 1.0, 2.0
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='prox_host_'), 'prox_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'prox_host.c'),
                               '-lm'])
        L = C.CDLL(so)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.prox_init.argtypes = [vp, i, i, vp, vp, i, i, i, i, vp, vp, d, i, vp]
        L.prox_step.argtypes = [vp, i, i, vp, vp, i, i, i, i, vp, vp, d, i, i, vp, vp]
        L.prox_apply.argtypes = [vp, i, i, i, i, d, d, d, d, vp]
        L.prox_apply.restype = i
        L.prox_allowance.restype = d
        L.prox_state_doubles.argtypes = [i, i]
        L.prox_state_doubles.restype = C.c_longlong
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def prox_apply(v, N, B, Dstim, mu, sigma, lam, t):
    """prox_{t h}(v) of one row by the machine's own group function."""
    v = np.ascontiguousarray(v, dtype=float)
    z = np.empty_like(v)
    rc = lib().prox_apply(_p(v), v.size, int(N), int(B), int(Dstim), float(mu), float(sigma), float(lam), float(t), _p(z))
    assert rc == 0, "prox_apply: v must hold 1 + Dstim + N B numbers, B <= 64"
    return z


class Mirror(object):
    """M rows of P = 1 + Dstim + N B parameters.  prior: (mu_b, sg_b, stim_sigma, mu, sigma); smooth_prior False: f = -ll
    (no terms for bias and stimulus weights).  target(X (M,P)) -> (ll (M,), grad (M,P)).  lam: a number or (M,)."""

    def __init__(self, target, X0, N, B, Dstim, prior, lam, gtol=1e-5, maxiter=500, max_backtrack=40, smooth_prior=True):
        self.lib = lib()
        self.target = target
        X0 = np.ascontiguousarray(X0, dtype=float)
        self.M, self.P = X0.shape
        M, P = self.M, self.P
        assert P == 1 + Dstim + N * B and self.lib.prox_nscal() == len(FIELDS)
        self.NBD = (int(N), int(B), int(Dstim))
        self.kind = 1 if smooth_prior else -1
        self.prm = np.array(prior, dtype=float)
        assert self.prm.shape == (5,)
        self.lam = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=float), (M,)))
        self.gtol, self.maxiter, self.max_backtrack = float(gtol), int(maxiter), int(max_backtrack)
        self.st = np.zeros(self.lib.prox_state_doubles(M, P))
        self.x = self.st[:M * P].reshape(M, P)
        self.gx = self.st[3 * M * P:4 * M * P].reshape(M, P)
        self.sc = self.st[5 * M * P:].reshape(len(FIELDS), M)
        self.x[:] = X0
        self.Xt = np.zeros((M, P))
        self.n_evals = 0
        self.F_trace = [[] for _ in range(M)]                  # F_x after every accepted step, row by row
        ll, grad = self._eval(self.x)
        self.lib.prox_init(_p(self.st), M, P, _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm), _p(self.lam), self.gtol,
                           self.maxiter, _p(self.Xt))

    def _eval(self, X):
        ll, grad = self.target(X.copy())
        self.n_evals += 1
        return np.ascontiguousarray(ll, dtype=float).copy(), np.ascontiguousarray(grad, dtype=float).copy()

    def field(self, name):
        return self.sc[SC[name]]

    def done(self):
        return bool(np.all(self.field('phase') == PHASE_DONE))

    def step(self):
        ll, grad = self._eval(self.Xt)
        F = np.zeros(self.M)
        self.lib.prox_step(_p(self.st), self.M, self.P, _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm), _p(self.lam),
                           self.gtol, self.maxiter, self.max_backtrack, _p(self.Xt), _p(F))
        for r in np.nonzero(~np.isnan(F))[0]:
            self.F_trace[r].append(F[r])

    def run(self, n_steps=None):
        """n_steps calls of the machine (None: until every row has ended)."""
        k = 0
        while (n_steps is None and not self.done()) or (n_steps is not None and k < n_steps):
            self.step()
            k += 1
            assert k < 10 ** 6
        return self

    def support(self):
        """(M, N) bool: the groups that are not exactly mu."""
        N, B, D = self.NBD
        return np.any(self.x[:, 1 + D:].reshape(self.M, N, B) != self.prm[3], axis=2)


# ---- the objective in numpy, for the tests' own checks ---------------------------------------------------------------
def oracle_target(probs, n_lo, n_hi):
    """target(X) for Mirror: ll and its gradient of neurons [n_lo, n_hi) from the C oracle, summed over the problems."""
    from oracle import c_oracle as CO

    def target(X):
        ll, g = 0.0, 0.0
        for p in probs:
            a, b = CO.ll_grad(p.S, p.fS, X, p.Weff, p.kind, p.dt, n_lo, n_hi, fstim=p.fstim)
            ll, g = ll + a, g + b
        return ll, g
    return target


def smooth_f_grad(target, X, Dstim, prior):
    """f (M,) and grad f (M, P) of pglm_prox.h from target's ll and gradient."""
    mu_b, sg_b, ss = prior[0], prior[1], prior[2]
    ll, g = target(np.ascontiguousarray(X))
    f = -ll + 0.5 * ((X[:, 0] - mu_b) / sg_b) ** 2 + 0.5 * np.sum((X[:, 1:1 + Dstim] / ss) ** 2, axis=1)
    G = -np.array(g)
    G[:, 0] += (X[:, 0] - mu_b) / sg_b ** 2
    G[:, 1:1 + Dstim] += X[:, 1:1 + Dstim] / ss ** 2
    return f, G


def h_value(X, N, B, Dstim, prior, lam):
    d = X[:, 1 + Dstim:].reshape(X.shape[0], N, B) - prior[3]
    nrm = np.sqrt(np.sum(d * d, axis=2))
    lam_s = np.broadcast_to(np.asarray(lam, dtype=float), (X.shape[0],)) / prior[4]
    with np.errstate(invalid='ignore'):
        return np.sum(np.where(nrm > 0.0, lam_s[:, None] * nrm, 0.0), axis=1)


def kkt_residual(X, G, N, B, Dstim, prior, lam):
    """The KKT residual of pglm_prox.h (step 5) from X and G = grad f, in numpy."""
    M = X.shape[0]
    mu, sigma = prior[3], prior[4]
    lam_s = np.broadcast_to(np.asarray(lam, dtype=float), (M,)) / sigma
    r = np.max(np.abs(G[:, :1 + Dstim]), axis=1)
    d = X[:, 1 + Dstim:].reshape(M, N, B) - mu
    gw = G[:, 1 + Dstim:].reshape(M, N, B)
    nrm = np.sqrt(np.sum(d * d, axis=2))
    with np.errstate(invalid='ignore', divide='ignore'):
        nz = np.max(np.abs(gw + lam_s[:, None, None] * d / nrm[:, :, None]), axis=2)
    zg = np.maximum(0.0, np.sqrt(np.sum(gw * gw, axis=2)) - lam_s[:, None])
    return np.maximum(r, np.max(np.where(nrm > 0.0, nz, zg), axis=1))


def prox_numpy(V, N, B, Dstim, prior, lam, t):
    """The closed form of prox_{t h}, row by row."""
    M = V.shape[0]
    mu, sigma = prior[3], prior[4]
    Z = V.copy()
    d = V[:, 1 + Dstim:].reshape(M, N, B) - mu
    nrm = np.sqrt(np.sum(d * d, axis=2))
    thr = t * np.broadcast_to(np.asarray(lam, dtype=float), (M,)) / sigma
    with np.errstate(invalid='ignore', divide='ignore'):
        fac = np.where(nrm > 0.0, np.maximum(0.0, 1.0 - thr[:, None] / nrm), 0.0)
    Z[:, 1 + Dstim:] = (mu + d * fac[:, :, None]).reshape(M, N * B)
    return Z
