"""The host mirror of the device NUTS chain: theano_pyglm_amd/csrc/pglm_nuts.h compiled for the host with gcc through
tests/csrc/nuts_host.c (the way tests/hmc_mirror.py builds hmc_host.c) and driven with numpy supplying ll and its gradient.
Shared by tests/test_nuts_host.py (no GPU) and tests/test_gpu_nuts.py (the device chain against this mirror fed by the
oracle).  Test infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('Uc H0 step t neuron seed_lo seed_hi done depth v i lw_tree lw_sub Us sum_acc n_leaf sel sel_sub hbar logeps_bar mu '
          'n_leapfrog n_div acc_post last_depth last_nleaf last_stop last_sel last_acc ve').split()
SC = dict((n, k) for k, n in enumerate(FIELDS))
NVEC = 17
QC = 0
END, DONE = 8, 64
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='nuts_host_'), 'nuts_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'nuts_host.c'),
                               '-lm'])
        L = C.CDLL(so)
        vp, u64, ci, cd = C.c_void_p, C.c_uint64, C.c_int, C.c_double
        L.nuts_init.argtypes = [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, u64, ci, vp, vp]
        L.nuts_step.argtypes = [vp, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, cd, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.nuts_uniform.argtypes = [u64] * 4
        L.nuts_uniform.restype = cd
        L.nuts_normal.argtypes = [u64] * 4
        L.nuts_normal.restype = cd
        L.nuts_state_doubles.argtypes = [ci, ci, ci]
        L.nuts_state_doubles.restype = C.c_longlong
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def draws(seed, neuron, t, P, max_depth):
    """The stateless draws of transition t of a neuron's row, in inference/nuts.py: nuts_transition's argument order."""
    L = lib()
    z = np.array([L.nuts_normal(seed, neuron, t, j) for j in range(P)])
    u_dir = np.array([L.nuts_uniform(seed, neuron, t, 2 * P + 1 + d) for d in range(max_depth)])
    u_merge = np.array([L.nuts_uniform(seed, neuron, t, 2 * P + 17 + d) for d in range(max_depth)])
    u_leaf = np.array([L.nuts_uniform(seed, neuron, t, 2 * P + 33 + k) for k in range(2 ** max_depth - 1)])
    return z, u_dir, u_merge, u_leaf


class Mirror(object):
    """M rows of P parameters, neurons n_lo .. n_lo + M - 1.  prior: None (ll is the whole log density) or
    (kind, N, B, Dstim, (mu_b, sg_b, stim_sigma, mu, sigma, lam)).  target(X (M,P)) -> (ll (M,), grad (M,P)).
    W (M,P,P) or minv (M,P) or neither.  The chain: n_warmup + n_keep * thin transitions per row."""

    def __init__(self, target, X0, n_keep, n_warmup=0, thin=1, max_depth=8, n_lo=0, prior=None, step0=0.1, seed=0, minv=None,
                 W=None, delta=0.8):
        self.lib = lib()
        self.target = target
        X0 = np.ascontiguousarray(X0, dtype=float)
        self.M, self.P = M, P = X0.shape
        self.D = D = int(max_depth)
        assert self.lib.nuts_nscal() == len(FIELDS) and self.lib.nuts_nvec() == NVEC
        self.st = np.zeros(self.lib.nuts_state_doubles(M, P, D))
        self.vec = self.st[:(NVEC + 2 * D) * M * P].reshape(NVEC + 2 * D, M, P)
        self.sc = self.st[(NVEC + 2 * D) * M * P:].reshape(len(FIELDS), M)
        self.vec[QC] = X0
        if prior is None:
            self.kind, self.NBD, self.prm = -1, (0, 0, 0), np.zeros(6)
        else:
            self.kind, self.NBD, self.prm = int(prior[0]), tuple(int(v) for v in prior[1:4]), np.array(prior[4], dtype=float)
            assert P == 1 + self.NBD[2] + self.NBD[0] * self.NBD[1]
        self.minv = None if minv is None else np.ascontiguousarray(minv, dtype=float)
        self.W = None if W is None else np.ascontiguousarray(W, dtype=float)
        self.n_keep, self.n_warmup, self.thin, self.delta = int(n_keep), int(n_warmup), int(thin), float(delta)
        self.Xt = np.zeros((M, P))
        self.tmp = np.zeros(P)
        self.samples = np.zeros((self.n_keep, M, P))
        self.stats = np.zeros((self.n_keep, 2, M))
        self.mg = np.full((M, 4), np.inf)                      # smallest margins; [:, 3]: leaves with a non-finite H
        self.mg[:, 3] = 0.0
        self.acts = np.zeros(M, dtype=np.int32)
        self.n_evals = 0
        self.log = [[] for _ in range(M)]                       # per row: one dict per completed transition
        step = np.ascontiguousarray(np.broadcast_to(np.asarray(step0, dtype=float), (M,)))
        ll, grad = self._eval(self.vec[QC])
        self.lib.nuts_init(_p(self.st), M, P, D, int(n_lo), _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm), _p(self.W),
                           _p(self.minv), _p(step), int(seed), self.n_warmup + self.n_keep * self.thin, _p(self.Xt),
                           _p(self.tmp))

    def _eval(self, X):
        ll, grad = self.target(X.copy())
        self.n_evals += 1
        return np.ascontiguousarray(ll, dtype=float).copy(), np.ascontiguousarray(grad, dtype=float).copy()

    def done(self):
        return self.sc[SC['done']] != 0.0

    def step(self):
        """One evaluation and one leapfrog step of every row that is not done."""
        ll, grad = self._eval(self.Xt)
        self.lib.nuts_step(_p(self.st), self.M, self.P, self.D, _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm),
                           _p(self.W), _p(self.minv), self.delta, self.n_warmup, self.thin, self.n_keep, _p(self.Xt),
                           _p(self.samples), _p(self.stats), _p(self.mg), _p(self.acts), _p(self.tmp))
        for r in np.flatnonzero(self.acts & END):
            self.log[r].append({'depth': int(self.sc[SC['last_depth'], r]), 'n_leaf': int(self.sc[SC['last_nleaf'], r]),
                                'stop': int(self.sc[SC['last_stop'], r]), 'sel': int(self.sc[SC['last_sel'], r]),
                                'alpha': float(self.sc[SC['last_acc'], r]), 'step': float(self.sc[SC['step'], r]),
                                'q': self.vec[QC, r].copy(), 'launch': self.n_evals - 1})
        return self.acts.copy()

    def run(self, limit=10 ** 7):
        """To the end of every row's chain.  -> number of steps."""
        n = 0
        while not self.done().all():
            self.step()
            n += 1
            assert n < limit
        return n
