"""The host mirror of the lock-step HMC chain: theano_pyglm_amd/csrc/pglm_hmc.h compiled for the host with gcc through
tests/csrc/hmc_host.c (the way tests/test_newton_cg_host.py builds ncg_host.c) and driven with numpy supplying ll and its
gradient.  Shared by tests/test_hmc_host.py (no GPU) and tests/test_gpu_hmc.py (the device chain against this mirror fed by
the oracle).  Test infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = dict(U0=0, H0=1, step=2, avg_accept=3, n_accept=4, t=5, acc=6, neuron=7, seed_lo=8, seed_hi=9)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='hmc_host_'), 'hmc_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'hmc_host.c'),
                               '-lm'])
        L = C.CDLL(so)
        vp, u64 = C.c_void_p, C.c_uint64
        L.hmc_init.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_double, u64]
        L.hmc_begin.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
        L.hmc_leap.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                               vp, vp, vp]
        L.hmc_normal.argtypes = [u64] * 4
        L.hmc_normal.restype = C.c_double
        L.hmc_uniform.argtypes = [u64] * 3
        L.hmc_uniform.restype = C.c_double
        L.hmc_state_doubles.argtypes = [C.c_int, C.c_int]
        L.hmc_state_doubles.restype = C.c_longlong
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Mirror(object):
    """M rows of P parameters, neurons n_lo .. n_lo + M - 1.  prior: None (ll is the whole log density) or
    (kind, N, B, Dstim, (mu_b, sg_b, stim_sigma, mu, sigma, lam)).  target(X (M,P)) -> (ll (M,), grad (M,P))."""

    def __init__(self, target, X0, n_lo=0, prior=None, step0=0.1, seed=0, minv=None):
        self.lib = lib()
        self.target = target
        X0 = np.ascontiguousarray(X0, dtype=float)
        self.M, self.P = X0.shape
        M, P = self.M, self.P
        assert self.lib.hmc_nscal() == len(SC)
        self.st = np.zeros(self.lib.hmc_state_doubles(M, P))
        self.q = self.st[:M * P].reshape(M, P)
        self.p = self.st[M * P:2 * M * P].reshape(M, P)
        self.g = self.st[3 * M * P:4 * M * P].reshape(M, P)
        self.sc = self.st[4 * M * P:].reshape(len(SC), M)
        self.q[:] = X0
        if prior is None:
            self.kind, self.NBD, self.prm = -1, (0, 0, 0), np.zeros(6)
        else:
            self.kind, self.NBD, self.prm = int(prior[0]), tuple(int(v) for v in prior[1:4]), np.array(prior[4], dtype=float)
            assert P == 1 + self.NBD[2] + self.NBD[0] * self.NBD[1]
        self.minv = None if minv is None else np.ascontiguousarray(minv, dtype=float)
        self.Xt = np.zeros((M, P))
        self.n_evals = 0
        ll, grad = self._eval(self.q)
        self.lib.hmc_init(_p(self.st), M, P, int(n_lo), _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm), float(step0),
                          int(seed))

    def _eval(self, X):
        ll, grad = self.target(X.copy())
        self.n_evals += 1
        return np.ascontiguousarray(ll, dtype=float).copy(), np.ascontiguousarray(grad, dtype=float).copy()

    def begin(self, p_in=None):
        """p_in (M,P): momenta to use instead of the stateless draw (tests only)."""
        pin = None if p_in is None else np.ascontiguousarray(p_in, dtype=float)
        self.lib.hmc_begin(_p(self.st), self.M, self.P, _p(self.minv), _p(self.Xt), _p(pin))

    def leap(self, last, n_warmup=0):
        ll, grad = self._eval(self.Xt)
        margin = np.zeros(self.M)
        sample = np.zeros((self.M, self.P))
        self.lib.hmc_leap(_p(self.st), self.M, self.P, _p(self.minv), _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm),
                          1 if last else 0, int(n_warmup), _p(self.Xt), _p(sample), _p(margin))
        return sample, margin

    def transition(self, n_leapfrog, n_warmup=0, p_in=None):
        """-> (q (M,P) after the transition, accepted (M,) bool, margin (M,) = |log u - (H0 - H1)|)."""
        self.begin(p_in)
        for i in range(n_leapfrog):
            sample, margin = self.leap(i == n_leapfrog - 1, n_warmup)
        return sample, self.sc[SC['acc']] != 0.0, margin

    def run(self, n_transitions, n_leapfrog, n_warmup=0):
        """-> (samples (n, M, P), accepted (n, M) bool, margins (n, M))."""
        out = [self.transition(n_leapfrog, n_warmup) for _ in range(n_transitions)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
