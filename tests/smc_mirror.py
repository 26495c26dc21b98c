"""The host mirror of the adaptive sequential Monte Carlo run: theano_pyglm_amd/csrc/pglm_smc.h over pglm_ais.h compiled
for the host with gcc through tests/csrc/smc_host.c (which includes ais_host.c) and driven with numpy supplying ll and its
gradient.  Shared by tests/test_smc_host.py (no GPU) and tests/test_gpu_smc.py (the device against this mirror).  Test
infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests.ais_mirror import NVEC, SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = dict(beta=0, log_Z=1, step=2, stage=3, done=4, n_resampled=5, acc=6, live=7, rs=8, ess=9)
REC = dict(beta=0, ess=1, cess=2, resampled=3, accept_rate=4, step_sz=5)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='smc_host_'), 'smc_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'smc_host.c'),
                               '-lm'])
        L = C.CDLL(so)
        vp, u64, i, d = C.c_void_p, C.c_uint64, C.c_int, C.c_double
        L.ais_init.argtypes = [vp, i, i, i, i, i, i, i, i, vp, d, u64, vp]
        L.ais_start.argtypes = [vp, i, i, i, vp, vp, i, i, i, vp]
        L.ais_state_doubles.argtypes = [i, i]
        L.ais_state_doubles.restype = C.c_longlong
        L.smc_state_doubles.argtypes = [i, i, i, i]
        L.smc_state_doubles.restype = C.c_longlong
        L.smc_uniform.argtypes = [u64, u64, u64]
        L.smc_uniform.restype = d
        L.smc_init.argtypes = [vp, i, i, i, i, d]
        L.smc_stage_only.argtypes = [vp, vp, i, i, i, i, i, d, d, d, u64, vp]
        L.smc_gather_retemper.argtypes = [vp, vp, i, i, i, i, i, i, i, vp]
        L.smc_stage.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, i, d, d, d, u64, vp]
        L.smc_begin.argtypes = [vp, vp, i, i, i, i, vp, vp]
        L.smc_leap.argtypes = [vp, vp, i, i, i, i, vp, vp, vp, i, i, i, vp, i, vp, vp]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Blocks(object):
    """The two state blocks of K particles x M neurons with S stage records, as numpy views (the device's layout)."""

    def __init__(self, K, M, P, S):
        L = lib()
        self.K, self.M, self.P, self.S, self.R = K, M, P, S, K * M
        R = self.R
        assert L.smc_nscal() == len(NS)
        self.st = np.zeros(L.ais_state_doubles(R, P))
        self.smc = np.zeros(L.smc_state_doubles(K, M, P, S))
        self._views()

    def _views(self):
        K, M, P, S, R = self.K, self.M, self.P, self.S, self.R
        vec = self.st[:NVEC * R * P].reshape(NVEC, R, P)
        self.q, self.p, self.q0, self.g, self.gll, self.gu = vec
        self.sc = self.st[NVEC * R * P:].reshape(len(SC), R)
        o = len(NS) * M
        self.ns = self.smc[:o].reshape(len(NS), M)
        self.rec = self.smc[o:o + len(REC) * S * M].reshape(len(REC), S, M)
        o += len(REC) * S * M
        self.anc, self.w, self.acc = self.smc[o:o + R], self.smc[o + R:o + 2 * R], self.smc[o + 2 * R:o + 3 * R]
        self.nact = self.smc[o + 3 * R:o + 3 * R + 1]
        self.scratch = self.smc[o + 3 * R + 1:]

    def set(self, st, smc):
        self.st[:] = st
        self.smc[:] = smc


class Mirror(Blocks):
    """smc_glms on the host.  prior: (N, B, Dstim, (mu_b, sg_b, stim_sigma, mu, sigma, lam)), Gaussian.  target(X (M, P)) ->
    (ll (M,), grad (M, P)) is called once per particle block, as the device calls pgl_ll_grad_dev."""

    def __init__(self, target, K, M, prior, n_lo=0, step0=0.1, seed=0, minv=None, S=64, n_steps=1, n_leapfrog=5, cess=0.9,
                 ess_min=0.5, delta_min=1e-6):
        NBD = tuple(int(v) for v in prior[:3])
        Blocks.__init__(self, int(K), int(M), 1 + NBD[2] + NBD[0] * NBD[1], int(S))
        self.lib = lib()
        self.target, self.NBD, self.prm = target, NBD, np.array(prior[3], dtype=float)
        self.seed, self.n_steps, self.n_leapfrog = int(seed), int(n_steps), int(n_leapfrog)
        self.rho, self.ess_min, self.delta_min = float(cess), float(ess_min), float(delta_min)
        self.minv = None if minv is None else np.ascontiguousarray(minv, dtype=float)
        self.Xt = np.zeros((self.R, self.P))
        self.n_evals = 0
        self.lib.ais_init(_p(self.st), self.K, self.M, self.P, int(n_lo), 0, *NBD, _p(self.prm), float(step0), self.seed,
                          _p(self.Xt))
        self.lib.smc_init(_p(self.smc), self.K, self.M, self.P, self.S, float(step0))
        self.draws = self.q.copy()
        ll, grad = self._eval(self.Xt)
        self.ll_draws = ll.copy()
        self.lib.ais_start(_p(self.st), self.K, self.M, self.P, _p(ll), _p(grad), *NBD, _p(self.prm))

    def _eval(self, X):
        ll, grad = np.zeros(self.R), np.zeros((self.R, self.P))
        for k in range(self.K):
            s = slice(k * self.M, (k + 1) * self.M)
            a, b = self.target(X[s].copy())
            ll[s], grad[s] = a, b
        self.n_evals += 1
        return ll, grad

    def stage(self):
        """One stage call (three launches on the device) -> margins (2, M)."""
        margins = np.zeros((2, self.M))
        self.lib.smc_stage(_p(self.st), _p(self.smc), self.K, self.M, self.P, self.S, *self.NBD, _p(self.prm), self.n_steps,
                           self.rho, self.ess_min, self.delta_min, self.seed, _p(margins))
        return margins

    def stage_only(self):
        margins = np.zeros((2, self.M))
        self.lib.smc_stage_only(_p(self.st), _p(self.smc), self.K, self.M, self.P, self.S, self.n_steps, self.rho,
                                self.ess_min, self.delta_min, self.seed, _p(margins))
        return margins

    def gather_retemper(self):
        self.lib.smc_gather_retemper(_p(self.st), _p(self.smc), self.K, self.M, self.P, self.S, *self.NBD, _p(self.prm))

    def begin(self):
        self.lib.smc_begin(_p(self.st), _p(self.smc), self.K, self.M, self.P, self.S, _p(self.minv), _p(self.Xt))

    def leap(self, ll, grad, last, margin=None):
        ll, grad = np.ascontiguousarray(ll, dtype=float), np.ascontiguousarray(grad, dtype=float)
        self.lib.smc_leap(_p(self.st), _p(self.smc), self.K, self.M, self.P, self.S, _p(self.minv), _p(ll), _p(grad),
                          *self.NBD, _p(self.prm), 1 if last else 0, _p(self.Xt), _p(margin))

    def transition(self):
        self.begin()
        margin = np.zeros(self.R)
        for i in range(self.n_leapfrog):
            ll, grad = self._eval(self.Xt)
            self.leap(ll, grad, i == self.n_leapfrog - 1, margin)
        return margin

    def run(self, max_stages=None, on_stage=None):
        """The whole run -> the result dict of smc_glms (the parts the host can give)."""
        max_stages = self.S if max_stages is None else int(max_stages)
        n = 0
        while n < max_stages and self.nact[0] > 0.0:
            self.stage()
            n += 1
            if on_stage is not None:
                on_stage(n, self)
            if self.nact[0] == 0.0:
                break
            for _ in range(self.n_steps):
                self.transition()
        return self.result()

    def result(self):
        fin = self.ns[NS['done']] != 0.0
        S = int(self.ns[NS['stage']].max())
        lw = self.sc[SC['logw']].reshape(self.K, self.M).copy()
        return {'log_Z': np.where(fin, self.ns[NS['log_Z']], np.nan), 'finished': fin,
                'n_stages': self.ns[NS['stage']].astype(int), 'n_resampled': self.ns[NS['n_resampled']].astype(int),
                'betas': self.rec[REC['beta'], :S].copy(), 'ess': self.rec[REC['ess'], :S].copy(),
                'cess': self.rec[REC['cess'], :S].copy(), 'resampled': self.rec[REC['resampled'], :S] == 1.0,
                'accept_rate': self.rec[REC['accept_rate'], :S].copy(), 'step_sz': self.rec[REC['step_sz'], :S].copy(),
                'log_weights': normalise(lw), 'samples': self.q.reshape(self.K, self.M, self.P).copy(),
                'n_evals': self.n_evals}


def normalise(lw):
    """log weights (K, M) -> normalised over the particles; a column of -inf stays."""
    top = np.max(lw, axis=0)
    ok = np.isfinite(top)
    with np.errstate(invalid='ignore', divide='ignore'):
        z = np.where(ok, top + np.log(np.sum(np.exp(lw - np.where(ok, top, 0.0)), axis=0)), 0.0)
    return lw - z
