"""The host mirror of the annealed importance sampling run: theano_pyglm_amd/csrc/pglm_ais.h compiled for the host with
gcc through tests/csrc/ais_host.c (the way tests/hmc_mirror.py builds hmc_host.c) and driven with numpy supplying ll and
its gradient.  Shared by tests/test_ais_host.py (no GPU) and tests/test_gpu_ais.py (the device run against this mirror fed
by the oracle).  Test infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = dict(U0=0, H0=1, step=2, avg_accept=3, n_accept=4, t=5, acc=6, neuron=7, seed_lo=8, seed_hi=9, ll0=10, lp0=11, beta=12,
          logw=13, particle=14)
NVEC = 6
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='ais_host_'), 'ais_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'ais_host.c'),
                               '-lm'])
        L = C.CDLL(so)
        vp, u64, i, d = C.c_void_p, C.c_uint64, C.c_int, C.c_double
        L.ais_init.argtypes = [vp, i, i, i, i, i, i, i, i, vp, d, u64, vp]
        L.ais_start.argtypes = [vp, i, i, i, vp, vp, i, i, i, vp]
        L.ais_temper.argtypes = [vp, i, i, i, i, i, i, vp, d, vp]
        L.ais_begin.argtypes = [vp, i, i, i, vp, vp]
        L.ais_leap.argtypes = [vp, i, i, i, vp, vp, vp, i, i, i, vp, i, i, vp, vp, vp, vp]
        L.ais_normal.argtypes = [u64, C.c_longlong, u64, u64, u64]
        L.ais_normal.restype = d
        L.ais_state_doubles.argtypes = [i, i]
        L.ais_state_doubles.restype = C.c_longlong
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Mirror(object):
    """K particles (particle0 ..) of M neurons (n_lo ..), rows particle-major.  prior: (N, B, Dstim, (mu_b, sg_b, stim_sigma,
    mu, sigma, lam)), Gaussian.  target(X (M,P)) -> (ll (M,), grad (M,P)) is called once per particle block, as the device
    calls pgl_ll_grad_dev."""

    def __init__(self, target, K, M, prior, n_lo=0, particle0=0, step0=0.1, seed=0, minv=None):
        self.lib = lib()
        self.target = target
        self.K, self.M = int(K), int(M)
        self.NBD, self.prm = tuple(int(v) for v in prior[:3]), np.array(prior[3], dtype=float)
        self.P = P = 1 + self.NBD[2] + self.NBD[0] * self.NBD[1]
        self.R = R = self.K * self.M
        assert self.lib.ais_nscal() == len(SC)
        self.st = np.zeros(self.lib.ais_state_doubles(R, P))
        vec = self.st[:NVEC * R * P].reshape(NVEC, R, P)
        self.q, self.p, self.q0, self.g, self.gll, self.gu = vec
        self.sc = self.st[NVEC * R * P:].reshape(len(SC), R)
        self.minv = None if minv is None else np.ascontiguousarray(minv, dtype=float)
        assert self.minv is None or self.minv.shape == (M, P)
        self.Xt = np.zeros((R, P))
        self.n_evals = 0
        self.lib.ais_init(_p(self.st), self.K, self.M, P, int(n_lo), int(particle0), *self.NBD, _p(self.prm), float(step0),
                          int(seed), _p(self.Xt))
        self.draws = self.q.copy()
        ll, grad = self._eval(self.Xt)
        self.ll_seen = [ll.copy()]
        self.lib.ais_start(_p(self.st), self.K, self.M, P, _p(ll), _p(grad), *self.NBD, _p(self.prm))

    def _eval(self, X):
        ll, grad = np.zeros(self.R), np.zeros((self.R, self.P))
        for k in range(self.K):
            s = slice(k * self.M, (k + 1) * self.M)
            a, b = self.target(X[s].copy())
            ll[s], grad[s] = a, b
        self.n_evals += 1
        return ll, grad

    def temper(self, beta, step_row=None):
        sr = None if step_row is None else np.ascontiguousarray(step_row, dtype=float)
        assert sr is None or sr.shape == (self.M,)
        self.lib.ais_temper(_p(self.st), self.K, self.M, self.P, *self.NBD, _p(self.prm), float(beta), _p(sr))

    def transition(self, n_leapfrog, adapt, acc_out=None, step_out=None):
        """-> margins (R,) = |log u - (H0 - H1)| of the decisions."""
        self.lib.ais_begin(_p(self.st), self.K, self.M, self.P, _p(self.minv), _p(self.Xt))
        margin = np.zeros(self.R)
        for i in range(n_leapfrog):
            ll, grad = self._eval(self.Xt)
            self.ll_seen.append(ll.copy())
            self.lib.ais_leap(_p(self.st), self.K, self.M, self.P, _p(self.minv), _p(ll), _p(grad), *self.NBD, _p(self.prm),
                              1 if i == n_leapfrog - 1 else 0, 1 if adapt else 0, _p(self.Xt), _p(acc_out), _p(step_out),
                              _p(margin))
        return margin

    def run(self, betas, n_steps, n_leapfrog, adapt=False, step_table=None, on_temper=None):
        """The whole ladder.  step_table (J-1, M) or None.  -> dict: log_weights (K, M), samples (K, M, P), accepts
        (J-1, R) counts, steps (J-1, R) each row's step after the temperature's last transition, margins
        ((J-1) n_steps, R), accepted ((J-1) n_steps, R) bool."""
        betas = np.asarray(betas, dtype=float)
        J = betas.size - 1
        accepts, steps = np.zeros((max(J - 1, 0), self.R)), np.zeros((max(J - 1, 0), self.R))
        margins, accepted = [], []
        for j in range(1, J + 1):
            row = None if (step_table is None or j == J) else np.asarray(step_table, dtype=float)[j - 1]
            self.temper(betas[j], row)
            if on_temper is not None:
                on_temper(j, self)
            if j == J:
                break
            for _ in range(n_steps):
                margins.append(self.transition(n_leapfrog, adapt, accepts[j - 1], steps[j - 1]))
                accepted.append(self.sc[SC['acc']] != 0.0)
        return {'log_weights': self.sc[SC['logw']].reshape(self.K, self.M).copy(),
                'samples': self.q.reshape(self.K, self.M, self.P).copy(), 'accepts': accepts, 'steps': steps,
                'margins': np.array(margins).reshape(-1, self.R), 'accepted': np.array(accepted, dtype=bool).reshape(-1, self.R)}


def run_with_pilot(target, K, M, prior, betas, n_steps, n_leapfrog, step0=0.1, seed=0, minv=None, n_lo=0, particle0=0):
    """What inference/batched_ais.py: ais_glms does, on the host: one adapting pilot particle (particle index -1) whose
    weights are discarded gives the (J-1, M) step table, then K particles run frozen on it."""
    pilot = Mirror(target, 1, M, prior, n_lo=n_lo, particle0=-1, step0=step0, seed=seed, minv=minv)
    table = pilot.run(betas, n_steps, n_leapfrog, adapt=True)['steps']
    mir = Mirror(target, K, M, prior, n_lo=n_lo, particle0=particle0, step0=step0, seed=seed, minv=minv)
    out = mir.run(betas, n_steps, n_leapfrog, adapt=False, step_table=table)
    out['step_table'] = table
    return out
