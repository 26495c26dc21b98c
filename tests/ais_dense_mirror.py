"""The host mirror of the dense-mass annealed importance sampling run: theano_pyglm_amd/csrc/pglm_ais_dense.h compiled for the
host with gcc through tests/csrc/ais_dense_host.c, driven like tests/ais_mirror.py (whose Mirror it extends: same state
block, same init, start and temper, same target).  Shared by tests/test_ais_dense_host.py (no GPU) and
tests/test_gpu_ais_dense.py.  Test infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import ais_mirror as AM

ROOT = AM.ROOT
SC = AM.SC
_LIB = None
_p = AM._p


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='ais_dense_host_'), 'ais_dense_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so,
                               os.path.join(ROOT, 'tests', 'csrc', 'ais_dense_host.c'), '-lm'])
        L = C.CDLL(so)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.aisd_begin.argtypes = [vp, i, i, i, vp, vp]
        L.aisd_leap.argtypes = [vp, i, i, i, vp, vp, vp, i, i, i, vp, i, i, vp, vp, vp, vp]
        L.aisd_tempered_diag.argtypes = [i, i, vp, d, vp, d, vp, vp]
        _LIB = L
    return _LIB


def tempered_diag(P, Dstim, prm, beta, gdiag, floor):
    """csrc/pglm_ais_dense.h per element: (diag(beta G + Lambda), the fallback factor's diagonal) from diag G (P,)."""
    prm = np.ascontiguousarray(prm, dtype=float)
    gd = np.ascontiguousarray(gdiag, dtype=float)
    out, fb = np.zeros(P), np.zeros(P)
    lib().aisd_tempered_diag(int(P), int(Dstim), _p(prm), float(beta), _p(gd), float(floor), _p(out), _p(fb))
    return out, fb


class DenseMirror(AM.Mirror):
    """AM.Mirror with the inverse mass matrices W W^T, W (M, P, P) lower triangular, one per neuron, shared by its particles;
    self.p holds r = W^T p.  W: one stack for every temperature, or factors(j) -> the stack for the moves at betas[j]."""

    def __init__(self, target, K, M, prior, W, n_lo=0, particle0=0, step0=0.1, seed=0):
        AM.Mirror.__init__(self, target, K, M, prior, n_lo=n_lo, particle0=particle0, step0=step0, seed=seed)
        self.dlib = lib()
        self.factors = W if callable(W) else (lambda j: W)
        self.W = None

    def transition(self, n_leapfrog, adapt, acc_out=None, step_out=None):
        W = self.W
        assert W.shape == (self.M, self.P, self.P) and W.flags['C_CONTIGUOUS']
        self.dlib.aisd_begin(_p(self.st), self.K, self.M, self.P, _p(W), _p(self.Xt))
        margin = np.zeros(self.R)
        for i in range(n_leapfrog):
            ll, grad = self._eval(self.Xt)
            self.ll_seen.append(ll.copy())
            self.dlib.aisd_leap(_p(self.st), self.K, self.M, self.P, _p(W), _p(ll), _p(grad), *self.NBD, _p(self.prm),
                                1 if i == n_leapfrog - 1 else 0, 1 if adapt else 0, _p(self.Xt), _p(acc_out), _p(step_out),
                                _p(margin))
        return margin

    def run(self, betas, n_steps, n_leapfrog, adapt=False, step_table=None, on_temper=None):
        J = len(betas) - 1

        def temper(j, mir):
            if j < J:
                self.W = np.ascontiguousarray(self.factors(j), dtype=float)
            if on_temper is not None:
                on_temper(j, mir)
        return AM.Mirror.run(self, betas, n_steps, n_leapfrog, adapt=adapt, step_table=step_table, on_temper=temper)


def run_with_pilot(target, K, M, prior, W, betas, n_steps, n_leapfrog, step0=0.1, seed=0, n_lo=0, particle0=0):
    """AM.run_with_pilot with the dense mass: the pilot particle (index -1) runs on the same factors."""
    pilot = DenseMirror(target, 1, M, prior, W, n_lo=n_lo, particle0=-1, step0=step0, seed=seed)
    table = pilot.run(betas, n_steps, n_leapfrog, adapt=True)['steps']
    mir = DenseMirror(target, K, M, prior, W, n_lo=n_lo, particle0=particle0, step0=step0, seed=seed)
    out = mir.run(betas, n_steps, n_leapfrog, adapt=False, step_table=table)
    out['step_table'] = table
    return out
