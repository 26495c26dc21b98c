"""The host mirror of the dense-mass HMC chain: theano_pyglm_amd/csrc/pglm_hmc_dense.h compiled for the host with gcc through
tests/csrc/hmc_dense_host.c, driven like tests/hmc_mirror.py (whose Mirror it extends: same state block, same init, same
target).  Shared by tests/test_hmc_dense_host.py (no GPU) and tests/test_gpu_hmc_dense.py.  Test infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import hmc_mirror as HM

ROOT = HM.ROOT
SC = HM.SC
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='hmc_dense_host_'), 'hmc_dense_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so,
                               os.path.join(ROOT, 'tests', 'csrc', 'hmc_dense_host.c'), '-lm'])
        L = C.CDLL(so)
        vp = C.c_void_p
        L.hmcd_tri_matvec.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
        L.hmcd_begin.argtypes = [vp, C.c_int, C.c_int, vp, vp]
        L.hmcd_leap.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                vp, vp, vp]
        _LIB = L
    return _LIB


_p = HM._p


def tri_matvec(W, x, trans):
    """The mirror's product: y (M, P) = W x or W^T x, lower triangle only."""
    W = np.ascontiguousarray(W, dtype=float)
    x = np.ascontiguousarray(x, dtype=float)
    M, P = x.shape
    assert W.shape == (M, P, P)
    y = np.zeros((M, P))
    lib().hmcd_tri_matvec(_p(W), M, P, 1 if trans else 0, _p(x), _p(y))
    return y


class DenseMirror(HM.Mirror):
    """HM.Mirror with the inverse mass matrices W W^T, W (M, P, P) lower triangular; self.p holds r = W^T p."""

    def __init__(self, target, X0, W, n_lo=0, prior=None, step0=0.1, seed=0):
        HM.Mirror.__init__(self, target, X0, n_lo=n_lo, prior=prior, step0=step0, seed=seed)
        self.dlib = lib()
        self.W = np.ascontiguousarray(W, dtype=float)
        assert self.W.shape == (self.M, self.P, self.P)

    def begin(self, p_in=None):
        assert p_in is None
        self.dlib.hmcd_begin(_p(self.st), self.M, self.P, _p(self.W), _p(self.Xt))

    def leap(self, last, n_warmup=0):
        ll, grad = self._eval(self.Xt)
        margin = np.zeros(self.M)
        sample = np.zeros((self.M, self.P))
        self.dlib.hmcd_leap(_p(self.st), self.M, self.P, _p(self.W), _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm),
                            1 if last else 0, int(n_warmup), _p(self.Xt), _p(sample), _p(margin))
        return sample, margin
