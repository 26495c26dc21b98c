"""The host mirror of the warm-up mass adaptation: theano_pyglm_amd/csrc/pglm_adapt.h compiled for the host with gcc through
tests/csrc/adapt_host.c, on top of the HMC and NUTS mirrors (tests/hmc_mirror.py, tests/nuts_mirror.py).  Shared by
tests/test_adapt_host.py (no GPU) and tests/test_gpu_adapt.py (the device chains against these mirrors).  Test
infrastructure."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import hmc_mirror as HM
from tests import nuts_mirror as NM
from theano_pyglm_amd.inference import mass_adapt as MA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_p = HM._p


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix='adapt_host_'), 'adapt_host.so')
        subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tests', 'csrc', 'adapt_host.c'),
                               '-lm'])
        L = C.CDLL(so)
        vp, u64, ci, cd = C.c_void_p, C.c_uint64, C.c_int, C.c_double
        L.adapt_state_doubles.argtypes = [ci, ci]
        L.adapt_state_doubles.restype = C.c_longlong
        L.adapt_chain_seed.argtypes = [u64, u64]
        L.adapt_chain_seed.restype = u64
        L.adapt_minv.argtypes = [cd, cd]
        L.adapt_minv.restype = cd
        L.adapt_welford.argtypes = [cd, cd, vp, vp]
        for name in ('adapt_restart_hmc', 'adapt_restart_nuts'):
            getattr(L, name).argtypes = [vp]
        for name in ('adapt_fresh_hmc', 'adapt_fresh_nuts'):
            getattr(L, name).argtypes = [vp, cd]
        L.adapt_hmc_step.argtypes = [vp, ci, ci, vp, vp, vp]
        L.adapt_nuts_step.argtypes = [vp, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, cd, ci, ci, ci, vp, vp, vp, vp, vp]
        _LIB = L
    return _LIB


class Adapt(object):
    """The adaptation state of R rows of P parameters for a warm-up of n_warmup transitions."""

    def __init__(self, R, P, n_warmup):
        self.lib = lib()
        self.windows = MA.adapt_windows(n_warmup)
        self.sched = MA.schedule_ints(self.windows)
        self.st = np.zeros(self.lib.adapt_state_doubles(R, P))
        self.mean = self.st[:R * P].reshape(R, P)
        self.m2 = self.st[R * P:2 * R * P].reshape(R, P)
        self.count = self.st[2 * R * P:2 * R * P + R]
        self.widx = self.st[2 * R * P + R:]
        self.minv = np.ones((R, P))


class HmcMirror(HM.Mirror):
    """hmc_mirror.Mirror under mass='adapt': the adaptation step after every transition."""

    def __init__(self, target, X0, n_warmup, **kw):
        assert kw.get('minv') is None
        HM.Mirror.__init__(self, target, X0, **kw)
        self.ad = Adapt(self.M, self.P, n_warmup)
        self.minv = self.ad.minv
        self.n_warmup = int(n_warmup)

    def transition(self, n_leapfrog, n_warmup=None, p_in=None):
        out = HM.Mirror.transition(self, n_leapfrog, self.n_warmup, p_in)
        self.ad.lib.adapt_hmc_step(_p(self.st), self.M, self.P, _p(self.ad.st), _p(self.ad.sched), _p(self.minv))
        return out


class NutsMirror(NM.Mirror):
    """nuts_mirror.Mirror under mass='adapt' (diagonal): adapt_nuts_step instead of nuts_step."""

    def __init__(self, target, X0, n_keep, n_warmup, **kw):
        assert kw.get('minv') is None and kw.get('W') is None
        R, P = np.shape(X0)
        self.ad = Adapt(R, P, n_warmup)
        kw['minv'] = self.ad.minv
        NM.Mirror.__init__(self, target, X0, n_keep, n_warmup=n_warmup, **kw)
        self.minv = self.ad.minv                                  # (the array the chain reads IS the one adaptation rewrites)

    def step(self):
        ll, grad = self._eval(self.Xt)
        self.ad.lib.adapt_nuts_step(_p(self.st), self.M, self.P, self.D, _p(ll), _p(grad), self.kind, *self.NBD, _p(self.prm),
                                    _p(self.minv), _p(self.ad.st), _p(self.ad.sched), self.delta, self.n_warmup, self.thin,
                                    self.n_keep, _p(self.Xt), _p(self.samples), _p(self.stats), _p(self.acts), _p(self.tmp))
        SC = NM.SC
        for r in np.flatnonzero(self.acts & NM.END):
            self.log[r].append({'depth': int(self.sc[SC['last_depth'], r]), 'n_leaf': int(self.sc[SC['last_nleaf'], r]),
                                'stop': int(self.sc[SC['last_stop'], r]), 'sel': int(self.sc[SC['last_sel'], r]),
                                'alpha': float(self.sc[SC['last_acc'], r]), 'step': float(self.sc[SC['step'], r]),
                                'q': self.vec[NM.QC, r].copy(), 'launch': self.n_evals - 1,
                                'minv': self.minv[r].copy()})
        return self.acts.copy()
