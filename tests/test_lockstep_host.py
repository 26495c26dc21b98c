"""Host tests of what the lock-step drivers share (inference/lockstep.py: session; batched_hmc.resolve_mass) on stub
population, handle and torch objects.  No GPU needed."""
import sys
import types

import numpy as np
import pytest


class _Stream(object):
    made = 0

    def __init__(self, dev):
        _Stream.made += 1
        self.dev, self.cuda_stream, self.log = dev, 1000 + _Stream.made, []

    def wait_stream(self, other):
        self.log.append(('wait_stream', other))

    def synchronize(self):
        self.log.append('synchronize')


class _StreamContext(object):
    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        self.stream.log.append('enter')

    def __exit__(self, *exc):
        self.stream.log.append('exit')
        return False


def _stub_torch():
    torch = types.ModuleType('torch')
    torch.device = lambda kind, index: types.SimpleNamespace(type=kind, index=index)
    torch.cuda = types.SimpleNamespace(Stream=_Stream, current_stream=lambda dev: ('current', dev.index), stream=_StreamContext)
    return torch


class _Handle(object):
    def __init__(self):
        self.streams = []

    def set_stream(self, s):
        self.streams.append(s)


class _Population(object):
    def __init__(self, n_seq=2, device=0):
        self.device = device
        self.data_sequences = ['data%d' % i for i in range(n_seq)]
        self.handles = dict((d, _Handle()) for d in self.data_sequences)
        self.set = []

    def set_data(self, data):
        self.set.append(data)

    def _handle(self, data):
        assert self.set[-1] == data                             # (the handle of the sequence that was just set)
        return self.handles[data]


@pytest.fixture
def lockstep(monkeypatch):
    from theano_pyglm_amd.inference import lockstep as LS
    monkeypatch.setitem(sys.modules, 'torch', _stub_torch())
    monkeypatch.setattr(LS, '_STREAMS', {})
    return LS


def test_session_switches_the_handles_and_puts_them_back(lockstep):
    popn = _Population()
    with lockstep.session(popn) as (torch, dev, stream, handles):
        assert torch is sys.modules['torch'] and dev.index == 0
        assert handles == [popn.handles[d] for d in popn.data_sequences]
        assert all(h.streams == [stream.cuda_stream] for h in handles)
        # behind whatever the caller queued, and the drivers' stream is torch's current one inside the block
        assert stream.log == [('wait_stream', ('current', 0)), 'enter']
    assert stream.log[2:] == ['exit', 'synchronize']
    assert all(h.streams == [stream.cuda_stream, None] for h in handles)


def test_session_cleans_up_behind_an_exception(lockstep):
    popn = _Population()
    seen = {}
    with pytest.raises(KeyError, match="from the block"):
        with lockstep.session(popn) as (_, _, stream, handles):
            seen['stream'], seen['handles'] = stream, handles
            raise KeyError("from the block")
    assert seen['stream'].log[2:] == ['exit', 'synchronize']
    assert all(h.streams == [seen['stream'].cuda_stream, None] for h in seen['handles'])


def test_session_survives_a_failing_synchronize(lockstep, monkeypatch):
    """The synchronisation on the way out is best effort (a device error is already on its way to the caller): the handles
    still go back to their own streams, and the block's exception is the one that propagates."""
    def broken(self):
        raise RuntimeError("device lost")
    monkeypatch.setattr(_Stream, 'synchronize', broken)
    popn = _Population(1)
    with pytest.raises(KeyError):
        with lockstep.session(popn):
            raise KeyError("from the block")
    assert popn.handles['data0'].streams[-1] is None


def test_session_keeps_one_stream_per_device(lockstep):
    with lockstep.session(_Population()) as (_, _, first, _):
        pass
    with lockstep.session(_Population(1)) as (_, _, second, _):
        pass
    with lockstep.session(_Population(1, device=1)) as (_, _, other, _):
        pass
    assert second is first and other is not first
    assert set(lockstep._STREAMS) == {0, 1}


def test_the_drivers_share_the_one_stream_cache():
    from theano_pyglm_amd.inference import (batched_ais, batched_bfgs, batched_hmc, batched_newton_cg, batched_nuts,
                                            batched_prox, lockstep)
    for mod in (batched_ais, batched_bfgs, batched_hmc, batched_newton_cg, batched_nuts, batched_prox):
        assert not hasattr(mod, '_STREAMS') and mod.session is lockstep.session


# ---- resolve_mass ------------------------------------------------------------------------------------------------
class _NoHessians(object):
    """A population of P = 5 parameters per neuron whose Hessian routines must not be reached."""
    N = 4
    glm = types.SimpleNamespace(P=5)

    def compute_hessian_packed(self, *a, **kw):
        raise AssertionError("a Hessian was asked for")


def _no_hessians(monkeypatch):
    from theano_pyglm_amd.inference import batched_ais, batched_hmc, laplace

    def refuse(*a, **kw):
        raise AssertionError("a Hessian routine was called")
    for mod, name in ((batched_hmc, '_laplace_minv'), (batched_hmc, '_laplace_rows'), (batched_hmc, '_laplace_dense_factor'),
                      (batched_hmc, '_laplace_dense_factor_device'), (batched_ais, '_ll_hessians'),
                      (laplace, 'laplace_on_device')):
        monkeypatch.setattr(mod, name, refuse)
    return _NoHessians()


def test_resolve_mass_errors(monkeypatch):
    from theano_pyglm_amd.inference.batched_hmc import resolve_mass
    popn = _no_hessians(monkeypatch)
    for bad in (np.ones((3, 4)), np.ones((2, 5)), np.ones(5), 2.0):               # M = 3, P = 5
        with pytest.raises(ValueError, match=r"mass: an \(M, P\) = \(3, 5\) array of positive inverse masses"):
            resolve_mass(popn, None, bad, 1, 4, 1e-8)
    for entry in (0.0, -1.0, np.nan, np.inf):
        m = np.ones((3, 5))
        m[1, 2] = entry
        with pytest.raises(ValueError, match=r"mass: an \(M, P\) = \(3, 5\) array of positive inverse masses"):
            resolve_mass(popn, None, m, 1, 4, 1e-8)
    for bad in (np.ones((3, 5, 4)), np.ones((2, 5, 5)), np.ones((3, 4, 4))):
        with pytest.raises(ValueError, match=r"mass: an \(M, P, P\) = \(3, 5, 5\) array of inverse mass matrices"):
            resolve_mass(popn, None, bad, 1, 4, 1e-8)
    for dense in ('laplace', 'tempered'):
        with pytest.raises(ValueError, match=r"mass: None, 'laplace', 'laplace_dense', an \(M, P\) or an \(M, P, P\) array"):
            resolve_mass(popn, None, 'dense', 1, 4, 1e-8, dense=dense)
    S = np.tile(np.eye(5), (3, 1, 1))
    S[2, 0, 1] = 0.5                                            # not symmetric: factor_inverse_mass's own message
    with pytest.raises(ValueError, match="not symmetric"):
        resolve_mass(popn, None, S, 1, 4, 1e-8)


def test_resolve_mass_forms(monkeypatch):
    from theano_pyglm_amd.inference import batched_hmc as B
    popn = _no_hessians(monkeypatch)
    assert B.resolve_mass(popn, None, None, 0, 4, 1e-8)[:3] == (None, None, None)
    m = 0.5 + np.arange(15.0).reshape(3, 5)
    minv, factor, dense_rows, setup_s = B.resolve_mass(popn, None, m.tolist(), 1, 4, 1e-8)
    assert np.array_equal(minv, m) and minv.flags['C_CONTIGUOUS'] and minv.dtype == float
    assert factor is None and dense_rows is None and setup_s >= 0.0
    A = np.random.default_rng(3).standard_normal((3, 5, 5))
    S = A @ np.swapaxes(A, 1, 2) + 5.0 * np.eye(5)
    minv, factor, dense_rows, _ = B.resolve_mass(popn, None, S, 1, 4, 1e-8)
    assert minv is None and dense_rows is None and np.array_equal(factor, B.factor_inverse_mass(S))
    # the tempered dense mass of annealed importance sampling: a marker, and no Hessian routine runs
    for on_device in (False, True):
        assert B.resolve_mass(popn, None, 'laplace_dense', 1, 4, 1e-8, factor_on_device=on_device, dense='tempered')[:3] == \
            (None, 'tempered', None)


def test_resolve_mass_laplace_routes(monkeypatch):
    """'laplace' and 'laplace_dense' go to the helpers of batched_hmc (where tests and tools patch and import them), with
    the range and the floor; the time they take is setup_s."""
    from theano_pyglm_amd.inference import batched_hmc as B
    calls = []

    def helper(name, result):
        def f(population, x, n_lo, n_hi, floor):
            calls.append((name, x, n_lo, n_hi, floor))
            return result
        return f
    W, rows = np.zeros((3, 5, 5)), np.array([True, False, True])
    monkeypatch.setattr(B, '_laplace_minv', helper('minv', np.full((3, 5), 2.0)))
    monkeypatch.setattr(B, '_laplace_dense_factor', helper('host', (W, rows)))
    monkeypatch.setattr(B, '_laplace_dense_factor_device', helper('device', (W, rows)))
    popn = _NoHessians()
    minv, factor, dense_rows, _ = B.resolve_mass(popn, 'x', 'laplace', 1, 4, 1e-6)
    assert np.array_equal(minv, np.full((3, 5), 2.0)) and factor is None and dense_rows is None
    for on_device in (False, True):
        minv, factor, dense_rows, _ = B.resolve_mass(popn, 'x', 'laplace_dense', 1, 4, 1e-6, factor_on_device=on_device)
        assert minv is None and factor is W and dense_rows is rows
    assert calls == [('minv', 'x', 1, 4, 1e-6), ('host', 'x', 1, 4, 1e-6), ('device', 'x', 1, 4, 1e-6)]


# ---- the guarded line-search step (csrc/pglm_linesearch.h: pgl_ls_guarded_step) -----------------------------------
REACH = ('converged', 'warning: take the trial', 'warning: take the best step', 'warning: fail',
         'cut off by max_trials as the trial became the best step', 'non-finite f', 'non-finite dphi')


@pytest.mark.parametrize('constants', [0, 1], ids=['newton-cg/newton', 'bfgs'])
def test_guarded_step_direct_and_wrappers_agree(constants, tmp_path):
    """Scripted searches on a quartic and on a function with a kink (tests/csrc/ls_guarded_host.c, built by gcc): on every
    call the direct pgl_ls_guarded_step, the Newton-CG wrapper and the dense Newton wrapper agree on the decision, on the
    step length and value of the point taken and on all 18 doubles of the line-search state; every way a search can end
    is reached, and each search ends the way its script says."""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / 'ls_guarded_host.so')
    subprocess.check_call(['gcc', '-O2', '-Wall', '-Wextra', '-Werror', '-shared', '-fPIC', '-o', so,
                           os.path.join(root, 'tests', 'csrc', 'ls_guarded_host.c'), '-lm'])
    lib = ctypes.CDLL(so)
    assert lib.lsg_nreach() == len(REACH)
    reached = (ctypes.c_int * len(REACH))()
    rc = lib.lsg_run(constants, reached)
    assert rc == 0, "case %d: check %d failed" % (rc // 100 - 1, rc % 100)
    missing = [name for name, n in zip(REACH, reached) if n == 0]
    assert not missing, missing
    assert sum(reached) == lib.lsg_ncases()
