"""Host side of the dense Hessians: the priors' dense Hessian against the columns of hess_log_prior_vec, the Laplace
algebra on hand-made quadratics, the error paths of the public interface, and the dry run of the k_hess dispatch over the
shape grid.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. priors ---------------------------------------------------------------------------------------------------------
def _models():
    from theano_pyglm_amd.models.model_factory import make_model
    gauss = make_model('standard_glm', N=3, dt=0.001)
    gauss['impulse']['prior'] = {'type': 'normal', 'mu': 0.3, 'sigma': 2.0}
    lasso = make_model('standard_glm', N=3, dt=0.001)
    lasso['impulse']['prior'] = {'type': 'group_lasso', 'mu': 0.1, 'sigma': 2.0, 'lam': 1.5}
    basis = make_model('standard_glm', N=3, dt=0.001)
    basis['bkgd'] = {'type': 'basis', 'D_stim': 2, 'dt_max': 0.3, 'basis': basis['bkgd']['basis']}
    basis['impulse']['prior'] = {'type': 'normal', 'mu': 0.0, 'sigma': 1.0}
    return [gauss, lasso, basis]


@pytest.mark.parametrize('k', [0, 1, 2], ids=['gaussian', 'group_lasso', 'basis_stimulus'])
def test_hess_log_prior_is_the_matrix_of_hess_log_prior_vec_columns(k):
    from theano_pyglm_amd.components.priors import Gaussian, GroupLasso
    from theano_pyglm_amd.population import Population
    from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars
    popn = Population(_models()[k])
    glm, syms = popn.glm, popn.glm_syms()
    assert isinstance(glm.imp_model.prior, GroupLasso if k == 1 else Gaussian)
    xn = popn.sample(np.random.RandomState(4))['glms'][1]
    xn['imp']['w_ir'] = 0.5 + np.random.default_rng(6).standard_normal(np.size(xn['imp']['w_ir']))   # away from a zero group
    w0, shapes = packdict(get_vars(syms, xn))
    Hp = glm.hess_log_prior(xn)
    assert Hp.shape == (w0.size, w0.size)
    cols = np.stack([packdict(get_vars(syms, glm.hess_log_prior_vec(xn, unpackdict(e, shapes))))[0] for e in np.eye(w0.size)],
                    axis=1)
    assert np.array_equal(Hp, cols)
    assert np.allclose(Hp, Hp.T, rtol=1e-13, atol=0.0)
    if k == 1:
        assert np.count_nonzero(Hp - np.diag(np.diag(Hp))) > 0      # the group blocks are not diagonal


# ---- 2. the Laplace algebra --------------------------------------------------------------------------------------------
def test_laplace_of_a_gaussian_is_exact():
    """log p(theta) = c - 1/2 (theta - m)^T A (theta - m): Z = e^c (2 pi)^(P/2) det(A)^(-1/2), covariance A^-1."""
    from theano_pyglm_amd.inference.laplace import laplace_from_hessian
    rng = np.random.default_rng(3)
    P = 7
    M = rng.standard_normal((P, P))
    A = M.dot(M.T) + P * np.eye(P)
    c = -12.5
    r = laplace_from_hessian(A, c)
    assert r['pd'] is True
    assert np.allclose(r['cov'], np.linalg.inv(A), rtol=1e-12, atol=1e-14)
    assert np.allclose(r['stderr_vec'], np.sqrt(np.diag(np.linalg.inv(A))), rtol=1e-12)
    assert np.allclose(r['chol'].dot(r['chol'].T), A, rtol=1e-13)
    want = c + 0.5 * P * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(A)[1]
    assert abs(r['log_evidence'] - want) <= 1e-12 * abs(want)
    # a diagonal case by hand: independent normals of variance 1 / a_i
    a = np.array([0.5, 2.0, 8.0])
    r = laplace_from_hessian(np.diag(a), 0.0)
    assert np.allclose(r['stderr_vec'], 1.0 / np.sqrt(a), rtol=1e-15)
    assert abs(r['log_evidence'] - np.sum(0.5 * np.log(2 * np.pi / a))) <= 1e-14


def test_laplace_of_an_indefinite_matrix_is_nan_not_an_error():
    from theano_pyglm_amd.inference.laplace import laplace_from_hessian
    for A in (np.diag([1.0, -2.0, 3.0]), np.diag([1.0, 0.0]), np.array([[1.0, np.nan], [np.nan, 1.0]])):
        r = laplace_from_hessian(A, 1.0)
        assert r['pd'] is False
        assert np.isnan(r['log_evidence']) and np.all(np.isnan(r['cov'])) and np.all(np.isnan(r['stderr_vec']))
        assert np.all(np.isnan(r['chol']))


# ---- 3. error paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sparse_weighted_model', 'spatiotemporal_glm'])
def test_compute_hessian_of_unserved_packing_raises(name):
    from theano_pyglm_amd.inference.laplace import laplace_glms
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = Population(make_model(name, N=2, dt=0.001))
    x = popn.sample(np.random.RandomState(1))
    with pytest.raises(ValueError, match="Impulses|Stimulus"):
        popn.compute_hessian(x, 0)
    with pytest.raises(ValueError, match="Impulses|Stimulus"):
        popn.compute_hessian_packed(x)
    with pytest.raises(ValueError, match="Impulses|Stimulus"):
        popn.glm.hess_log_prior(x['glms'][0])
    with pytest.raises(ValueError, match="Impulses|Stimulus"):
        laplace_glms(popn, x)


def test_laplace_on_a_time_shard_raises():
    from theano_pyglm_amd.inference.laplace import laplace_glms
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = Population(make_model('standard_glm', N=2, dt=0.001))
    popn.set_time_shard(0, 2)
    with pytest.raises(ValueError, match="time-sharded"):
        laplace_glms(popn, popn.sample(np.random.RandomState(1)))


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------
def test_hess_symbols_and_version():
    import ctypes
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ('pgl_hess_dev', 'pgl_hess'):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert _lib.load().pgl_version() >= 104                  # (103: the version before the dense Hessian)
    for m in ('hess', 'hessian'):
        assert hasattr(_lib.DeviceGlm, m)
    with open(os.path.join(ROOT, 'include', 'pyglm_hip.h')) as f:
        hdr = f.read()
    assert 'int pgl_hess_dev(' in hdr and 'int pgl_hess(' in hdr


def test_every_reachable_hess_kernel_is_built_and_every_built_one_is_reachable():
    """Path 5 of the dry run (the k_hess launches of pgl_hess_dev after a prepare) over the shape grid of
    tools/reachable_kernels.shapes(), dense stimulus columns only: the instantiations it names are exactly the k_hess<
    instantiations in the library, and none of them uses scratch or spills a register."""
    import __graft_entry__ as ge
    ge.build_hip()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_resources as KR
    import reachable_kernels as RK
    from theano_pyglm_amd import _lib
    named = {}
    for N, B, nT, stim, Ds, count in RK.shapes():
        if stim:                                              # (a separable stimulus is unsupported: below)
            continue
        for n in _lib.plan_kernels(N, B=B, R=200, Dstim=Ds, nT=nT, stim=0, count=count, path=5):
            named.setdefault(n, (N, B, nT, Ds, count))
    with pytest.raises(_lib.PglError, match="separable"):
        _lib.plan_kernels(32, Dstim=27, stim=1, path=5)
    built = dict((KR.short(n), r) for n, r in KR.kernel_resources(_lib.LIB_PATH).items() if KR.short(n).startswith('k_hess<'))
    print("named %s; built %s" % (named, built))
    assert named and all(n.startswith('k_hess<') for n in named)
    assert sorted(named) == sorted(built)
    for n, r in built.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0 and r['spill_sgpr'] == 0, (n, r)
    assert len(built) <= 2
