"""The Laplace algebra of the device route (inference/laplace.py: laplace_from_factor -- one factorisation of the reversed
theta-layout matrix and one triangular inverse) on its numpy backend, against the host route (laplace_from_hessian and
batched_hmc.factor_inverse_mass), and the C symbols of the two kernels.  No GPU needed.

Tolerances: both routes are backward stable factorisations of the same matrix, so they differ by at most
c P u cond(C) relative (C the equilibrated matrix; Higham, Accuracy and Stability, ch. 10 and 14); the bound used is
64 P 2^-53 cond(C), the one of the device end-to-end test, and cond(C) <= 1e3 is asserted on these inputs (the scaling
d d^T alone spreads the entries over 24 orders of magnitude)."""
import ctypes

import numpy as np
import pytest

from tests import chol_cases as CC

SIZES = [1, 2, 33, 161]


def _case(P, M=3):
    A = CC.spd_stack(M, P, 4000 + P)                          # packed order
    pi = np.random.default_rng(5000 + P).permutation(P)        # packed position of every theta column
    return A, pi, A[:, pi[:, None], pi[None, :]]


def _algebra(A_theta, cov=False):
    from theano_pyglm_amd.inference import laplace as LP
    return LP.laplace_from_factor(A_theta, LP.numpy_factor, LP.numpy_inverse, np, cov=cov)


@pytest.mark.parametrize('P', SIZES)
def test_factor_route_agrees_with_the_host_route(P):
    from theano_pyglm_amd.inference.batched_hmc import factor_inverse_mass
    from theano_pyglm_amd.inference.laplace import laplace_from_hessian
    A, pi, A_theta = _case(P)
    res = _algebra(A_theta, cov=True)
    assert np.all(res['info'] == 0) and np.all(res['pd'])
    iu = np.triu_indices(P, 1)
    for m in range(A.shape[0]):
        host = laplace_from_hessian(A[m], 1.25)
        assert host['pd']
        cond = np.linalg.cond(CC.equilibrated(A[m])[0])
        assert cond <= 1e3
        tol = 64.0 * P * CC.U * cond
        W = res['W'][m]
        assert np.all(W[iu] == 0.0) and np.all(np.diag(W) > 0.0)
        cov_theta = host['cov'][np.ix_(pi, pi)]
        Wh = factor_inverse_mass(cov_theta)
        sd = np.sqrt(np.diag(cov_theta))
        errW = np.max(np.abs(W - Wh) / sd[:, None])
        err_sd = np.max(np.abs(res['stderr'][m] - sd) / sd)
        assert np.array_equal(host['stderr_vec'][pi], sd)
        log_ev = 1.25 + 0.5 * P * np.log(2.0 * np.pi) - 0.5 * res['logdet'][m]
        err_ev = abs(log_ev - host['log_evidence'])
        err_cov = np.max(np.abs(res['cov'][m] - cov_theta) / (sd[:, None] * sd[None, :]))
        print("P = %d row %d: cond(C) = %.2e tol = %.2e; W %.2e stderr %.2e log evidence %.2e cov %.2e"
              % (P, m, cond, tol, errW, err_sd, err_ev, err_cov))
        assert errW <= tol and err_sd <= tol and err_ev <= tol and err_cov <= tol


def test_failed_rows_are_nan_and_leave_their_neighbours_alone():
    P = 33
    A, pi, A_theta = _case(P, M=2)
    indef = CC.flip_eigenvalue(A_theta[0])
    nan = A_theta[1].copy()
    nan[20, 7] = nan[7, 20] = np.nan
    zero = A_theta[0].copy()
    zero[11, :] = zero[:, 11] = 0.0
    stack = np.stack([A_theta[0], indef, A_theta[1], nan, zero, A_theta[0]])
    res = _algebra(stack, cov=True)
    assert res['pd'].tolist() == [True, False, True, False, False, True]
    for m in (1, 3, 4):
        assert res['info'][m] != 0
        for key in ('W', 'stderr', 'cov'):
            assert np.all(np.isnan(res[key][m])), (m, key)
        assert np.isnan(res['logdet'][m])
    # the zero diagonal sits at theta column 11: column P - 1 - 11 of the reversed matrix
    assert res['info'][4] == P - 1 - 11 + 1
    for m, solo in ((0, A_theta[0]), (2, A_theta[1]), (5, A_theta[0])):
        one = _algebra(solo[None], cov=True)
        for key in ('W', 'stderr', 'cov', 'logdet'):
            assert np.array_equal(res[key][m], one[key][0]), (m, key)


def test_backend_reads_the_lower_triangle_only():
    from theano_pyglm_amd.inference import laplace as LP
    A = CC.spd_stack(2, 33, 77)
    junk = A.copy()
    iu = np.triu_indices(33, 1)
    junk[:, iu[0], iu[1]] = np.nan
    a = LP.numpy_factor(A.copy())
    b = LP.numpy_factor(junk)
    il = np.tril_indices(33)
    assert np.array_equal(a[0][:, il[0], il[1]], b[0][:, il[0], il[1]])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.all(b[3] == 0)
    assert np.all(np.isnan(b[0][:, iu[0], iu[1]]))            # the strict upper triangle is left as it came


def test_sliced_product_equals_the_longdouble_product():
    """chol_cases.lower_product_ld (what the device sweep measures its residuals with) against a plain np.longdouble
    product: equal to the rounding of the latter's own sums, nothing missed, on an ill-scaled factor."""
    P = 161
    A = CC.spd_stack(1, P, 9000 + P)[0]
    C, s = CC.equilibrated(A)
    L = np.linalg.cholesky(C)
    X = CC.substitution_inverse(L)
    F = L * s[:, None]
    for left, right, tr in ((L, X, False), (F, F, True)):
        prod, miss = CC.lower_product_ld(left, right, transpose=tr)
        rl = right.T if tr else right
        ref = np.tril(left.astype(np.longdouble).dot(rl.astype(np.longdouble)))
        mag = np.abs(left).dot(np.abs(rl))
        assert np.all(np.abs(prod - ref) + miss <= P * 2.0 ** -63 * mag)
        assert np.all(np.triu(prod, 1) == 0)


def test_new_symbols_are_in_the_library_and_check_their_arguments():
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pgl_chol_factor_dev', 'pgl_tri_inverse_dev'):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # no handle, and (checked before the device is touched) bad shapes: PGL_ERR_ARG
    assert lib.pgl_chol_factor_dev(None, p, 1, 2, 2, p, p, p) == -1
    assert lib.pgl_tri_inverse_dev(None, p, 1, 2, 2, p) == -1
    assert hasattr(_lib.DeviceGlm, 'chol_factor') and hasattr(_lib.DeviceGlm, 'tri_inverse')


def test_laplace_glms_keeps_its_host_route_by_default():
    import inspect
    from theano_pyglm_amd.inference.laplace import laplace_glms
    from theano_pyglm_amd.inference.batched_hmc import sample_glms_hmc
    sig = inspect.signature(laplace_glms)
    assert sig.parameters['device'].default is False and sig.parameters['cov'].default is False
    assert inspect.signature(sample_glms_hmc).parameters['factor_on_device'].default is False
