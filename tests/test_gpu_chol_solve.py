"""GPU tests of the batched solve against the equilibrated Cholesky factor (pgl_chol_solve_dev / DeviceGlm.chol_solve:
k_chol_solve in csrc/pglm_chol.hip.h) over the shapes where its blocking can break: P below, at and above the 32-column
block, one and several blocks, a partial last block (P = 33, 65, 129, 161), one matrix and several, ld = P and ld = P + 3
with NaN in the strict upper triangle and the padding.  Matrices: tests/chol_cases.spd_stack (entries over 24 orders of
magnitude), factored by pgl_chol_factor_dev.  No data set is needed; the handle supplies the stream only.

Bound: the componentwise backward error  max_i |A x - b|_i / (|A| |x| + |b|)_i, the product in np.longdouble, at most 4 x the
same quantity of the host solve of the same case (laplace.numpy_factor + two scipy.linalg.solve_triangular calls), or
P 2^-53 where that is larger: blocked and unblocked substitution share the order of the bound in P, not its constant.  The host
figure is computed here, not stored."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

from tests import chol_cases as CC
from tests import helpers as H
from theano_pyglm_amd.inference.laplace import numpy_factor

pytestmark = pytest.mark.gpu

PS = [1, 2, 31, 32, 33, 64, 65, 129, 161]
PADS = [0, 3]


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)
    yield h
    h.close()


def _padded(A, pad):
    M, P = A.shape[0], A.shape[1]
    out = np.full((M, P, P + pad), np.nan)
    il = np.tril_indices(P)
    out[:, il[0], il[1]] = A[:, il[0], il[1]]
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _solve(h, Ap, b, alias=False):
    """factor + solve on the device -> (x, info) as numpy arrays"""
    import torch
    dev = torch.device('cuda', 0)
    Ad = torch.tensor(Ap, dtype=torch.float64, device=dev)
    bd = torch.tensor(b, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    scale, _, info = h.chol_factor(Ad)
    xd = h.chol_solve(Ad, scale, info, bd, out=bd if alias else None)
    h.sync()
    assert alias == (xd.data_ptr() == bd.data_ptr())
    if not alias:
        assert np.array_equal(bd.cpu().numpy(), b)             # b is read only
    return xd.cpu().numpy(), info.cpu().numpy()


def _case(P):
    A = CC.spd_stack(3, P, 7000 + P)
    rng = np.random.default_rng(100 + P)
    b = rng.standard_normal((3, P)) * np.sqrt(np.diagonal(A, axis1=1, axis2=2))
    return A, b


_RUNS = {}


def _run(h, P, M, pad):
    """one device run per case, shared by the tests: the last M matrices of the stack of 3"""
    if (P, M, pad) not in _RUNS:
        A, b = _case(P)
        _RUNS[(P, M, pad)] = _solve(h, _padded(A[3 - M:], pad), b[3 - M:])
    return _RUNS[(P, M, pad)]


def backward_error(A, x, b):
    Al, xl, bl = A.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    return float(np.max(np.abs(Al.dot(xl) - bl) / (np.abs(Al).dot(np.abs(xl)) + np.abs(bl))))


def host_solve(A, b):
    F, scale, _, info = numpy_factor(A[None])
    assert info[0] == 0
    Ls = np.tril(F[0])
    y = solve_triangular(Ls, b / scale[0], lower=True)
    return solve_triangular(Ls, y, lower=True, trans='T') / scale[0]


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('P', PS)
def test_componentwise_backward_error(handle, P, M, pad):
    A, b = _case(P)
    x, info = _run(handle, P, M, pad)
    assert np.all(info == 0) and np.all(np.isfinite(x))
    for m in range(M):
        Am, bm = A[3 - M + m], b[3 - M + m]
        e_dev = backward_error(Am, x[m], bm)
        e_host = backward_error(Am, host_solve(Am, bm), bm)
        bound = max(4.0 * e_host, P * 2.0 ** -53)
        print("P = %d M = %d ld = P + %d row %d: backward error %.3e, host %.3e, bound %.3e" % (P, M, pad, m, e_dev, e_host, bound))
        assert e_dev <= bound


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('P', PS)
def test_same_bits_alone_in_a_batch_again_and_in_place(handle, P, pad):
    A, b = _case(P)
    x3, _ = _run(handle, P, 3, pad)
    x1, _ = _run(handle, P, 1, pad)
    assert _same_bits(x3[2], x1[0])                            # M = 1 against the same row inside M = 3
    again, _ = _solve(handle, _padded(A, pad), b)
    assert _same_bits(again, x3)                               # two runs
    inplace, _ = _solve(handle, _padded(A, pad), b, alias=True)
    assert _same_bits(inplace, x3)                             # d_x == d_b


def test_failed_rows_are_nan_and_leave_the_others_alone(handle):
    """An indefinite matrix (chol_cases.flip_eigenvalue) between two good ones: its row of x is NaN, the neighbours' bits are
    those of a batch without it."""
    P = 70
    A, b = CC.spd_stack(3, P, 31337), np.random.default_rng(3).standard_normal((3, P))
    good, _ = _solve(handle, _padded(A, 3), b)
    bad = A.copy()
    bad[1] = CC.flip_eigenvalue(A[1], which=P // 2)
    x, info = _solve(handle, _padded(bad, 3), b)
    assert info[0] == 0 and info[2] == 0 and info[1] != 0
    assert np.all(np.isnan(x[1]))
    assert _same_bits(x[0], good[0]) and _same_bits(x[2], good[2])
    xa, _ = _solve(handle, _padded(bad, 3), b, alias=True)
    assert np.all(np.isnan(xa[1])) and _same_bits(xa[0], good[0]) and _same_bits(xa[2], good[2])


def test_argument_checks(handle):
    import ctypes as C
    import torch
    p = C.c_void_p(torch.zeros(64, dtype=torch.float64, device='cuda:0').data_ptr())
    for M, P, ld in ((0, 4, 4), (2, 0, 4), (2, 4, 3)):
        assert handle.lib.pgl_chol_solve_dev(handle.h, p, M, P, ld, p, p, p, p) == -1
    assert handle.lib.pgl_chol_solve_dev(handle.h, p, 2, 4, 4, p, p, None, p) == -1
    A = torch.zeros((2, 4, 4), dtype=torch.float64, device='cuda:0')
    s = torch.ones((2, 4), dtype=torch.float64, device='cuda:0')
    i = torch.zeros(2, dtype=torch.int32, device='cuda:0')
    with pytest.raises(ValueError):
        handle.chol_solve(A, s, i, torch.zeros((2, 3), dtype=torch.float64, device='cuda:0'))
    with pytest.raises(ValueError):
        handle.chol_solve(A, s, i.to(torch.int64), s.clone())
