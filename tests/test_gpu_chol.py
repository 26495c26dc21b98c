"""GPU sweep of the batched equilibrated Cholesky factorisation and the triangular inverse (pgl_chol_factor_dev,
pgl_tri_inverse_dev: csrc/pglm_chol.hip.h) over the shapes where the tiling can break: P below, at and above the 32-column
block and the 64-row trailing tile, one and several blocks, the 128-row panel chunk (P = 161, 200), C3's P = 641, the
stress shape P = 1221, and more matrices than compute units.  Inputs: tests/chol_cases.py (entries spread over 24 orders of
magnitude), ld = P + 3 with NaN in the strict upper triangle and the padding columns.

Bounds (derived, not measured on the device):
  factor   |A - (D^1/2 Ls)(D^1/2 Ls)^T|_ij <= (P + 8) 2^-52 sqrt(A_ii A_jj), the product in np.longdouble: Higham's componentwise
           bound gamma_{P+1} |L||L^T| with (|L||L^T|)_ij <= sqrt(a_ii a_jj), six roundings for the scaling, a factor of two.
  logdet   against 2 sum log diag chol(C) + sum log A_ii with numpy's factor of the same C; tolerance = 4 x the gap between
           that value and np.linalg.slogdet(A) on the same matrix (another summation order), floored at
           1e-12 max(1, |logdet|), both computed by the test (slogdet's LU depends on the BLAS at hand).  Gaps measured on
           the CPU on these inputs: <= 2.3e-15 (P = 1, 2, 5), <= 1.5e-13 (P = 31 .. 33), <= 1.8e-13 (P = 64, 65), 3.5e-13
           (P = 161), 2.1e-12 (P = 200), 4.6e-12 .. 1.1e-11 (P = 641), 0 .. 1.8e-12 (P = 1221), with |logdet| from 1 (P = 2)
           through 4 208 (P = 641) to 9 403 (P = 1221): the floor decides everywhere.
  inverse  max_{i >= j} |Ls X - I|_ij / (|Ls||X|)_ij at most 8 x that of a float64 forward substitution of the same Ls
           computed here (the margin covers the blocked order); np.linalg.solve is no reference, its LU misses the
           componentwise bound on these matrices.
Both residuals cover every entry of the lower triangle at every shape; the extended-precision products are
chol_cases.lower_product_ld's (error-free float64 slices added in np.longdouble: an np.longdouble matrix product itself takes
8 s at P = 1221).  numpy's own factor sits at 0.002 (P = 1221) to 0.13 (P = 2) of the factor bound on these inputs."""
import numpy as np
import pytest

from tests import chol_cases as CC
from tests import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (2, 3), (31, 3), (32, 3), (33, 3), (64, 3), (65, 3), (161, 3), (200, 3), (641, 2), (1221, 1), (5, 300)]
PAD = 3


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)
    yield h
    h.close()


def _padded(A):
    """(M, P, P + 3): the lower triangle of A, NaN above the diagonal and in the padding columns."""
    M, P = A.shape[0], A.shape[1]
    out = np.full((M, P, P + PAD), np.nan)
    il = np.tril_indices(P)
    out[:, il[0], il[1]] = A[:, il[0], il[1]]
    return out


def _factor(h, Ap, inverse=False):
    """-> (lower triangle in place, scale, logdet, info) as numpy arrays; with inverse, the inverse ran behind the factor."""
    import torch
    dev = torch.device('cuda', 0)
    Ad = torch.tensor(Ap, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    scale, logdet, info = h.chol_factor(Ad)
    if inverse:
        h.tri_inverse(Ad, info)
    h.sync()
    return Ad.cpu().numpy(), scale.cpu().numpy(), logdet.cpu().numpy(), info.cpu().numpy()


_RUNS = {}


def _runs(h, P, M):
    """One device factorisation and one factor + inverse per shape, shared by the tests of that shape."""
    if (P, M) not in _RUNS:
        A = CC.spd_stack(M, P, 9000 + P)
        Ap = _padded(A)
        _RUNS[(P, M)] = (A, Ap, _factor(h, Ap), _factor(h, Ap, inverse=True))
    return _RUNS[(P, M)]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize('P,M', SHAPES)
def test_factor_logdet_and_layout(handle, P, M):
    A, Ap, (F, scale, logdet, info), _ = _runs(handle, P, M)
    assert np.all(info == 0)
    il = np.tril_indices(P)
    mask = np.ones((P, P + PAD), dtype=bool)
    mask[il] = False
    assert _same_bits(F[:, mask], Ap[:, mask])                 # strict upper triangle and padding: the input's bits
    for m in range(min(M, 3)):
        assert np.all(np.abs(scale[m] - np.sqrt(np.diag(A[m]))) <= 2.0 ** -52 * scale[m])
        Ls = np.tril(F[m][:, :P])
        res = CC.factor_residual(A[m], Ls, scale[m])
        bound = (P + 8) * 2.0 ** -52
        C, _ = CC.equilibrated(A[m])
        res_np = CC.factor_residual(A[m], np.linalg.cholesky(C), scale[m]) if P <= 256 else np.nan   # (printed only)
        want = 2.0 * np.sum(np.log(np.diag(np.linalg.cholesky(C)))) + np.sum(np.log(np.diag(A[m])))
        gap = abs(want - np.linalg.slogdet(A[m])[1])
        tol = max(4.0 * gap, 1e-12 * max(1.0, abs(want)))
        print("P = %d row %d: factor residual %.3e (numpy %.3e) of bound %.3e; logdet %.6f off by %.2e, gap %.2e tol %.2e"
              % (P, m, res, res_np, bound, logdet[m], abs(logdet[m] - want), gap, tol))
        assert res <= bound
        assert abs(logdet[m] - want) <= tol
    if M > 3:                                                  # every row of the wide batch against its residual bound
        for m in range(M):
            assert CC.factor_residual(A[m], np.tril(F[m][:, :P]), scale[m]) <= (P + 8) * 2.0 ** -52


@pytest.mark.parametrize('P,M', SHAPES)
def test_inverse_residual_and_layout(handle, P, M):
    A, Ap, (F, _, _, _), (X, _, _, info) = _runs(handle, P, M)
    assert np.all(info == 0)
    il = np.tril_indices(P)
    mask = np.ones((P, P + PAD), dtype=bool)
    mask[il] = False
    assert _same_bits(X[:, mask], Ap[:, mask])
    for m in (range(M) if M <= 3 else (0, 1, 2, 255, 256, 257, M - 1)):      # (M = 300: rows past the compute units too)
        Ls = np.tril(F[m][:, :P])
        r_dev = CC.inverse_residual(Ls, np.tril(X[m][:, :P]))
        r_ref = CC.inverse_residual(Ls, CC.substitution_inverse(Ls))
        print("P = %d row %d: inverse residual %.3e, substitution %.3e" % (P, m, r_dev, r_ref))
        assert r_dev <= 8.0 * r_ref


@pytest.mark.parametrize('P,M', [(33, 3), (161, 3), (641, 2), (5, 300)])
def test_repeat_and_subset_give_the_same_bits(handle, P, M):
    A, Ap, first, firstinv = _runs(handle, P, M)
    again = _factor(handle, Ap)
    againinv = _factor(handle, Ap, inverse=True)
    for a, b in zip(first + firstinv, again + againinv):
        assert _same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)
    m = M - 1
    solo = _factor(handle, Ap[m:m + 1])
    soloinv = _factor(handle, Ap[m:m + 1], inverse=True)
    for a, b in zip(first + firstinv, solo + soloinv):
        assert _same_bits(a[m], b[0]) if a.dtype == np.float64 else a[m] == b[0]


def test_bad_rows_are_flagged_and_leave_the_others_alone(handle):
    """An indefinite matrix (one eigenvalue flipped) and one with a NaN entry in a batch of 4: ordinary inputs, the kernels
    run to their end, flag the rows and fill them with NaN."""
    P = 70
    A = CC.spd_stack(2, P, 31337)
    indef = CC.flip_eigenvalue(A[0], which=P // 2)
    k_fail = CC.first_failing_column(CC.equilibrated(indef)[0] if np.all(np.diag(indef) > 0) else indef)
    assert k_fail is not None
    nan = A[1].copy()
    nan[40, 9] = nan[9, 40] = np.nan
    batch = _padded(np.stack([A[0], indef, A[1], nan]))
    F, scale, logdet, info = _factor(handle, batch)
    X, _, _, info2 = _factor(handle, batch, inverse=True)
    print("indefinite row: info %d (numpy stops at column %d); NaN row: info %d" % (info[1], k_fail, info[3]))
    assert np.array_equal(info, info2)
    assert info[0] == 0 and info[2] == 0 and info[1] == k_fail + 1 and info[3] != 0
    il = np.tril_indices(P)
    for m in (1, 3):
        assert np.all(np.isnan(F[m][il])) and np.all(np.isnan(X[m][il]))
        assert np.all(np.isnan(scale[m])) and np.isnan(logdet[m])
    for m in (0, 2):
        solo = _factor(handle, batch[m:m + 1])
        soloinv = _factor(handle, batch[m:m + 1], inverse=True)
        assert _same_bits(F[m], solo[0][0]) and _same_bits(scale[m], solo[1][0]) and _same_bits(logdet[m], solo[2][0])
        assert _same_bits(X[m], soloinv[0][0])


def test_argument_checks(handle):
    import torch
    from theano_pyglm_amd._lib import PglError
    A = torch.zeros((2, 4, 3), dtype=torch.float64, device='cuda:0')
    with pytest.raises(ValueError):
        handle.chol_factor(A)                                  # ld < P
    import ctypes as C
    p = C.c_void_p(torch.zeros(64, dtype=torch.float64, device='cuda:0').data_ptr())
    for M, P, ld in ((0, 4, 4), (2, 0, 4), (2, 4, 3)):
        assert handle.lib.pgl_chol_factor_dev(handle.h, p, M, P, ld, p, p, p) == -1
        assert handle.lib.pgl_tri_inverse_dev(handle.h, p, M, P, ld, p) == -1
    with pytest.raises(PglError):
        from theano_pyglm_amd._lib import _chk
        _chk(handle.lib.pgl_chol_factor_dev(handle.h, p, 0, 4, 4, p, p, p))
