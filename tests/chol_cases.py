"""Shared inputs and references of the batched Cholesky / triangular inverse tests (test_laplace_device_host.py on the numpy
backend, test_gpu_chol.py on the device): ill-scaled symmetric positive definite matrices, the equilibrated matrix, a
substitution-based float64 inverse, and the extended-precision products the residuals are measured with."""
import numpy as np

U = 2.0 ** -53                                                # unit roundoff of float64


def spd_stack(M, P, seed):
    """(M, P, P): A = (G^T G) o (d d^T), G (2 P, P) standard normal, d = 10^uniform(-6, 6) with both ends present (P >= 2):
    entries spread over 24 orders of magnitude, the equilibrated matrix well conditioned.  Exactly symmetric."""
    rng = np.random.default_rng(seed)
    out = np.empty((M, P, P))
    for m in range(M):
        G = rng.standard_normal((2 * P, P))
        d = 10.0 ** rng.uniform(-6.0, 6.0, P)
        if P >= 2:
            d[rng.permutation(P)[:2]] = (1e-6, 1e6)
        A = G.T.dot(G) * d[:, None] * d[None, :]
        out[m] = np.tril(A) + np.tril(A, -1).T
    return out


def equilibrated(A):
    """(C, s): C = A o (r r^T), r = 1 / s, s = sqrt(diag A) -- laplace_from_hessian's scaling, the same operation order."""
    s = np.sqrt(np.diag(A))
    r = 1.0 / s
    return A * r[:, None] * r[None, :], s


def flip_eigenvalue(A, which=0):
    """A with the sign of one eigenvalue of its equilibrated form flipped: symmetric, indefinite, same scaling."""
    C, s = equilibrated(A)
    w, V = np.linalg.eigh(C)
    w[which] = -w[which]
    B = (V * w).dot(V.T) * s[:, None] * s[None, :]
    return np.tril(B) + np.tril(B, -1).T


def first_failing_column(A):
    """The first column k at which a Cholesky factorisation of A stops (leading minor k + 1 not positive definite)."""
    for k in range(A.shape[0]):
        try:
            np.linalg.cholesky(A[:k + 1, :k + 1])
        except np.linalg.LinAlgError:
            return k
    return None


def substitution_inverse(L):
    """X = L^-1 for lower triangular L by forward substitution in float64, one row at a time:
    X[i, :] = (e_i - L[i, :i] X[:i, :]) / L[i, i]."""
    P = L.shape[0]
    X = np.zeros((P, P))
    for i in range(P):
        row = -L[i, :i].dot(X[:i, :i + 1])
        row[i] += 1.0
        X[i, :i + 1] = row / L[i, i]
    return X


BETA = 20                                                     # bits per slice: P (2^BETA + 1)^2 < 2^53 for P <= 2048
NSLICE = 4


def _slices(M, axis):
    """M = S_0 + .. + S_3 + R exactly: slice s holds, for every row (axis 1) or column (axis 0) of M, the multiples of
    2^(ex - 20 (s + 1)) nearest to what the earlier slices left, 2^ex the power of two above the largest entry of that
    row / column (Ozaki's error-free splitting).  |R| <= 2^(ex - 81).  Returns ([S_s], bound (P,) on |R| per row / column)."""
    mx = np.max(np.abs(M), axis=axis, keepdims=True)
    ex = np.frexp(np.where(mx > 0.0, mx, 1.0))[1].astype(float)          # |M| < 2^ex
    R = np.array(M, dtype=float)
    out = []
    for s in range(NSLICE):
        sigma = 0.75 * np.exp2(ex + 53.0 - BETA * (s + 1))
        S = (R + sigma) - sigma
        out.append(S)
        R = R - S
    return out, np.max(np.abs(R), axis=axis)


def lower_product_ld(L, R, transpose=False, block=256):
    """(prod, err): the lower triangle of L R (R lower triangular) or of L R^T (transpose; R lower triangular as well) for
    lower triangular L in extended precision, the rest 0, and a bound on what prod misses.  An np.longdouble matrix
    product runs unvectorised (8 s at P = 1221), so the operands are split into 20-bit slices (_slices: rows of L, columns
    of the right factor); a float64 product of two slices is exact in any summation order (P terms of 2^40 units stay below
    2^53), runs in the BLAS, and the 16 products are added in np.longdouble.  err_ij bounds the part of the operands that
    four slices do not hold (entries 2^-81 below the largest of their row / column)."""
    P = L.shape[0]
    assert P <= 2048
    Lt, Rt = np.tril(L), np.tril(R)
    if transpose:
        Rt = np.ascontiguousarray(Rt.T)
    Ls, el = _slices(Lt, 1)
    Rs, er = _slices(Rt, 0)
    out = np.zeros((P, P), dtype=np.longdouble)
    for r0 in range(0, P, block):                              # block rows: columns and inner index stop at the row block's end
        r1 = min(P, r0 + block)
        for a in Ls:
            for b in Rs:
                out[r0:r1, :r1] += a[r0:r1, :r1].dot(b[:r1, :r1])
    err = (el[:, None] * np.sum(np.abs(Rt), axis=0)[None, :] + np.sum(np.abs(Lt), axis=1)[:, None] * er[None, :]) * 1.001
    return np.tril(out), np.tril(err)


def factor_residual(A, Ls, s):
    """max over i >= j of |A - (D^1/2 Ls)(D^1/2 Ls)^T|_ij / sqrt(A_ii A_jj), the product in extended precision
    (lower_product_ld; what it may miss is added to the difference)."""
    F = np.tril(Ls) * s[:, None]
    prod, miss = lower_product_ld(F, F, transpose=True)
    d = np.sqrt(np.diag(A)).astype(np.longdouble)
    err = (np.abs(np.tril(A).astype(np.longdouble) - prod) + miss) / (d[:, None] * d[None, :])
    return float(np.max(err))


def inverse_residual(Ls, X):
    """max over i >= j of |Ls X - I|_ij / (|Ls| |X|)_ij, the numerator in extended precision (lower_product_ld; what it may
    miss is added)."""
    P = Ls.shape[0]
    prod, miss = lower_product_ld(Ls, X)
    num = np.abs(prod - np.eye(P, dtype=np.longdouble)) + miss
    den = np.abs(np.tril(Ls)).dot(np.abs(np.tril(X)))
    il = np.tril_indices(P)
    return float(np.max(num[il] / den[il]))
