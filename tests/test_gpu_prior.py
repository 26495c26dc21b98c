"""GPU test of the field order of pgl_prior on its way to the row kernels.  Every lock-step entry point turns its
`const pgl_prior*` into the kernels' argument struct in one function (fill_prior, csrc/pglm_capi.hip), and the ctypes
binding lays the struct out as _lib.Prior; the priors the sampler tests use have sg_b == stim_sigma and mu == lam == 0, so
two swapped doubles would pass them.  Here pgl_bfgs_objective_dev runs with six different doubles, none of them 0 or 1,
against the numpy form of the same prior (bias.py:33, bkgd.py:76, priors.py:139 / 202 as components/priors.py states them).

Tolerance 1e-12 relative, entry by entry: every value is a sum of fewer than twenty f64 terms (rounding <= 20 x 2^-53 =
2.2e-15 of the largest term), the inputs are seeded so that no entry is below a tenth of its largest term (asserted: no
cancellation eats the margin), and a swapped pair of fields moves an entry by order one."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N, B, DS, L = 3, 2, 2, 4
P = 1 + DS + N * B
DOUBLES = (0.7, 1.3, 0.45, -0.2, 2.1, 0.35)                  # mu_b, sg_b, stim_sigma, mu, sigma, lam
TOL = 1e-12


def reference(kind, X, ll, grad):
    """f = -(ll + log prior), g = -(grad + grad log prior) of the rows X, and the larger of the two terms of every entry."""
    mu_b, sg_b, stim_sigma, mu, sigma, lam = DOUBLES
    lp = -0.5 / sg_b ** 2 * (X[:, 0] - mu_b) ** 2 - 0.5 / stim_sigma ** 2 * np.sum(X[:, 1:1 + DS] ** 2, axis=1)
    glp = np.zeros_like(X)
    glp[:, 0] = -(X[:, 0] - mu_b) / sg_b ** 2
    glp[:, 1:1 + DS] = -X[:, 1:1 + DS] / stim_sigma ** 2
    W = X[:, 1 + DS:].reshape(L, N, B)
    if kind == 0:
        lp += -0.5 / sigma ** 2 * np.sum((W - mu) ** 2, axis=(1, 2))
        gw = -(W - mu) / sigma ** 2
    else:
        z = (W - mu) / sigma
        nrm = np.sqrt(np.sum(z * z, axis=2, keepdims=True))
        lp += -lam * np.sum(nrm, axis=(1, 2))
        gw = -lam * z / nrm / sigma
    glp[:, 1 + DS:] = gw.reshape(L, N * B)
    return -(ll + lp), -(grad + glp), np.maximum(np.abs(ll), np.abs(lp)), np.maximum(np.abs(grad), np.abs(glp))


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(N, 200, H.std_ibasis()[:, :B], Dstim=DS, seed=5).device(0)
    yield h
    h.close()


@pytest.mark.parametrize('kind', [0, 1])
def test_objective_reads_every_prior_field_in_its_place(handle, kind):
    import torch
    from theano_pyglm_amd import _lib
    assert len(set(DOUBLES)) == 6 and not set(DOUBLES) & {0.0, 1.0}
    rng = np.random.default_rng(77)
    X = rng.standard_normal((L, P))
    ll = rng.standard_normal(L)
    grad = rng.standard_normal((L, P))
    f0, g0, fs, gs = reference(kind, X, ll, grad)
    assert np.min(np.abs(f0) / fs) > 0.1 and np.min(np.abs(g0) / gs) > 0.1
    dev = torch.device('cuda', 0)
    Xd = torch.tensor(X, dtype=torch.float64, device=dev)
    fd = torch.tensor(ll, dtype=torch.float64, device=dev)
    gd = torch.tensor(grad, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    handle.bfgs_objective_dev(L, P, Xd.data_ptr(), fd.data_ptr(), gd.data_ptr(), (kind,) + DOUBLES)
    handle.sync()
    f, g = fd.cpu().numpy(), gd.cpu().numpy()
    print("kind %d: max |f - f0| / |f0| = %.3e, max |g - g0| / |g0| = %.3e"
          % (kind, np.max(np.abs(f - f0) / np.abs(f0)), np.max(np.abs(g - g0) / np.abs(g0))))
    assert np.all(np.abs(f - f0) <= TOL * np.abs(f0))
    assert np.all(np.abs(g - g0) <= TOL * np.abs(g0))
    # the same prior as a Prior struct: the same bits
    fd.copy_(torch.tensor(ll, dtype=torch.float64, device=dev))
    gd.copy_(torch.tensor(grad, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    handle.bfgs_objective_dev(L, P, Xd.data_ptr(), fd.data_ptr(), gd.data_ptr(), _lib.as_prior((kind,) + DOUBLES))
    handle.sync()
    assert np.array_equal(fd.cpu().numpy(), f) and np.array_equal(gd.cpu().numpy(), g)


# ---- the shapes where the loops of the objective stride, and the NaN rules ------------------------------------------------
N2, B2, DS2, L2 = 3, 8, 300, 5                                # B = PGL_MAXB (the widest basis of the row kernels), Dstim > 256
P2 = 1 + DS2 + N2 * B2                                        # 325 > 256: the row loops take a second trip


@pytest.fixture(scope='module')
def wide_handle():
    ib = H.std_ibasis()
    ib = np.concatenate((ib, np.roll(ib, 17, axis=0)), axis=1)[:, :B2]
    assert ib.shape[1] == B2
    h = H.Problem(N2, 200, ib, Dstim=DS2, seed=6).device(0)
    yield h
    h.close()


def reference_wide(kind, X, ll, grad):
    """f, g of the rows X in longdouble with fit_glm's NaN rules, and the rounding bound of every entry: 8 n 2^-53 m with n
    the terms of the longest chain (f: the P prior terms and ll; g: the B squares under the root and a handful more) and m
    the sum of the absolute values of the terms"""
    LD = np.longdouble
    mu_b, sg_b, stim_sigma, mu, sigma, lam = [LD(v) for v in DOUBLES]
    X, grad, ll = X.astype(LD), grad.astype(LD), ll.astype(LD)
    lpt = np.zeros(X.shape, dtype=LD)                         # the prior terms of f, one per parameter (lasso: per group)
    glp = np.zeros(X.shape, dtype=LD)
    lpt[:, 0] = -0.5 / sg_b ** 2 * (X[:, 0] - mu_b) ** 2
    glp[:, 0] = -(X[:, 0] - mu_b) / sg_b ** 2
    lpt[:, 1:1 + DS2] = -0.5 / stim_sigma ** 2 * X[:, 1:1 + DS2] ** 2
    glp[:, 1:1 + DS2] = -X[:, 1:1 + DS2] / stim_sigma ** 2
    W = X[:, 1 + DS2:].reshape(-1, N2, B2)
    with np.errstate(all='ignore'):
        if kind == 0:
            lpt[:, 1 + DS2:] = (-0.5 / sigma ** 2 * (W - mu) ** 2).reshape(len(X), -1)
            gw = -(W - mu) / sigma ** 2
        else:
            z = (W - mu) / sigma
            nrm = np.sqrt(np.sum(z * z, axis=2, keepdims=True))
            lpt[:, 1 + DS2::B2] = -lam * nrm[:, :, 0]
            gw = -lam * z / nrm / sigma                       # 0 / 0 in a zero group: NaN, and the row is zeroed
    glp[:, 1 + DS2:] = gw.reshape(len(X), -1)
    f = -(ll + np.sum(lpt, axis=1))
    g = -(grad + glp)
    ftol = 8 * (P2 + 4) * 2.0 ** -53 * (np.abs(ll) + np.sum(np.abs(lpt), axis=1))
    gtol = 8 * (B2 + 8) * 2.0 ** -53 * (np.abs(grad) + np.abs(glp))
    badrow = np.any(np.isnan(g), axis=1)
    g[badrow], gtol[badrow] = 0.0, 0.0
    nanf = np.isnan(f)
    f[nanf], ftol[nanf] = 1e16, 0.0
    return f.astype(np.float64), g.astype(np.float64), ftol.astype(np.float64), gtol.astype(np.float64)


@pytest.mark.parametrize('kind', [0, 1])
def test_objective_at_striding_shapes_and_nan_rules(wide_handle, kind):
    """Rows 0 and 1 are ordinary; row 2 has a NaN ll (f = 1e16, the gradient as usual); row 3 a NaN in one gradient entry
    beyond column 256 (a zero row, f as usual); row 4 one impulse group exactly at mu, so that the lasso's gradient is 0 / 0
    there (kind 1: a zero row and a finite f; kind 0: an ordinary row)."""
    import torch
    rng = np.random.default_rng(78)
    X = rng.standard_normal((L2, P2))
    ll = rng.standard_normal(L2)
    grad = rng.standard_normal((L2, P2))
    ll[2] = np.nan
    grad[3, 300] = np.nan
    X[4, 1 + DS2 + B2:1 + DS2 + 2 * B2] = DOUBLES[3]
    f0, g0, ftol, gtol = reference_wide(kind, X, ll, grad)
    assert f0[2] == 1e16 and np.any(g0[2] != 0) and not g0[3].any() and np.isfinite(f0).all() and np.isfinite(g0).all()
    assert (not g0[4].any()) == (kind == 1) and g0[0].all() and g0[1].all()
    dev = torch.device('cuda', 0)
    Xd = torch.tensor(X, dtype=torch.float64, device=dev)
    fd = torch.tensor(ll, dtype=torch.float64, device=dev)
    gd = torch.tensor(grad, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    wide_handle.bfgs_objective_dev(L2, P2, Xd.data_ptr(), fd.data_ptr(), gd.data_ptr(), (kind,) + DOUBLES)
    wide_handle.sync()
    f, g = fd.cpu().numpy(), gd.cpu().numpy()
    with np.errstate(all='ignore'):
        print("kind %d wide: worst fraction of the rounding bound: f %.3g, g %.3g"
              % (kind, np.nanmax(np.abs(f - f0)[ftol > 0] / ftol[ftol > 0]), np.nanmax(np.abs(g - g0)[gtol > 0] / gtol[gtol > 0])))
    assert np.all(np.abs(f - f0) <= ftol) and np.all(np.abs(g - g0) <= gtol)
    assert f[2] == 1e16 and not g[3].any() and ((not g[4].any()) == (kind == 1))
