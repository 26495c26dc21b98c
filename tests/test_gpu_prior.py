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
