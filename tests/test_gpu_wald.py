"""k_wald_groups through pgl_wald_groups_dev on the synthetic W of tests/wald_cases.json: d_out and d_u equal the gcc mirror
(tests/csrc/wald_host.c) bit for bit -- B in {1, 2, 5, 16}, first in {1, 4}, G in {1, 5, 7} (and 52), P below one lane walk,
ending exactly at first + G B and crossing column 256, ld = P and P + 3 with NaN in the strict upper triangle and the pad, a
row with info != 0, d_u = NULL, determinism, the argument errors.  Then coupling_tests end to end on the small fitted
population of tests/test_gpu_laplace_device.py: the device route against the host route, and lr1 against the host objective
at the same points."""
import copy

import numpy as np
import pytest

from tests import helpers as H
from tests import wald_reference as WR

pytestmark = pytest.mark.gpu
CASES = WR.load()


@pytest.fixture(scope='module')
def handle():
    h = H.Problem(2, 200, H.std_ibasis(), seed=5).device(0)      # (the handle supplies device and stream only)
    yield h
    h.close()


def _dev(d):
    import torch
    return (torch.tensor(d['W'], device='cuda'), torch.tensor(d['theta'], device='cuda'), torch.tensor(d['c'], device='cuda'),
            torch.tensor(d['info'], device='cuda'))


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_kernel_equals_the_mirror_bit_for_bit(handle, case):
    import torch
    d = WR.make_case(case)
    first, G, B, M = case['first'], case['G'], case['B'], case['M']
    W, theta, c, info = _dev(d)
    out_h, u_h = WR.host_wald(d['W'], d['theta'], first, G, B, d['c'], info=d['info'], want_u=True)
    out, u = handle.wald_groups(W, theta, first, G, B, c, info, u=True)
    out2 = handle.wald_groups(W, theta, first, G, B, c, info)                   # d_u = NULL
    outb, ub = handle.wald_groups(W, theta, first, G, B, c, info, u=True)       # a second call
    handle.sync()
    torch.cuda.synchronize()
    out, u, out2, outb, ub = (t.cpu().numpy() for t in (out, u, out2, outb, ub))
    assert WR.same_bits(out, out_h) and WR.same_bits(u, u_h)
    assert WR.same_bits(out2, out_h)
    assert WR.same_bits(outb, out) and WR.same_bits(ub, u)
    # the host-pointer form
    oh, uh = handle.wald_groups_host(d['W'], d['theta'], first, G, B, d['c'], d['info'], u=True)
    assert WR.same_bits(oh, out_h) and WR.same_bits(uh, u_h)
    # a row with info != 0: NaN; the others have the bits of the call without it
    bad = np.nonzero(d['info'])[0]
    if bad.size:
        assert np.all(np.isnan(out[bad])) and np.all(np.isnan(u.reshape(G, M, -1)[:, bad]))
        zero = torch.zeros_like(info)
        torch.cuda.synchronize()                                                   # (filled on torch's stream, read on the handle's)
        ok = handle.wald_groups(W, theta, first, G, B, c, zero)
        handle.sync()                                                              # (the handle's stream is not torch's)
        ok = ok.cpu().numpy()
        keep = np.nonzero(d['info'] == 0)[0]
        assert WR.same_bits(ok[keep], out[keep]) and np.all(np.isfinite(ok[bad][..., 3]))
    # a group alone or among others
    for g in sorted(set([0, G // 2, G - 1])):
        o1, u1 = handle.wald_groups(W, theta, first + g * B, 1, B, c, info, u=True)
        handle.sync()
        assert WR.same_bits(o1.cpu().numpy()[:, 0], out[:, g]) and WR.same_bits(u1.cpu().numpy(), u[g * M:(g + 1) * M])


def test_argument_errors(handle):
    import torch
    from theano_pyglm_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    inf = torch.zeros(8, dtype=torch.int32, device='cuda')
    p, q = buf.data_ptr(), inf.data_ptr()
    ok = dict(W=p, M=2, P=11, ld=11, theta=p, first=1, G=2, B=5, c=p, info=q, out=p + 8 * 2048, u=None)
    order = ('W', 'M', 'P', 'ld', 'theta', 'first', 'G', 'B', 'c', 'info', 'out', 'u')

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.pgl_wald_groups_dev(handle.h, *[a[k] for k in order])

    assert call() == 0
    for kw in (dict(M=0), dict(G=0), dict(B=0), dict(ld=10), dict(first=-1), dict(G=3), dict(first=2), dict(W=None),
               dict(theta=None), dict(c=None), dict(info=None), dict(out=None)):
        assert call(**kw) == -1, kw                                                # PGL_ERR_ARG
    assert call(B=17, P=40, ld=40, G=1) == -4                                      # PGL_ERR_UNSUPPORTED
    assert lib.pgl_wald_groups_dev(None, *[ok[k] for k in order]) == -1
    with pytest.raises(_lib.PglError, match="PGL_WALD_MAX_B"):
        handle.wald_groups_dev(p, 1, 40, 40, p, 1, 1, 17, p, q, p)
    handle.sync()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fitted():
    from tests.test_gpu_laplace_device import _population
    from tests import chol_cases as CC
    from theano_pyglm_amd.inference.coord_descent import coord_descent
    from theano_pyglm_amd.inference.laplace import laplace_glms
    popn = _population()
    x = coord_descent(popn, x0=popn.sample(np.random.RandomState(103)), maxiter=1)
    host = laplace_glms(popn, x)
    tol = []
    for r in host:
        cond = np.linalg.cond(CC.equilibrated(r['A'])[0])
        assert r['pd'] and cond <= 1e8
        tol.append(64.0 * r['A'].shape[0] * CC.U * cond)
    yield popn, x, host, np.array(tol)
    popn.release_data()


def test_coupling_tests_device_against_host(fitted):
    """The tolerance of tests/test_gpu_laplace_device.py on the standard errors, 64 P u cond(C), applied to T scaled by
    kappa_2(S), S the group's block of the host covariance."""
    from theano_pyglm_amd.inference.connectivity import coupling_tests
    from theano_pyglm_amd.inference.laplace import theta_positions
    popn, x, host, tol = fitted
    N, B = popn.N, popn.glm.imp_model.B
    dev = coupling_tests(popn, x, alpha=0.05)
    ref = coupling_tests(popn, x, alpha=0.05, device=False)
    pi, _ = theta_positions(popn, x, 0)
    assert dev['wald'].shape == (N, N) and dev['dof'] == B and np.all(dev['pd']) and np.all(ref['pd'])
    assert np.all(dev['group_info'] == 0) and np.all(np.isfinite(dev['wald'])) and np.all(dev['wald'] >= 0.0)
    for m in range(N):
        cov = host[m]['cov'][np.ix_(pi, pi)]
        for g in range(N):
            o = 1 + popn.glm.Dstim + g * B
            kappa = np.linalg.cond(cov[o:o + B, o:o + B])
            eT = abs(dev['wald'][m, g] - ref['wald'][m, g])
            bound = tol[m] * kappa * abs(ref['wald'][m, g])
            print("post %d pre %d: T %.6g, |dT| %.2e, bound %.2e (kappa %.2e)" % (m, g, ref['wald'][m, g], eT, bound, kappa))
            assert eT <= bound
            assert abs(dev['weight'][m, g] - ref['weight'][m, g]) <= 1e-12 * max(1.0, abs(ref['weight'][m, g]))
            # (|d c^T S c| <= tol (sum |c_a| sqrt(S_aa))^2 <= tol B lambda_max |c|^2 and c^T S c >= lambda_min |c|^2; the root halves it)
            assert abs(dev['weight_se'][m, g] - ref['weight_se'][m, g]) <= 0.5 * B * tol[m] * kappa * ref['weight_se'][m, g]
    diag = np.eye(N, dtype=bool)
    assert np.all(np.isnan(dev['q_value'][diag])) and np.all(np.isfinite(dev['q_value'][~diag]))
    assert np.allclose(dev['p_value'], ref['p_value'], rtol=1e-6, atol=1e-300)
    both = coupling_tests(popn, x, include_self=True)
    assert np.all(np.isfinite(both['q_value'])) and np.array_equal(both['wald'], dev['wald'])
    part = coupling_tests(popn, x, n_lo=1, n_hi=3)
    assert part['wald'].shape == (2, N) and np.array_equal(part['wald'], dev['wald'][1:3])
    assert np.all(np.isnan(part['q_value'][[0, 1], [1, 2]]))


def test_one_step_lr_against_the_host_objective(fitted, monkeypatch):
    """lr1 against the same points through the host objective (compute_lp_grad_packed), to an absolute 4e-10 max(1, |log
    post|): the project's ll parity of 1e-10 on two terms, doubled.  The points are restated on the host from the device's
    factor W: u by the gcc mirror (the kernel's bits), theta - W u by numpy (connectivity.one_step_points).  They differ from
    the device's by the rounding of one triangular product, P u |theta| ~ 1e-14, which moves a log posterior whose gradient
    is of the order 1e3 by 1e-11 at the most: below the bound by four orders."""
    from theano_pyglm_amd.inference import connectivity as CN
    from theano_pyglm_amd.inference.laplace import laplace_on_device, theta_positions
    from theano_pyglm_amd.utils.packvec import unpackdict, set_vars
    popn, x, host, tol = fitted
    N, B = popn.N, popn.glm.imp_model.B
    res = CN.coupling_tests(popn, x, one_step_lr=True)
    lap, _, pi, shapes = laplace_on_device(popn, x)
    W = lap['W'].cpu().numpy()
    first = 1 + popn.glm.Dstim
    theta = popn.theta_matrix(x)
    out, u = WR.host_wald(W, theta, first, N, B, CN.effective_weight_contrast(popn), want_u=True)
    assert WR.same_bits(out[..., 0], res['wald'])                                  # (the same factor, the same bits)
    pts = CN.one_step_points(theta, W, u, first, N, B).reshape(N, N, -1)           # [pre g, post m]
    syms = popn.glm_syms()
    lp_hat, _ = popn.compute_lp_grad_packed(x)
    worst = 0.0
    for m in range(N):
        for g in range(N):
            assert np.all(pts[g, m, first + g * B:first + (g + 1) * B] == 0.0)     # the group's entries: exact zeros
            packed = np.zeros(pi.size)
            packed[pi] = pts[g, m]
            x2 = copy.deepcopy(x)
            set_vars(syms, x2['glms'][m], unpackdict(packed, shapes))
            lp, _ = popn.compute_lp_grad_packed(x2, m, m + 1)
            want = 2.0 * (lp_hat[m] - lp[0])
            err = abs(res['lr1'][m, g] - want)
            worst = max(worst, err / max(1.0, abs(lp_hat[m])))
            assert err <= 4e-10 * max(1.0, abs(lp_hat[m]))
    print("lr1 against the host objective: worst %.2e of max(1, |log post|)" % worst)
    assert np.array_equal(res['lr1_minus_wald'], res['lr1'] - res['wald'])
    rel = np.abs(res['lr1_minus_wald']) / np.maximum(res['wald'], 1.0)
    print("|lr1 - T| / max(T, 1): median %.3e max %.3e" % (np.median(rel), np.max(rel)))
    assert np.all(np.isfinite(res['lr1']))
    # one presynaptic neuron per chunk: the same bits
    monkeypatch.setattr(CN, 'EVAL_BUDGET_BYTES', 1)
    one = CN.coupling_tests(popn, x, one_step_lr=True)
    assert np.array_equal(one['lr1'], res['lr1']) and np.array_equal(one['wald'], res['wald'])


def test_synth_map_coupling_table_with_a_true_model(fitted):
    """harness/synth_map.py: coupling_table as --coupling-test --coupling-lr runs it, with a true model whose network has
    absent couplings: the truth it counts against is W_eff[pre, post] != 0 read as [post, pre]."""
    from theano_pyglm_amd.harness.synth_map import coupling_table
    from theano_pyglm_amd.inference import connectivity as CN
    popn, x, host, tol = fitted
    N = popn.N

    class TrueModel(object):                                   # (what coupling_table asks of the true population)
        def W_eff(self, vars):
            return vars['Weff']

    Weff = np.ones((N, N))
    Weff[0, 2] = Weff[3, 1] = Weff[1, 0] = 0.0                   # pre 0 -> post 2, pre 3 -> post 1, pre 1 -> post 0 absent
    text = coupling_table(popn, x, 0.05, True, TrueModel(), {'Weff': Weff})
    print(text)
    res = CN.coupling_tests(popn, x, alpha=0.05)
    truth = np.ones((N, N), dtype=bool)
    truth[2, 0] = truth[1, 3] = truth[0, 1] = False
    d = CN.detection_counts(res, truth)
    assert (d['positives'], d['negatives']) == (N * N - N - 3, 3)
    lines = text.splitlines()
    assert lines[0].startswith("coupling tests (Wald, %d d.o.f., Benjamini-Hochberg at 0.05): %d of %d pairs significant; %d of %d rows"
                               % (res['dof'], int(res['significant'].sum()), N * N - N, N, N))
    assert lines[1] == CN.format_table(res, 0.05, truth).splitlines()[1]
    assert "%d true couplings, 3 absent" % (N * N - N - 3) in lines[1] and ("area under the ROC of T %.3f" % d['auc']) in lines[1]
    assert lines[2].startswith("one-step likelihood ratio: |lr1 - T| / max(T, 1) median") and "over %d pairs" % (N * N) in lines[2]
    assert lines[3].startswith("(coupling tests in ")
    plain = coupling_table(popn, x)                              # without a true model and without lr1: the first line and the time
    assert len(plain.splitlines()) == 2 and plain.splitlines()[0] == lines[0]
