"""CPU tests of the lock-step dense Newton optimiser's core (theano_pyglm_amd/csrc/pglm_newton.h, compiled for the host with
gcc through tests/csrc/newton_host.c and driven by tests/newton_mirror.py with numpy supplying f, g, the Hessian, the factor
and the solve): it takes the iterates of a scalar numpy Newton driver that follows the same rules with code of its own, ends a
quadratic in one iteration, climbs the shift ladder where the Hessian is not positive definite and falls back on steepest
descent where it cannot be factored; plus the host side of the public interface.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import glm_oracle as O
from tests import chol_cases as CC
from tests import helpers as H
from tests import hessian_reference as HR
from tests import newton_mirror as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = np.array(NM.LADDER)


# ---- 1. the mirror takes the iterates of a scalar driver ------------------------------------------------------------------
def glm_problem(kind, seed=7):
    """N = 3, 3000 bins, Gaussian priors: target(X) and hessian(X, rows) from the oracle and tests/hessian_reference.py."""
    p = H.Problem(3, 3000, H.std_ibasis(200), kind=kind, seed=seed,
                  **({'bias_mu': 1.0, 'w_scale': 0.5} if kind == 'explinear' else {}))
    prior = (0, 1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
    Sf = p.S.astype(float)

    def target(X):
        ll, g = np.zeros(p.N), np.zeros((p.N, p.P))
        for n in range(p.N):
            ll[n], gb, _, gw = O.glm_ll_grad(n, Sf, p.fS, X[n, 1:].reshape(p.N, p.B), p.Weff[:, n], X[n, 0], p.dt, p.kind,
                                             None, None)
            g[n] = np.concatenate([[gb], gw.reshape(-1)])
        return ll, g

    def hessian(Xl, rows):
        keep = p.theta.copy()
        try:
            p.theta[rows] = Xl
            return HR.ref_hessian(p, list(rows))[0]
        finally:
            p.theta[:] = keep

    return p, prior, target, hessian


def scalar_newton(target, hessian, x0, r, prior, N, B, gtol, maxiter):
    """One row, no state machine: Newton with the ladder, numpy's own Cholesky and solve, scipy's DCSRCH wrapper for the
    search (scalar_search_wolfe1 with the machine's constants; without an old value its first step is 1).  Returns the
    iterates [x_0, x_1, ..] and the status."""
    from scipy.optimize._linesearch import scalar_search_wolfe1
    X = np.array(x0, dtype=float)

    def fg(x):
        X[r] = x
        ll, g = target(X)
        f, gg = NM.objective(X[r:r + 1], ll[r:r + 1], g[r:r + 1], prior, N, B, 0)
        return float(f[0]), gg[0]

    x = X[r].copy()
    its = [x.copy()]
    f, g = fg(x)
    for _ in range(maxiter):
        if np.max(np.abs(g)) <= gtol:
            return its, 0
        A0 = -(hessian(x[None], [r])[0] + NM.prior_hessian(x, prior, N, B, 0))
        p = None
        for shift in LADDER:
            A = A0 + shift * np.diag(np.diag(A0))
            s = np.sqrt(np.diag(A))
            try:
                Lc = np.linalg.cholesky(A / np.outer(s, s))
            except np.linalg.LinAlgError:
                continue
            cand = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g / s)) / s
            if g.dot(cand) < 0:
                p = cand
                break
        if p is None:
            p = -g
        cache = {}

        def phi(a):
            cache[a] = fg(x + a * p)
            return cache[a][0]

        def dphi(a):
            return cache[a][1].dot(p)

        a, f1, _ = scalar_search_wolfe1(phi, dphi, f, None, g.dot(p), c1=1e-4, c2=0.9, amax=50.0, amin=1e-8, xtol=1e-14)
        assert a is not None
        x = x + a * p
        f, g = cache[a]
        its.append(x.copy())
    return its, (0 if np.max(np.abs(g)) <= gtol else 1)


@pytest.mark.parametrize('kind', ['exp', 'explinear'])
def test_mirror_takes_the_scalar_drivers_iterates(kind):
    """Same target, same Hessian, same start; the bound is the one tests/test_newton_cg_host.py holds the Newton-CG core to
    against scipy (1e-10 of the largest iterate entry): two float64 implementations of the same steps differ by rounding
    alone (numpy's Cholesky against numpy_factor + solve_triangular, blocked against sequential dot products)."""
    p, prior, target, hessian = glm_problem(kind)
    gtol, maxiter = 1e-6, 30
    m = NM.Mirror(target, hessian, p.theta, p.N, p.B, 0, prior, gtol=gtol, maxiter=maxiter).init()
    rec = [[p.theta[r].copy()] for r in range(p.N)]
    while not np.all(m.field('phase') == NM.PHASE_DONE):
        nit = m.field('nit').copy()
        m.outer()
        for r in np.nonzero(m.field('nit') > nit)[0]:
            rec[r].append(m.vec[r, 0].copy())
    assert np.all(m.field('status') == 0), m.field('status')
    for r in range(p.N):
        its, status = scalar_newton(target, hessian, p.theta, r, prior, p.N, p.B, gtol, maxiter)
        scale = max(np.max(np.abs(v)) for v in its)
        assert status == 0 and len(its) == len(rec[r]) == int(m.field('nit')[r]) + 1
        err = max(np.max(np.abs(a - b)) for a, b in zip(its, rec[r])) / scale
        print("%s row %d: nit %d nfev %d nhess %d nfact %d, max iterate error %.2e" % (
            kind, r, m.field('nit')[r], m.field('nfev')[r], m.field('nhess')[r], m.field('nfact')[r], err))
        assert err <= 1e-10
        assert m.field('nit')[r] >= 2 and m.field('nhess')[r] == m.field('nit')[r]
        assert all(np.array_equal(s, [0.0]) for s in m.shifts[r]) and m.fallback[r] == 0      # the plain path


# ---- 2. quadratics: one iteration, the ladder, the fallback ---------------------------------------------------------------
def quadratic_mirror(A_true, H_seen, b, gtol, maxiter=50):
    """Rows minimise f_m = 0.5 x^T A_true[m] x - b[m]^T x from x = 0; the machine is shown -H_seen[m] as the Hessian of ll.
    No prior (prior None: f = -ll)."""
    M, P = b.shape

    def target(X):
        Ax = np.einsum('mij,mj->mi', A_true, X)
        return -(0.5 * np.sum(X * Ax, axis=1) - np.sum(b * X, axis=1)), -(Ax - b)

    def hessian(Xl, rows):
        return -H_seen[list(rows)]

    return NM.Mirror(target, hessian, np.zeros((M, P)), P - 1, 1, 0, None, gtol=gtol, maxiter=maxiter).init()


def test_quadratic_ends_in_one_iteration():
    """f = 0.5 x^T A x - b^T x with A from chol_cases.spd_stack (entries over 24 orders of magnitude), b = A x*: the Newton
    step is the solution, step 1 satisfies both Wolfe conditions (phi'(1) = 0 up to rounding) and the gradient there is
    the residual of the solve.  gtol: 64 P u max_i (|A| |x*| + |b|)_i -- the componentwise backward error of a Cholesky
    solve is of order P u (Higham, Accuracy and Stability, theorem 10.4), with a margin of 64 for its constant."""
    M, P = 3, 33
    A = CC.spd_stack(M, P, 4242)
    rng = np.random.default_rng(5)
    d = np.sqrt(np.diagonal(A, axis1=1, axis2=2))
    xs = rng.standard_normal((M, P)) / d                       # (scaled like the solution of an equilibrated system)
    b = np.einsum('mij,mj->mi', A, xs)
    gtol = 64 * P * CC.U * np.max(np.einsum('mij,mj->mi', np.abs(A), np.abs(xs)) + np.abs(b))
    m = quadratic_mirror(A, A, b, gtol).run()
    print("gtol %.3e, max|g| at the end %.3e" % (gtol, np.max(np.abs(m.vec[:, 1]))))
    assert np.all(m.field('status') == 0)
    assert np.all(m.field('nit') == 1), m.field('nit')
    assert np.all(m.field('nfev') == 2) and np.all(m.field('nhess') == 1) and np.all(m.field('nfact') == 1)
    assert np.all(m.ls[:, 0] == 1.0)                           # the accepted step
    assert np.max(np.abs(m.vec[:, 0] - xs) * d) <= 1e-9


def test_shift_ladder_and_steepest_descent_fallback():
    """Row 0: positive definite (no shift).  Row 1: chol_cases.flip_eigenvalue on the smallest eigenvalue of the
    equilibrated matrix -- the plain factor fails, the ladder climbs until shift * diag A outweighs the flipped eigenvalue.
    Row 2: a well-scaled matrix shown to the machine with a NaN entry -- every factor fails and the row searches along -g.
    The quadratic of row 1 is unbounded below, so the fit is cut at maxiter = 2; f must fall at every iteration."""
    P = 12
    A = CC.spd_stack(3, P, 77)
    A[2] = CC.equilibrated(A[2])[0]
    w = np.linalg.eigvalsh(CC.equilibrated(A[1])[0])
    A[1] = CC.flip_eigenvalue(A[1], which=0)
    seen = A.copy()
    seen[2, 5, 2] = seen[2, 2, 5] = np.nan
    rng = np.random.default_rng(9)
    b = rng.standard_normal((3, P)) * np.sqrt(np.abs(np.diagonal(A, axis1=1, axis2=2)))
    x0s = np.linalg.solve(A[0], b[0])                          # (gtol as in the test above: row 0 ends after one step)
    gtol = 64 * P * CC.U * np.max(np.abs(A[0]).dot(np.abs(x0s)) + np.abs(b[0]))
    m = quadratic_mirror(A, seen, b, gtol, maxiter=2).run()
    assert m.field('status')[0] == 0 and m.field('nit')[0] == 1
    print("smallest eigenvalue flipped: %.3e; shifts %s; fallbacks %s; status %s; f %s"
          % (w[0], m.shifts, m.fallback, m.field('status'), m.f_trace))
    # the intended paths
    assert all(np.array_equal(s, [0.0]) for s in m.shifts[0]) and m.fallback[0] == 0
    first = np.array(m.shifts[1][0])
    assert len(first) >= 2 and np.allclose(first, LADDER[:len(first)], rtol=1e-12) and first[-1] > w[0]
    assert m.fallback[1] == 0 and m.field('nfact')[1] > m.field('nhess')[1]
    assert all(np.allclose(s, LADDER, rtol=1e-12) for s in m.shifts[2]) and m.fallback[2] == len(m.shifts[2]) >= 1
    assert m.field('nfact')[2] == len(LADDER) * m.field('nhess')[2]
    for r in range(3):
        assert m.field('status')[r] != 3
        assert len(m.f_trace[r]) >= 2 and np.all(np.diff(m.f_trace[r]) < 0), (r, m.f_trace[r])


def test_exits_of_the_machine():
    """maxiter <= 0: every row status 1 untouched; a start that is already converged: status 0, no Hessian; a gradient
    holding a NaN is zeroed and converges at once; a NaN objective at every trial: status 2, x unchanged."""
    P = 8
    A = CC.equilibrated(CC.spd_stack(1, P, 3)[0])[0][None]
    b = np.ones((1, P))
    m = quadratic_mirror(A, A, b, 1e-9, maxiter=0)
    assert m.field('status')[0] == 1 and m.field('phase')[0] == NM.PHASE_DONE and m.field('nit')[0] == 0
    m = quadratic_mirror(A, A, b, 10.0)
    assert m.field('status')[0] == 0 and m.field('nhess')[0] == 0 and m.field('nfev')[0] == 1
    m = quadratic_mirror(A, A, b, 1e-9)
    m.target = lambda X: (np.full(1, np.nan), np.zeros((1, P)))
    m.run()
    assert m.field('status')[0] == 2 and np.array_equal(m.vec[0, 0], np.zeros(P)) and m.field('nit')[0] == 0
    m = NM.Mirror(lambda X: (np.zeros(1), np.full((1, P), np.nan)), None, np.zeros((1, P)), P - 1, 1, 0, None).init()
    assert m.field('status')[0] == 0 and np.array_equal(m.vec[0, 1], np.zeros(P))


def test_prior_hessian_is_the_derivative_of_the_prior_gradient():
    """newton_mirror.prior_hessian (what pgl_newton_assemble_dev is held to) against central differences of
    newton_mirror.objective's gradient, Gaussian and group lasso, with a basis stimulus block."""
    N, B, D = 3, 4, 2
    P = 1 + D + N * B
    rng = np.random.default_rng(1)
    x = rng.standard_normal(P)
    for prior in ((0, 0.3, 1.7, 0.6, 0.2, 1.3, 0.0), (1, 0.3, 1.7, 0.6, 0.2, 1.3, 0.8)):
        Hp = NM.prior_hessian(x, prior, N, B, D)
        num = np.zeros((P, P))
        for c in range(P):
            e = np.zeros(P)
            e[c] = 1e-5
            gp = NM.objective((x + e)[None], np.zeros(1), np.zeros((1, P)), prior, N, B, D)[1][0]
            gm = NM.objective((x - e)[None], np.zeros(1), np.zeros((1, P)), prior, N, B, D)[1][0]
            num[:, c] = -(gp - gm) / 2e-5
        assert np.max(np.abs(Hp - num)) <= 1e-8 * max(1.0, np.max(np.abs(Hp)))
        assert np.array_equal(Hp, Hp.T)


# ---- 3. host side of the public interface ------------------------------------------------------------------------------
def test_keyword_errors_before_any_device_work():
    from theano_pyglm_amd.inference import batched_newton as B
    from theano_pyglm_amd.inference import coord_descent as cd
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = Population(make_model('standard_glm', N=2, dt=0.001))
    x = popn.sample(np.random.RandomState(1))
    for kw in ({'use_rop': True}, {'prox': True}, {'batched': True}, {'batched': False}):
        with pytest.raises(ValueError, match="newton=True"):
            cd.coord_descent(popn, x, newton=True, **kw)
    assert B.supported(popn)
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):
        p2 = Population(make_model(name, N=2, dt=0.001))
        assert not B.supported(p2)
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            cd.coord_descent(p2, p2.sample(np.random.RandomState(1)), newton=True)
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            B.fit_glms_newton_torch(p2, p2.sample(np.random.RandomState(1)))


def test_newton_symbols_layout_and_kernels():
    import __graft_entry__ as ge
    ge.build_hip()
    import sys
    from theano_pyglm_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    names = ('pgl_chol_solve_dev', 'pgl_newton_state_doubles', 'pgl_newton_init_dev', 'pgl_newton_assemble_dev',
             'pgl_newton_direction_dev', 'pgl_newton_trial_dev', 'pgl_newton_search_step_dev')
    hdr = open(os.path.join(ROOT, 'include', 'pyglm_hip.h')).read()
    for n in names:
        assert hasattr(lib, n) and n in _lib.SYMBOLS and (n + '(') in hdr
    for m in ('chol_solve', 'newton_state_doubles', 'newton_init_dev', 'newton_assemble_dev', 'newton_direction_dev',
              'newton_trial_dev', 'newton_search_step_dev'):
        assert hasattr(_lib.DeviceGlm, m)
    assert _lib.load().pgl_newton_state_doubles(3, 7) == 3 * 7 * 5 + 3 * (len(NM.FIELDS) + NM.NLS)
    src = open(os.path.join(ROOT, 'theano_pyglm_amd', 'csrc', 'pglm_newton.h')).read()
    for text in ('#define PGL_NEWTON_SHIFT0 1e-6', '#define PGL_NEWTON_SHIFT_MUL 100.0', '#define PGL_NEWTON_SHIFT_MAX 1e2'):
        assert text in src
    ladder = [0.0]
    while NM.lib().newton_next_shift(ladder[-1]) > 0:
        ladder.append(NM.lib().newton_next_shift(ladder[-1]))
    assert np.allclose(ladder, LADDER, rtol=1e-12) and len(ladder) == len(LADDER)
    # the new kernels use no scratch and spill nothing (the compiler's resource report in the code object's metadata)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import reachable_kernels as RK
    built = RK.built_fused()
    mine = dict((n, r) for n, r in built.items() if n.startswith('k_newton_') or n in ('k_chol_solve', 'k_row_trial'))
    assert sorted(mine) == ['k_chol_solve', 'k_newton_assemble', 'k_newton_direction', 'k_newton_init',
                            'k_newton_search_step', 'k_row_trial'], sorted(mine)  # (k_row_trial: shared with Newton-CG)
    for n, r in mine.items():
        assert r['scratch'] == 0 and r['spill_vgpr'] == 0, (n, r)
