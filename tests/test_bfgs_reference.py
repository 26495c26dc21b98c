"""CPU tests of the numpy reference of the lock-step BFGS row kernels (tests/bfgs_reference.py): it is scipy's BFGS, its
dense matrix, its update history and its dense-with-pending-update form are one algebra, the device block packs and unpacks
bit for bit, and every single-launch case that tests/test_gpu_bfgs_rows.py runs on the device is valid -- no decision of it
hangs on rounding -- and takes the branch it is named for."""
import ctypes
import os

import numpy as np
import pytest
import scipy.optimize as opt

from tests import bfgs_reference as R

NAMES = [c['name'] for c in R.CASES]


def _convex(P, quartic):
    """a quadratic of condition number 100 (eigenvalues log-spaced in [1, 100], rotated), optionally plus a quartic"""
    rng = np.random.default_rng(7 + P)
    Q = np.linalg.qr(rng.standard_normal((P, P)))[0]
    A = (Q * np.logspace(0, 2, P)) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.standard_normal(P)
    q = 0.5 if quartic else 0.0

    def fun(x):
        return float(0.5 * x @ A @ x - b @ x + 0.25 * q * np.sum(x ** 4)), A @ x - b + q * x ** 3

    return fun, rng.standard_normal(P)


@pytest.mark.parametrize('quartic', [False, True])
@pytest.mark.parametrize('P', [2, 26, 71])
def test_reference_is_scipys_bfgs(P, quartic):
    """Convex objectives, no restart: the same nit and nfev as scipy.optimize.minimize(method='BFGS'), and iterates equal to
    scipy's callback iterates.  Tolerance: 10 x the largest relative difference between the reference's own two runs, sums in
    longdouble against plain float64 np.dot (scipy's BLAS order is a third ordering of the same sums).  Measured here over
    the six cases: one ulp (P = 2, the floor of the measurement) to 1.0e-11 (P = 71, 58 iterations); scipy lies within 0 to 2.4 x of it (printed by the test)."""
    fun, x0 = _convex(P, quartic)
    f1 = lambda r, x: fun(x)
    st, its, log, _ = R.fit(f1, x0[None, :], gtol=1e-5, maxiter=225, init_scaling=0, sums='ld')
    st2, its2, _, _ = R.fit(f1, x0[None, :], gtol=1e-5, maxiter=225, init_scaling=0, sums='f64')
    xs = []
    res = opt.minimize(lambda v: fun(v)[0], x0, jac=lambda v: fun(v)[1], method='BFGS', callback=lambda xk: xs.append(xk.copy()),
                       options=dict(gtol=1e-5, maxiter=225))
    assert not any(d['reset'] or d['again'] for decs in log for d in decs)
    assert int(st.iters[0]) == res.nit and int(st.nfev[0]) == res.nfev - 1, (st.iters[0], res.nit, st.nfev[0], res.nfev)
    assert len(its2[0]) == len(its[0]) == len(xs)
    scale = max(np.max(np.abs(x)) for x in xs)
    # (one ulp is the resolution of this measurement: at P = 2 both orderings give the same bits)
    measured = max(max(np.max(np.abs(a - b)) for a, b in zip(its[0], its2[0])) / scale, 2.0 ** -52)
    worst = max(np.max(np.abs(a - b)) for a, b in zip(its[0], xs)) / scale
    print("P %d quartic %d: nit %d nfev %d, longdouble against float64 sums %.3e, against scipy %.3e"
          % (P, quartic, res.nit, res.nfev, measured, worst))
    assert worst <= 10 * measured


@pytest.mark.parametrize('name', NAMES)
def test_the_forms_are_one_algebra(name):
    """The reference's real matrix is advanced by the product formula (I - rho s y^T) H (I - rho y s^T) + rho s s^T alone.  H
    rebuilt from the history as hscale I + sum_j U_j V_j^T, and H of the dense form with its pending update, equal it before
    and after the launch, to the rounding of the stored factors (8 n 2^-53 m per entry, n = 3 per stored update) plus, after
    the launch, what the bounds of the factors written by it allow.  pack / unpack round-trip bit for bit."""
    for form in ('merged', 'dense'):
        st0, args, spec, st1, out = R.run_case(name, form)
        for st in (st0, st1):
            for r in range(st.M):
                tl = lambda nm, shp: st.tol[nm][r] if nm in st.tol else np.zeros(shp)
                if st.form == 'hist':
                    Hm = R.history_matrix(st, r)
                    K = int(st.hk[r])
                    S, HY, c = np.abs(st.hist[r, :K, 0]), np.abs(st.hist[r, :K, 1]), np.abs(st.coef[r, :K])
                    mag = abs(st.hscale[r]) * np.eye(st.P) + np.einsum('k,ki,kj->ij', c[:, 0], S, S) + \
                        np.einsum('k,ki,kj->ij', c[:, 1], HY, S) + np.einsum('k,ki,kj->ij', c[:, 1], S, HY)
                    n = 3 * K + 1
                    tH, tc = tl('hist', st.hist[r].shape)[:K, 1], tl('coef', st.coef[r].shape)[:K]
                    extra = np.einsum('k,ki,kj->ij', tc[:, 0], S, S) + np.einsum('k,ki,kj->ij', tc[:, 1], HY, S) + \
                        np.einsum('k,ki,kj->ij', tc[:, 1], S, HY) + np.einsum('k,ki,kj->ij', c[:, 1], tH, S) + \
                        np.einsum('k,ki,kj->ij', c[:, 1], S, tH) + float(tl('hscale', ())) * np.eye(st.P)
                else:
                    Hm = R.dense_matrix(st, r)
                    mag = np.abs(np.asarray(Hm, dtype=np.float64)) + np.abs(st.U[r]) @ np.abs(st.V[r]).T
                    n = 5
                    extra = tl('U', st.U[r].shape) @ np.abs(st.V[r]).T + np.abs(st.U[r]) @ tl('V', st.V[r].shape).T + \
                        float(tl('hscale', ())) * np.eye(st.P)
                    if st.ident[r] == 0:
                        extra = extra + tl('Hd', st.Hd[r].shape)[:, :st.P]
                err = np.abs(np.asarray(Hm - st.H[r], dtype=np.float64))
                assert np.all(err <= 8 * n * R.U53 * mag + extra), (name, form, r, float(np.max(err / (8 * n * R.U53 * mag + extra))))
            a = R.pack(st)
            assert a.size == R.state_doubles(st.M, st.P)
            b = R.pack(R.unpack(a, st.M, st.P))
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
            u = R.unpack(a, st.M, st.P)
            for nm in R.VEC + R.SCAL + ('U', 'V', 'ls'):
                assert np.array_equal(getattr(u, nm), getattr(st, nm), equal_nan=True), nm


def test_state_doubles_is_the_librarys():
    from theano_pyglm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpyglm_hip.so is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.pgl_bfgs_state_doubles.restype = ctypes.c_longlong
    lib.pgl_bfgs_state_doubles.argtypes = [ctypes.c_int, ctypes.c_int]
    for M, P in [(1, 1), (3, 65), (5, 513)] + [(len(c['rows']), c['P']) for c in R.CASES]:
        assert lib.pgl_bfgs_state_doubles(M, P) == R.state_doubles(M, P)


@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('name', NAMES)
def test_every_gpu_case_is_valid_and_takes_its_branch(name, form):
    st0, args, spec, st1, out = R.run_case(name, form)
    for d in out['decisions']:
        assert d['dp_stable'], d
        assert d['sy_margin'] >= R.MARGIN and d['sl_margin'] >= R.MARGIN, d
    exp = R.expected_decisions(spec)
    assert len(exp) == len(out['decisions'])
    for d, e in zip(out['decisions'], exp):
        assert all(d[k] == v for k, v in e.items()), (d, e)
    assert R.KMAX > spec['hk_bound'] >= 1
    # the history slots no update has reached hold 1e30 and stay so (a reset row keeps its old entries: nobody reads them)
    if st1.form == 'hist':
        for r in range(st1.M):
            k = int(max(st0.hk[r] + 1, st1.hk[r]))           # (an update appended just before a reset included)
            assert np.all(st1.hist[r, k:] == 1e30) and np.all(st1.coef[r, k:] == 1e30)


def test_the_cases_cover_what_they_are_meant_to():
    """every P, history length, list kind and outcome the GPU test is to see occurs in some case"""
    assert {c['P'] for c in R.CASES} == {1, 2, 63, 64, 65, 129, 255, 256, 257, 261, 513}
    assert {rs['hk'] for c in R.CASES for rs in c['rows']} >= {0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 33}
    assert {len(c['rows']) for c in R.CASES} >= {1, 3, 5}
    assert any(c.get('list') and len(c['list']) < len(c['rows']) for c in R.CASES)
    assert any(c.get('pos_next') and -1 in [c['pos_next'][r] for r in c['list']] for c in R.CASES)
    assert {rs['out'] for c in R.CASES for rs in c['rows']} == set(R.EXPECT)
    assert {c.get('init_scaling', 0) for c in R.CASES if any(rs.get('restarts') and rs['hk'] == 0 and rs['out'] == 'conv'
                                                              for rs in c['rows'])} == {0, 1}
