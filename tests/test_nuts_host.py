"""CPU tests of the NUTS row state machine (csrc/pglm_nuts.h built by gcc: tests/nuts_mirror.py) against the list
statement inference/nuts.py: nuts_transition, its moments on a Gaussian with a closed form, its dual averaging, and the
stateless draws (subset = batch, repeat = same bits)."""
import numpy as np
import pytest

from tests import nuts_mirror as NM
from theano_pyglm_amd.inference import nuts as NUTS
from theano_pyglm_amd.inference.batched_hmc import summarize

P = 5
_R = np.random.RandomState(7)
_B = _R.randn(P, P)
COV = _B.dot(_B.T) / P + 0.2 * np.eye(P)                       # a correlated Gaussian: condition number ~ 30
PREC = np.linalg.inv(COV)
MEAN = np.array([1.0, -2.0, 0.5, 0.0, 3.0])


def gauss(X):
    D = X - MEAN
    return -0.5 * np.einsum('mi,ij,mj->m', D, PREC, D), -D.dot(PREC)


def quartic(X):                                               # a non-quadratic term: the leapfrog energies err
    ll, g = gauss(X)
    return ll - 0.1 * np.sum(X ** 4, axis=1), g - 0.4 * X ** 3


def _mass(kind, M):
    if kind == 'identity':
        return None, None
    if kind == 'diag':
        return np.tile(np.diag(COV) * np.array([0.5, 1.0, 2.0, 1.0, 0.7]), (M, 1)), None
    W = np.linalg.cholesky(COV) + np.triu(np.full((P, P), 7.5), 1)          # junk above the diagonal: never read
    return None, np.tile(W, (M, 1, 1))


# (target, mass, max_depth, step0, seed): 2 rows x 200 transitions each
CASES = [(t, m, d, s, 3) for t in ('gauss', 'quartic') for m, s in (('identity', 0.35), ('diag', 0.5), ('dense', 0.6))
         for d in (3, 6)] + [('quartic', 'identity', 6, 1.9, 5), ('quartic', 'dense', 3, 2.5, 5)]
_STOPS = {}


def _compare_case(tname, mname, D, step0, seed):
    tgt = gauss if tname == 'gauss' else quartic
    M, n_trans, n_lo = 2, 200, 3
    minv, W = _mass(mname, M)
    X0 = MEAN + 0.3 * np.random.RandomState(11).randn(M, P)
    mir = NM.Mirror(tgt, X0, n_trans, max_depth=D, n_lo=n_lo, step0=step0, seed=seed, minv=minv, W=W)
    mir.run()
    stops, inner = np.zeros(5, dtype=int), 0
    for r in range(M):
        assert len(mir.log[r]) == n_trans                      # all transitions are compared
        Wr = W[r] if W is not None else (np.diag(np.sqrt(minv[r])) if minv is not None else None)
        q = X0[r].copy()
        ll, g = tgt(q[None])
        U, g = -ll[0], -g[0]
        for t in range(n_trans):
            ref = NUTS.nuts_transition(q, U, g, lambda x: tuple(-a[0] for a in tgt(x[None])), step0, D,
                                       *NM.draws(seed, n_lo + r, t, P, D), W=Wr)
            got = mir.log[r][t]
            assert (got['depth'], got['n_leaf'], got['stop'], got['sel']) == \
                (ref['depth'], ref['n_leaf'], ref['stop'], ref['sel']), (tname, mname, D, r, t, got, ref)
            assert np.max(np.abs(got['q'] - ref['q'])) <= 1e-12 * max(1.0, np.max(np.abs(ref['q'])))
            assert abs(got['alpha'] - ref['alpha']) <= 1e-12
            stops[ref['stop']] += 1
            # an inner block: the subtree was discarded before its last leaf
            inner += ref['stop'] == NUTS.STOP_SUB and ref['n_leaf'] < 2 ** ref['depth'] - 1
            q, U, g = got['q'], ref['U'], ref['g']              # (the machine's point: errors do not accumulate)
        assert np.array_equal(mir.samples[:, r], np.array([e['q'] for e in mir.log[r]]))
    return stops, inner


@pytest.mark.parametrize('case', CASES, ids=lambda c: "%s-%s-d%d-step%g" % c[:4])
def test_state_machine_equals_list_statement(case):
    stops, inner = _compare_case(*case)
    print(case, "stops (sub, tree, depth, divergent):", stops[1:], "inner blocks:", inner)
    _STOPS[case] = (stops, inner)


def test_every_stop_reason_occurs():
    for c in CASES:
        if c not in _STOPS:
            _STOPS[c] = _compare_case(*c)
    tot = sum(s for s, _ in _STOPS.values())
    inner = sum(i for _, i in _STOPS.values())
    print("stops (sub, tree, depth, divergent):", tot[1:], "inner sub-blocks:", inner)
    assert tot[NUTS.STOP_SUB] > 0 and inner > 0 and tot[NUTS.STOP_TREE] > 0
    assert tot[NUTS.STOP_DEPTH] > 0 and tot[NUTS.STOP_DIVERGENT] > 0


def _restated_steps(step0, alphas, delta):
    """Hoffman & Gelman (2014) algorithm 5, restated: the step after each warm-up transition; the last is exp(log ebar)."""
    mu, hbar, lebar, steps = np.log(10.0 * step0), 0.0, 0.0, []
    for m, a in enumerate(alphas, 1):
        hbar = (1.0 - 1.0 / (m + 10.0)) * hbar + (delta - a) / (m + 10.0)
        le = mu - np.sqrt(m) / 0.05 * hbar
        lebar = m ** -0.75 * le + (1.0 - m ** -0.75) * lebar
        steps.append(np.clip(np.exp(lebar if m == len(alphas) else le), 1e-4, 10.0))
    return np.array(steps)


def test_moments_acceptance_and_dual_averaging():
    M, n_keep, n_warm, delta = 2, 4000, 500, 0.8
    X0 = np.tile(MEAN, (M, 1))
    mir = NM.Mirror(gauss, X0, n_keep, n_warmup=n_warm, max_depth=8, step0=0.1, seed=17, delta=delta)
    mir.run()
    s = summarize(mir.samples)
    sd = np.sqrt(np.diag(COV))
    for r in range(M):
        se = s['sd'][r] / np.sqrt(s['ess'][r])
        print("row %d: ess %s, mean error / se %s, var ratio %s" % (r, np.round(s['ess'][r]), np.round((s['mean'][r] - MEAN) / se, 2),
                                                                  np.round(s['sd'][r] ** 2 / sd ** 2, 3)))
        assert np.all(np.abs(s['mean'][r] - MEAN) <= 4.0 * se)
        assert np.all(np.abs(s['sd'][r] ** 2 / sd ** 2 - 1.0) <= 0.15)
        alphas = np.array([e['alpha'] for e in mir.log[r]])
        steps = np.array([e['step'] for e in mir.log[r]])
        assert abs(alphas[n_warm:].mean() - delta) <= 0.05
        assert abs(mir.sc[NM.SC['acc_post'], r] / (len(alphas) - n_warm) - alphas[n_warm:].mean()) <= 1e-12
        want = _restated_steps(0.1, alphas[:n_warm], delta)
        assert np.max(np.abs(steps[:n_warm] / want - 1.0)) <= 1e-12
        assert np.all(steps[n_warm:] == steps[n_warm - 1]) and mir.sc[NM.SC['step'], r] == steps[-1]
        assert np.allclose(NUTS.dual_averaging_steps(0.1, alphas[:n_warm], delta), want, rtol=1e-12, atol=0.0)


def test_subset_equals_batch_and_repeat_is_bit_equal():
    X0 = MEAN + 0.3 * np.random.RandomState(5).randn(4, P)
    kw = dict(n_warmup=6, thin=2, max_depth=5, step0=0.2, seed=23)

    def chain(lo, hi):
        m = NM.Mirror(quartic, X0[lo:hi], 10, n_lo=lo, **kw)
        m.run()
        return m
    full, again, sub = chain(0, 4), chain(0, 4), chain(1, 3)
    assert np.array_equal(full.st, again.st) and np.array_equal(full.samples, again.samples)
    assert np.array_equal(sub.samples, full.samples[:, 1:3]) and np.array_equal(sub.stats, full.stats[:, :, 1:3])
    assert np.array_equal(sub.sc[NM.SC['step']], full.sc[NM.SC['step'], 1:3])
    assert np.all(full.done()) and np.all(full.sc[NM.SC['t']] == 26)
    assert len(set(full.sc[NM.SC['n_leapfrog']])) > 1          # the rows did not take the same number of steps


def test_synth_map_takes_nuts():
    import inspect
    from theano_pyglm_amd.harness import synth_map
    assert inspect.signature(synth_map.run_synth_test).parameters['nuts'].default == 0
    assert list(inspect.signature(synth_map.nuts_bias_table).parameters)[:5] == ['popn', 'x', 'n_draws', 'mass', 'laplace_device']
    assert "--nuts N" in synth_map.__doc__


def test_synth_map_main_passes_nuts_and_its_mass_on(tmp_path, monkeypatch):
    """main() with --nuts: the flag and --hmc-mass reach run_synth_test (the fit itself is replaced: no GPU here)."""
    import pickle
    from theano_pyglm_amd.harness import synth_map
    data = tmp_path / 'data.pkl'
    data.write_bytes(pickle.dumps({'N': 2}))
    seen = {}
    monkeypatch.setattr(synth_map, 'run_synth_test', lambda *a, **kw: seen.update(kw, args=a))
    synth_map.main(['-d', str(data), '-r', str(tmp_path), '--nuts', '7', '--hmc-mass', 'laplace_dense'])
    assert seen['nuts'] == 7 and seen['hmc_mass'] == 'laplace_dense' and seen['hmc'] == 0 and seen['args'][1] == {'N': 2}
    assert synth_map.parser().parse_args(['-d', 'x']).nuts == 0
