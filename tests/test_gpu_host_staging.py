"""The host-array forms share one set of staging buffers on the handle (pgl_context::stage): what one call leaves there must
never reach the next.  One handle serves every host form in turn -- forwards at the full sizes, backwards with every size
about a quarter (each slot then holds a longer, older array than the call needs), forwards again at the full sizes (each slot
grows back), with a KS and an ACF call of no values at all between large ones (the one-element floor of stage_up) -- and every
result must equal, bit for bit, the same call on a fresh handle that has served nothing else.

Shape: the smallest population of the goodness-of-fit tests, 8 neurons, and three 256-bin chunks plus a ragged tail."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N, NT = 8, 3 * 256 + 37
_problem = []


def problem():
    if not _problem:
        _problem.append(H.Problem(N, NT, H.std_ibasis(200), kind='explinear', seed=211, weighted=True, rate_hz=50.0))
    return _problem[0]


def _inputs(q):
    """The arrays of every call, all sizes divided by q."""
    rng = np.random.default_rng(300 + q)
    ks_lens = [4300 // q, 500 // q, 200 // q]                # (q = 1: the first segment crosses the 4096-value sort tile)
    acf_runs = [[1500 // q, 1500 // q], [1000 // q], [600 // q, 400 // q]]
    lens = [l for seg in acf_runs for l in seg]
    return {
        'ks_tau': rng.exponential(size=sum(ks_lens)), 'ks_off': np.concatenate(([0], np.cumsum(ks_lens))),
        'psis_ll': -50.0 + 3.0 * rng.standard_normal((32 // q, 7 if q == 1 else 2)),
        'diag_x': rng.standard_normal((64 // q, 2 * (3 if q == 1 else 1), 2)),
        'acf_tau': rng.exponential(size=sum(lens)), 'acf_run_off': np.concatenate(([0], np.cumsum(lens))),
        'acf_seg_run': np.concatenate(([0], np.cumsum([len(seg) for seg in acf_runs]))),
        'range': (0, NT) if q == 1 else (0, 208), 'rows': (0, N) if q == 1 else (2, 4),
        'v': rng.standard_normal((N, 1 + N * 8)),             # (cut to P columns at the call)
    }


FULL, QUARTER = _inputs(1), _inputs(4)
NONE = {'ks_tau': np.zeros(0), 'ks_off': np.zeros(4, dtype=np.int64), 'acf_tau': np.zeros(0),
        'acf_run_off': np.zeros(3, dtype=np.int64), 'acf_seg_run': np.arange(3)}


def _draw(fn):
    def call(d, p, i):
        d.set_time_range(*i['range'])
        return fn(d, p, i)
    return call


def _rows(fn):
    def call(d, p, i):
        lo, hi = i['rows']
        d.set_time_range(*i['range'])
        return fn(d, p, i, lo, hi)
    return call


def _flat(r):
    return tuple(x for x in r if x is not None) if isinstance(r, tuple) else (r,)


CALLS = [
    ('ks_uniform_host', lambda d, p, i: d.ks_uniform_host(i['ks_tau'], i['ks_off'], zsorted=True)),
    ('psis_loo_host', lambda d, p, i: d.psis_loo_host(i['psis_ll'], weights=True)),
    ('chain_diag_host', lambda d, p, i: d.chain_diag_host(i['diag_x'], n_chains=2)),
    ('rescale_acf_host', lambda d, p, i: d.rescale_acf_host(i['acf_tau'], i['acf_run_off'], i['acf_seg_run'], 8, scores=True)),
    ('pointwise', _draw(lambda d, p, i: d.pointwise(p.theta, p.Weff, 1))),
    ('rate_windows', _draw(lambda d, p, i: d.rate_windows(p.theta, p.Weff, 50))),
    ('rescale', _draw(lambda d, p, i: d.rescale(p.theta, p.Weff))),
    ('rescale_corr', _draw(lambda d, p, i: d.rescale_corr(p.theta, p.Weff, seed=5, draw=1))),
    ('hvp', _rows(lambda d, p, i, lo, hi: d.hvp(p.theta[lo:hi], i['v'][lo:hi, :p.P], p.Weff, lo, hi))),
    ('hessian', _rows(lambda d, p, i, lo, hi: d.hessian(p.theta[lo:hi], p.Weff, lo, hi))),
    ('ll_grad', _rows(lambda d, p, i, lo, hi: d.ll_grad(p.theta[lo:hi], p.Weff, lo, hi))),
]


def _alone(fn, inputs):
    p = problem()
    d = p.device(0)
    try:
        return _flat(fn(d, p, inputs))
    finally:
        d.close()


def test_shared_staging_never_leaks_between_host_forms():
    p = problem()
    calls = dict(CALLS)
    alone = {(name, id(i)): _alone(fn, i) for name, fn in CALLS for i in (FULL, QUARTER)}
    for name in ('ks_uniform_host', 'rescale_acf_host'):
        alone[(name, id(NONE))] = _alone(calls[name], NONE)
    assert alone[('ks_uniform_host', id(FULL))][0][0, 3] == 4300 and alone[('ks_uniform_host', id(NONE))][0].shape == (3, 4)
    assert alone[('psis_loo_host', id(FULL))][1].shape == (32, 7) and alone[('rescale', id(FULL))][0].size > 100
    third = []                                               # forwards again, the calls of no values between large ones
    for name, fn in CALLS:
        third.append((name, FULL))
        if name == 'ks_uniform_host':
            third.append((name, NONE))
        if name == 'chain_diag_host':
            third.append(('rescale_acf_host', NONE))
    order = [(name, FULL) for name, _ in CALLS] + [(name, QUARTER) for name, _ in reversed(CALLS)] + third
    d = p.device(0)
    try:
        for k, (name, i) in enumerate(order):
            got = _flat(calls[name](d, p, i))
            want = alone[(name, id(i))]
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (k, name)
    finally:
        d.close()
