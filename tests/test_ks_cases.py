"""The case table of the goodness-of-fit sweep (tests/ks_cases.json) reaches what it claims, and its checks hold for the
reference arithmetic and fail for five emulated defects.  No GPU needed.

Per case every tag of its `hits` is checked; over the table every tag of NEEDED is reached.  The numpy mirrors of the kernels
(tests/gof_reference.corr_mirror / ks_mirror, float64) pass the checks of tests/test_gpu_ks.py on every case -- the bound on
tau', the exact statements (an interval between consecutive event bins IS the event term; every sub-range, on the chunk grid
or not, gives the whole range's bits), 1e-14 on D, D+ and D- -- and each wrong mirror fails at least one case: q_k subtracted
from the whole interval, j counted from the time range, ties ranked by `<` in both maxima, padding with 0 instead of +inf,
the tile boundary off by one; and the chunk grid anchored at the start of the range."""
import numpy as np
import pytest

from tests import gof_reference as GR
from tests import rescale_reference as RR

T = GR.load()
L, TILE = GR.L, GR.TILE
SEED = 5
NEEDED_KS = {'n<2', 'pow2', 'padded', 'one-tile', 'full-tile', 'two-tiles', 'three-tiles', 'five-tiles', 'global-step',
             'global-half-cleaner', 'ties', 'clumped', 'tau=0', 'inf', 'void', 'sorted', 'reversed'}
NEEDED_CORR = {'open=0', 'one-edge', 'multi-edge', 'multi-spike', 'q=1e-8', 'q=0.3', 'q=30', 'mid-list', 'on-grid', 'off-grid',
               'mixed-vote', 'regrouped-waves'}
CORR = [(c, lo, hi, hits) for c in T['corr'] for lo, hi, hits in GR.corr_ranges(c)]
LD_IS_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def _ks_holds(tag, c):
    tau, n = GR.ks_tau(c), c['n']
    P = 1
    while P < max(n, 1):
        P <<= 1
    tiles = -(-n // TILE)
    steps = GR.network_steps(P) if n >= 2 else []
    if tag == 'n<2':
        return n < 2
    if tag == 'pow2':
        return n >= 2 and P == n
    if tag == 'padded':
        return n >= 2 and P > n
    if tag == 'full-tile':
        return n == TILE
    if tag.endswith('-tile') or tag.endswith('-tiles'):
        return tiles == {'one': 1, 'two': 2, 'three': 3, 'five': 5}[tag.split('-')[0]]
    if tag == 'global-step':                   # a flip step wider than the tile
        return any(j == 0 and k > TILE for k, j in steps)
    if tag == 'global-half-cleaner':           # and a half-cleaner of stride >= the tile, with a real pair: TILE + stride < n
        return any(j >= TILE and j + TILE < n for k, j in steps)
    if tag == 'ties':
        return n >= 2 and np.unique(tau).size <= n // 2 + 1
    if tag == 'clumped':
        z = -np.expm1(-tau)
        return z.min() >= 1.0 - 1e-12 and np.unique(z).size > 100
    if tag == 'tau=0':
        return np.all(tau == 0.0)
    if tag == 'inf':
        return np.count_nonzero(np.isinf(tau)) == 1 and np.all(tau >= 0)
    if tag == 'void':
        return n >= 2 and np.count_nonzero(~(tau >= 0.0)) == 1
    if tag == 'sorted':
        return np.all(np.diff(tau) > 0)
    if tag == 'reversed':
        return np.all(np.diff(tau) < 0)
    raise AssertionError("unknown tag %r" % tag)


def _pairs(p, n, t_lo, t_hi):
    ev = RR.events(p.S, n, t_lo, t_hi)
    return list(zip(ev[:-1].tolist(), ev[1:].tolist()))


def _corr_holds(tag, c, t_lo, t_hi):
    p = GR.problem(c)
    pairs = [(n, a, b) for n in range(p.N) for a, b in _pairs(p, n, t_lo, t_hi)]
    if tag == 'open=0':
        return any(b == a + 1 for _, a, b in pairs)
    if tag == 'one-edge':
        return any(b // L == a // L + 1 for _, a, b in pairs)
    if tag == 'multi-edge':                    # whole chunks between the two events: their totals enter one by one
        return any(b // L >= a // L + 2 for _, a, b in pairs)
    if tag == 'multi-spike':
        return any(p.S[t_lo + b, n] > 1 for n, a, b in pairs)
    if tag.startswith('q='):
        want = float(tag[2:])
        qs = np.concatenate(GR.corr_reference(c, t_lo, t_hi, SEED, 1)[2])
        return bool(np.any((qs >= want / 2.2) & (qs <= want * 2.2)))
    if tag == 'mid-list':                      # a neuron with intervals in the range and events before it
        return t_lo > 0 and any(GR.first_index(p, n, t_lo) > 0 and len(_pairs(p, n, t_lo, t_hi)) > 0 for n in range(p.N))
    if tag == 'mixed-vote':                    # explinear, a wave of several chunks, and bins where the vote of the wave picks
        # another series than the lane's own current allows, with all three series in use among the lanes
        own = GR.own_class(p.x[t_lo:t_hi])
        return c['kind'] == 'explinear' and RR.xs_of(p.N) < 64 and set(np.unique(own)) == {0, 1, 2} and \
            np.count_nonzero(GR.vote_class(c, t_lo, t_hi) != own) >= 100
    if tag == 'regrouped-waves':               # other chunks share a wave than in the whole range (t_lo // 256 no multiple of the
        # chunks per wave), and the vote falls otherwise on bins of the sub-range
        per_wave = 64 // RR.xs_of(p.N)
        whole = GR.vote_class(c, 0, c['nT'])[t_lo:t_hi]
        return (t_lo // L) % per_wave != 0 and np.count_nonzero(GR.vote_class(c, t_lo, t_hi) != whole) >= 100
    if tag == 'on-grid':
        return t_lo > 0 and t_lo % L == 0
    if tag == 'off-grid':
        return t_lo % L != 0 and t_lo % 16 == 0
    raise AssertionError("unknown tag %r" % tag)


def test_every_case_hits_what_it_claims():
    names = [c['name'] for c in T['ks']] + [c['name'] for c in T['corr']] + [T['multi']['name']]
    assert len(set(names)) == len(names)
    bad = [(c['name'], t) for c in T['ks'] for t in c['hits'] if not _ks_holds(t, c)]
    bad += [(c['name'], (lo, hi), t) for c, lo, hi, hits in CORR for t in hits if not _corr_holds(t, c, lo, hi)]
    assert not bad, "claimed but not reached: %s" % bad
    assert NEEDED_KS <= set(t for c in T['ks'] for t in c['hits'])
    assert NEEDED_CORR <= set(t for _, _, _, hits in CORR for t in hits)
    assert sorted(c['n'] for c in T['ks'] if c['content'] == 'uniform') == [0, 1, 2, 3, 4095, 4096, 4097, 8192, 8193, 20000]
    assert set(c['content'] for c in T['ks']) == {'uniform', 'equal', 'half_tied', 'clumped', 'zero', 'one_inf', 'one_nan',
                                                  'one_negative', 'sorted', 'reversed'}
    for c in T['corr']:
        assert c['N'] <= 8 and c['nT'] <= 2048
        for lo, hi, _ in GR.corr_ranges(c):
            assert 0 <= lo < hi <= c['nT'] and lo % 16 == 0
    tau, off = GR.multi()
    lens = np.diff(off)
    assert lens.size == 300 and off[-1] == tau.size
    full = np.flatnonzero(lens >= 2)
    assert np.any(lens[full[:-1] + 1] == 0) and np.any(lens[1:][lens[:-1] == 0] >= 2)      # empty ones between full ones
    assert {0, 1, 2, 3, TILE, TILE + 1} <= set(lens.tolist())


def _ks_passes(tau, got):
    """the checks of tests/test_gpu_ks.py on (D, D+, D-, n, zsorted)"""
    ref = GR.ks_reference(tau)
    if np.isnan(ref[0]):
        return bool(np.all(np.isnan(got[:3])) and got[3] == tau.size)
    z = got[4]
    zn = np.sort(-np.expm1(-tau))
    if not (got[3] == tau.size and np.all(np.diff(z) >= 0) and np.all(np.abs(z - zn) <= 2 * np.spacing(zn))):
        return False
    return bool(np.max(np.abs(np.array(got[:3]) - ref[:3])) <= GR.KS_TOL)


@pytest.mark.skipif(not LD_IS_WIDER, reason="numpy.longdouble is float64 here")
def test_ks_mirror_passes_and_every_fault_fails_somewhere():
    caught = dict((f, []) for f in GR.KS_FAULTS)
    for c in T['ks']:
        tau = GR.ks_tau(c)
        got = GR.ks_mirror(tau)
        assert _ks_passes(tau, got), c['name']
        if c['n'] >= 2 and np.all(tau >= 0):
            assert np.array_equal(got[4], np.sort(-np.expm1(-tau))), c['name']         # the network sorts
            from theano_pyglm_amd.inference import gof
            assert got[0] == gof.ks_uniform(-np.expm1(-tau)), c['name']                # and the maxima are numpy's, bit for bit
        for f in GR.KS_FAULTS:
            if not _ks_passes(tau, GR.ks_mirror(tau, f)):
                caught[f].append(c['name'])
    print(caught)
    for f in GR.KS_FAULTS:
        assert caught[f], "no case notices the fault %r" % f
    assert {'all_equal', 'half_tied', 'all_zero'} <= set(caught['tie_lt'])
    assert {'three', 'n4095', 'n4097', 'n8193', 'n20000'} <= set(caught['pad_zero']) and 'n4096' not in caught['pad_zero']
    assert {'n4097', 'n8192', 'n8193', 'n20000'} <= set(caught['tile_edge'])
    assert not {'n4095', 'n4096'} & set(caught['tile_edge'])                           # one tile cannot see that one


def _corr_passes(c, t_lo, t_hi, hits, fault, whole):
    """the checks on a mirror of the corrected intervals: the bound; open = 0 exactly; the whole range's bits in a sub-range"""
    p = GR.problem(c)
    ref = GR.corr_reference(c, t_lo, t_hi, SEED, 1)
    tau, off = GR.corr_mirror(c, t_lo, t_hi, SEED, 1, fault)
    ok = np.array_equal(off, RR.offsets(ref[0])) and GR.corr_ratio(tau, off, ref) <= 1.0
    from oracle import glm_oracle as O
    for n in range(p.N):
        j0 = GR.first_index(p, n, t_lo)
        for i, (a, b) in enumerate(_pairs(p, n, t_lo, t_hi)):
            if b == a + 1:
                e = -np.log1p(GR.uniform(SEED, 1, n, j0 + i + 1) * np.expm1(-(p.dt * O.nlin(p.x[t_lo + b, n], p.kind))))
                ok = ok and tau[off[n] + i] == e
        if whole is not None:                  # any sub-range, on the chunk grid or not: the whole range's bits
            k = int(off[n + 1] - off[n])
            ok = ok and np.array_equal(whole[0][whole[1][n] + j0:whole[1][n] + j0 + k], tau[off[n]:off[n + 1]])
    return bool(ok), (tau, off)


@pytest.mark.skipif(not LD_IS_WIDER, reason="numpy.longdouble is float64 here")
def test_corr_mirror_passes_and_every_fault_fails_somewhere():
    caught = dict((f, []) for f in GR.CORR_FAULTS)
    whole = {}
    for c, t_lo, t_hi, hits in CORR:
        ok, got = _corr_passes(c, t_lo, t_hi, hits, None, whole.get(c['name']))
        ref = GR.corr_reference(c, t_lo, t_hi, SEED, 1)
        print("%-12s [%4d, %4d): float64 mirror %.2e of the bound, %d intervals" % (c['name'], t_lo, t_hi, GR.corr_ratio(*got, ref), got[1][-1]))
        assert ok, (c['name'], t_lo)
        whole.setdefault(c['name'], got)
        for f in GR.CORR_FAULTS:
            if not _corr_passes(c, t_lo, t_hi, hits, f, whole[c['name']])[0]:
                caught[f].append((c['name'], t_lo))
    print(caught)
    for f in GR.CORR_FAULTS:
        assert caught[f], "no case notices the fault %r" % f
    assert all(lo > 0 for _, lo in caught['j_from_range'])                             # the whole range cannot see that one
    assert ('exp_q', 0) in caught['sub_q']                                             # consecutive event bins: open = 0 exactly
    assert caught['grid_from_range'] and all(lo % L != 0 for _, lo in caught['grid_from_range'])   # ranges that start mid-chunk
    # draw 0 and draw 1 differ, and the uncorrected interval bounds the corrected one
    c = T['corr'][0]
    a, b = GR.corr_reference(c, 0, c['nT'], SEED, 0), GR.corr_reference(c, 0, c['nT'], SEED, 1)
    assert all(np.all(x != y) for x, y in zip(a[0], b[0]))
    assert all(np.all(t <= o + q) and np.all(t > o) for t, o, q in zip(a[0], a[1], a[2]))


def test_dry_run_names_the_corrected_launches():
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    fwd = _lib.plan_kernels(8, B=5, R=200, nT=5000, path=2)
    assert _lib.plan_kernels(8, B=5, R=200, nT=5000, path=9) == fwd + ['k_rcorr_chunk<0>', 'k_rescale_scan', 'k_rcorr_finish']
    assert _lib.plan_kernels(8, B=5, R=200, nT=5000, path=6) == fwd + ['k_rescale_chunk<0>', 'k_rescale_scan', 'k_rescale_finish']
