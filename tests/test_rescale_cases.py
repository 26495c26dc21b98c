"""The case table of the time-rescaling sweep (tests/rescale_cases.json) reaches what it claims, and the sweep's bound holds
for the reference arithmetic and fails for four emulated defects.  No GPU needed: the geometry k_rescale_chunk / _scan /
_finish derive from a time range (256-bin chunks from t_lo, 64 scan segments of `per` chunks, 8 rows in flight, a 256-thread
stride over a neuron's events), the spike arrays and the reference currents of the cases.

Per (case, range) every tag of its `hits` is checked; over the table every tag of NEEDED is reached.  The numpy mirror of
the kernels' decomposition (tests/rescale_reference.mirror, float64) stays inside the GPU test's bound on every case, and
each of its faults -- the cum term dropped, a segment's write-back started one chunk late, the tail mask dropped, the stride
loop cut after one trip -- leaves that bound on at least one case: the bound is checked against the reference arithmetic,
not against the kernel.  tests/test_gpu_rescale_sweep.py runs every case on the device."""
import numpy as np
import pytest

from oracle import glm_oracle as O
from tests import hvp_reference as R
from tests import rescale_reference as RR

L, SEGS = RR.L, RR.SEGS
MARGIN = 0.5
NEEDED = {'single-short-chunk', 'single-full-chunk', 'exact-multiple', 'ragged-tail', 'event-on-first-bin', 'event-on-last-bin',
          'events-on-chunk-edge', 'events-behind-t_hi', 'odd-tile-start', 'per=1', 'per=2', 'per=3', 'empty-segments',
          'full-64-segments', 'gap>=2', 'gaps-1-2-3', 'gap-crosses-segment', 'gap-first-to-last', 'dense', 'two-spike-bins',
          'N=1', 'N=16', 'N=17', 'xs=48', 'N>64', 'regime-tail+', 'regime-tail-', 'regime-mid', 'regime-small', 'regime-mixed',
          'exp'}
CASES = RR.load_cases()
RANGES = [(c, lo, hi, hits) for c in CASES for lo, hi, hits in RR.ranges(c)]


def _pairs(S, n, t_lo, t_hi):
    """(ca, cb) of every interval of neuron n: the chunks of consecutive events"""
    ch = RR.events(S, n, t_lo, t_hi) // L
    return list(zip(ch[:-1].tolist(), ch[1:].tolist()))


def _all_pairs(S, t_lo, t_hi):
    return [(n, ca, cb) for n in range(S.shape[1]) for ca, cb in _pairs(S, n, t_lo, t_hi)]


def _alone(c, n):
    """neuron n's column holds its planted events only"""
    return any(e['n'] == n and not e.get('keep') for e in c['plant'])


def _regime(c, t_lo, t_hi):
    """|bias + x| over the range and |bias| itself (the rows past the end), per neuron: (min, max, sign or 0)"""
    p = RR.problem(c)
    x = np.vstack((RR.currents(c, t_lo, t_hi), p.theta[:, 0][None, :]))
    sign = np.where(np.all(x > 0, axis=0), 1, np.where(np.all(x < 0, axis=0), -1, 0))
    return np.abs(x).min(axis=0), np.abs(x).max(axis=0), sign


def _class(lo, hi):
    """'tail' / 'mid' / 'small' where a neuron's |x| clears the vote thresholds by MARGIN, else None"""
    if lo >= RR.VOTE_TAIL + MARGIN:
        return 'tail'
    if lo >= RR.VOTE_MID + MARGIN and hi <= RR.VOTE_TAIL - MARGIN:
        return 'mid'
    if hi <= RR.VOTE_MID - MARGIN:
        return 'small'
    return None


def _holds(tag, c, t_lo, t_hi):
    p = RR.problem(c)
    S, N = p.S, c['N']
    nchunks, per, live, last = RR.geometry(t_lo, t_hi)
    n = t_hi - t_lo
    if tag == 'single-short-chunk':
        return nchunks == 1 and n < L
    if tag == 'single-full-chunk':
        return nchunks == 1 and n == L
    if tag == 'exact-multiple':                # the event lookup at t_hi enters through the recording's last 16-bin tile
        return n % L == 0 and t_hi % 16 == 0 and t_hi == c['nT']
    if tag == 'ragged-tail':
        return last % RR.UNROLL != 0
    if tag == 'event-on-first-bin':
        return bool(S[t_lo].any())
    if tag == 'event-on-last-bin':
        return bool(S[t_hi - 1].any())
    if tag == 'events-on-chunk-edge':
        edges = np.arange(t_lo + L, t_hi, L)
        return bool(np.any((S[edges - 1] > 0) & (S[edges] > 0)))
    if tag == 'events-behind-t_hi':            # counted: the event on t_hi - 1; not counted: the events on t_hi and t_hi + 1
        ok = False
        for m in range(N):
            if _alone(c, m) and S[t_hi - 1, m] and S[t_hi, m] and S[t_hi + 1, m]:
                taus, stats = RR.reference(c, t_lo, t_hi)
                inside = int(np.count_nonzero(S[t_lo:t_hi, m]))
                ok = stats[m, 1] == inside and taus[m].size == inside - 1 and inside >= 2 and \
                    np.count_nonzero(S[t_lo:, m]) == inside + 2
        return ok
    if tag == 'odd-tile-start':
        return t_lo % 16 == 0 and (t_lo // 16) % 2 == 1
    if tag.startswith('per='):
        return per == int(tag[4:])
    if tag == 'empty-segments':
        return live < SEGS
    if tag == 'full-64-segments':
        return live == SEGS and nchunks == SEGS
    if tag == 'gap>=2':
        return any(cb - ca >= 2 for _, ca, cb in _all_pairs(S, t_lo, t_hi))
    if tag == 'gaps-1-2-3':                    # of a neuron whose events are alone in its column
        return any(_alone(c, m) and {1, 2, 3} <= set(cb - ca for ca, cb in _pairs(S, m, t_lo, t_hi)) for m in range(N))
    if tag == 'gap-crosses-segment':           # cum[cb] - cum[ca + 1] with the two rows written by different segments
        return any(cb - ca >= 2 and cb // per != (ca + 1) // per for _, ca, cb in _all_pairs(S, t_lo, t_hi))
    if tag == 'gap-first-to-last':
        return any(_alone(c, m) and _pairs(S, m, t_lo, t_hi) == [(0, nchunks - 1)] for m in range(N)) and nchunks >= 3
    if tag == 'dense':                         # > 1024 events (five trips of the 256-thread stride), two whole chunks of events
        for m in range(N):
            ev = S[t_lo:t_hi, m] > 0
            full = [k for k in range(nchunks - 1) if ev[k * L:(k + 1) * L].all()]
            if ev.sum() > 1024 and len(full) >= 2 and np.any(S[t_lo:t_hi, m][full[0] * L:(full[0] + 1) * L] > 1):
                others = [int((S[t_lo:t_hi, k] > 0).sum()) for k in range(N) if k != m]
                return max(others) > 256       # and a neuron of the background with a second trip
        return False
    if tag == 'two-spike-bins':
        return bool(np.any(S[t_lo:t_hi] > 1))
    if tag in ('N=1', 'N=16', 'N=17'):
        return N == int(tag[2:])
    if tag == 'xs=48':
        return RR.xs_of(N) == 48 and L % 48 != 0
    if tag == 'N>64':
        return N > 64 and RR.xs_of(N) // 16 >= 5
    if tag == 'exp':
        b = p.theta[:, 0]
        return c['kind'] == 'exp' and b.min() <= -19.0 and b.max() >= 7.0 and np.all(np.diff(np.sort(b)) < 2.5)
    if tag.startswith('regime-'):
        if not (c['kind'] == 'explinear' and N == 16 and RR.xs_of(N) == N):      # every lane of every wave holds a neuron
            return False
        lo, hi, sign = _regime(c, t_lo, t_hi)
        cls = [_class(a, b) for a, b in zip(lo, hi)]
        if tag == 'regime-tail+':
            return all(k == 'tail' for k in cls) and np.all(sign == 1)
        if tag == 'regime-tail-':
            return all(k == 'tail' for k in cls) and np.all(sign == -1)
        if tag == 'regime-mid':
            return all(k == 'mid' for k in cls) and np.any(sign == 1) and np.any(sign == -1)
        if tag == 'regime-small':
            return all(k == 'small' for k in cls) and np.any(RR.currents(c, t_lo, t_hi) > 0) and \
                np.any(RR.currents(c, t_lo, t_hi) < 0)
        if tag == 'regime-mixed':              # every neuron inside one regime, no two neighbours in the same
            return None not in cls and {'tail', 'mid', 'small'} <= set(cls) and \
                all(cls[i] != cls[i + 1] for i in range(N - 1)) and np.any(sign == 1) and np.any(sign == -1)
    raise AssertionError("unknown tag %r" % tag)


def test_case_table_is_well_formed():
    assert len(set(c['name'] for c in CASES)) == len(CASES)
    for c, t_lo, t_hi, hits in RANGES:
        assert 0 <= t_lo < t_hi <= c['nT'] and t_lo % 16 == 0, c['name']
        assert c['kind'] in ('explinear', 'exp') and c['nT'] * c['N'] <= 33000 * 70, c['name']
        x = RR.currents(c)
        assert np.all(np.abs(x) <= 600.0), c['name']                   # nothing denormal: the relative bound means something
        assert RR.xs_of(c['N']) % 16 == 0 and 0 <= RR.xs_of(c['N']) - c['N'] < 16


def test_every_range_hits_what_it_claims():
    bad = [(c['name'], (t_lo, t_hi), t) for c, t_lo, t_hi, hits in RANGES for t in hits if not _holds(t, c, t_lo, t_hi)]
    assert not bad, "claimed but not reached: %s" % bad
    reached = set(t for _, _, _, hits in RANGES for t in hits)
    assert NEEDED <= reached, "no case for: %s" % sorted(NEEDED - reached)
    for c, t_lo, t_hi, hits in RANGES:
        nchunks, per, live, last = RR.geometry(t_lo, t_hi)
        S = RR.problem(c).S
        far = sorted(set((ca, cb) for _, ca, cb in _all_pairs(S, t_lo, t_hi) if cb - ca >= 2))
        ev = np.count_nonzero(S[t_lo:t_hi], axis=0)
        print("%-17s [%5d, %5d): %3d chunks, per %d, %2d live segments, last chunk %3d bins (%% 8 = %d), xs %d (256 %% xs = %d), "
              "events per neuron %d..%d, %d kinds of (ca, cb) with cb - ca >= 2"
              % (c['name'], t_lo, t_hi, nchunks, per, live, last, last % 8, RR.xs_of(c['N']), L % RR.xs_of(c['N']),
                 ev.min(), ev.max(), len(far)))


def test_the_scan_cases_hold_the_planted_neurons():
    """scan_per2: 65 chunks + 3 bins = 66 chunks, per 2, 33 live segments; scan_64: 64 chunks; scan_per3: 129 chunks, per 3;
    each with the isolated long-gap neurons, the dense neuron and the first-to-last interval."""
    geo = {'scan_per2': (66, 2, 33), 'scan_64': (64, 1, 64), 'scan_per3': (129, 3, 43)}
    for name, want in geo.items():
        c = [c for c in CASES if c['name'] == name][0]
        assert RR.geometry(0, c['nT'])[:3] == want, name
        hits = RR.ranges(c)[0][2]
        assert {'gaps-1-2-3', 'gap-crosses-segment', 'gap-first-to-last', 'dense', 'two-spike-bins'} <= set(hits), name
    c = [c for c in CASES if c['name'] == 'scan_per2'][0]
    assert c['nT'] == 65 * L + 3 and SEGS - 33 == 31


def test_reference_rate_equals_the_oracles():
    """oracle.glm_oracle.nlin against the longdouble rate of the reference on every case's currents: 1e-13 relative."""
    for c in CASES:
        x = RR.currents(c)
        ref = RR.rate_longdouble(x, c['kind'])
        err = float(np.max(np.abs(O.nlin(x, c['kind']) - ref) / ref))
        print("%-17s max relative difference %.2e" % (c['name'], err))
        assert err <= 1e-13, c['name']


def test_currents_are_the_feature_rows_of_the_gof_test():
    c = [c for c in CASES if c['name'] == 'n17'][0]
    p = RR.problem(c)
    x = RR.currents(c)
    for n in (0, 16):
        xr = R.feature_rows(p.fS, p.fstim, p.Weff[:, n], 0, p.nT).dot(p.theta[n])
        assert np.max(np.abs(x[:, n] - xr)) <= 1e-13 * np.max(np.abs(xr))
    assert np.std(x[:, 0]) > 0


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps, reason="numpy.longdouble is float64 here")
def test_mirror_meets_the_bound_and_every_fault_leaves_it():
    caught = dict((f, []) for f in RR.FAULTS)
    for c, t_lo, t_hi, hits in RANGES:
        ref = RR.reference(c, t_lo, t_hi)
        tau, off, lam = RR.mirror(c, t_lo, t_hi)
        assert np.array_equal(off, RR.offsets(ref[0]))
        rt, rl = RR.ratios(tau, off, lam, ref)
        print("%-17s [%5d, %5d): float64 mirror %.2e of the tau bound, %.2e of the Lambda bound" % (c['name'], t_lo, t_hi, rt, rl))
        assert rt <= 1.0 and rl <= 1.0, (c['name'], rt, rl)
        for f in RR.FAULTS:
            ft, fl = RR.ratios(*RR.mirror(c, t_lo, t_hi, f), ref)
            if ft > 1.0 or fl > 1.0:
                caught[f].append((c['name'], t_lo, 'tau' if ft > 1.0 else 'Lambda'))
    for f in RR.FAULTS:
        print(f, caught[f])
        assert caught[f], "no case notices the fault %r" % f
    names = lambda f, what: set(n for n, _, w in caught[f] if w == what)
    # the defects the issue names are caught where the table says so
    assert {'scan_per2', 'scan_per3'} <= names('scan_late', 'tau')           # interior rows of cum, per >= 2
    assert {'scan_per2', 'scan_64', 'scan_per3', 'n16', 'tail_neg'} <= names('no_cum', 'tau')
    assert {'scan_per2', 'scan_64', 'scan_per3'} <= names('stride_once', 'tau')
    assert {'one_short_chunk', 'ragged_tail', 'n1', 'mid_both_signs'} <= names('no_tail_mask', 'Lambda')
    assert 'exact_chunks' not in names('no_tail_mask', 'Lambda')           # a last chunk of 8 k bins cannot see that one


def test_dry_run_names_the_three_launches():
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    for c in CASES:
        names = _lib.plan_kernels(c['N'], B=5, R=32, Dstim=0, nT=c['nT'], n_lo=0, count=c['N'], path=6)
        assert names[-3:] == ['k_rescale_chunk<0>', 'k_rescale_scan', 'k_rescale_finish'], (c['name'], names)
        assert not any(n.startswith('k_rescale') for n in names[:-3])
