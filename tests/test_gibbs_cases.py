"""tests/gibbs_cases.json kept honest on the CPU (no GPU): every case provably reaches the edge its name and its "hits" state
(from geometry() -- the Python statement of pgl_gibbs_ll_cols' launch arithmetic -- and the reference's currents), a float64
numpy mirror of the regime-split decomposition stays within the sweep's bound on every case, and the bound rejects each
emulated defect of that mirror on the case built for it."""
import numpy as np
import pytest

from tests import gibbs_reference as GR

CASES = GR.load_cases()
BY_NAME = dict((c['name'], c) for c in CASES)
LL_CASES = [c for c in CASES if c['update'] is None]
IDS = [c['name'] for c in CASES]


def _call(c):
    t_lo, t_hi = GR.case_range(c)
    return c['cols'], c['pre'], GR.case_weights(c), t_lo, t_hi


def _x(c):
    return GR.currents(c, *_call(c)).astype(np.float64)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_case_shape_limits(c):
    s = c['problem']
    assert s['nT'] <= 2400 and (s['N'] <= 17 or (s['N'] == 40 and 'xs' in c['hits']))     # one wide population, two launches of it
    w = GR.case_weights(c)
    assert len(np.unique(w)) == w.size                         # every weight of a call distinct: a permuted output moves every entry
    if c['form'] == 'cols':
        assert w.shape[1] <= GR.KMAX


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_excluded_binade_is_empty_and_nothing_overflows(c):
    x = _x(c)
    assert not np.any((x > GR.X_NAN) & (x < GR.X_FLUSH))
    assert np.all(np.isfinite(x)) and np.max(x) < 700.0 * (1 if c['problem']['kind'] == 'exp' else 10)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_case_reaches_its_edge(c):
    p = GR.problem(c)
    R = GR.taps(p)
    assert R == 179                                            # the bin numbers of the table are written for these taps
    t_lo, t_hi = GR.case_range(c)
    nrows = t_hi - t_lo
    hits = dict(c['hits'])
    g = GR.case_geometry(c) if c['form'] == 'cols' else {}
    g1 = GR.case_geometry(c, 1)
    assert g1['path'] == 'f64' and (p.kind == 'exp' or c['form'] != 'cols' or g['path'] == 'regime')
    if p.kind == 'exp':
        assert g['path'] == 'f64' and g['kernels'] == ['k_gibbs_ll_cols', 'k_gibbs_reduce_cols']
    for key in ('nsub', 'ygroups', 'nsplit', 'same_pre', 'nloop', 'nblk', 'sblk'):
        if key in hits:
            assert g[key] == hits.pop(key), key
    if 'CP' in hits or 'gtb' in hits:
        gg = g1 if 'gtb' in hits else g
        for key in ('CP', 'gtb'):
            if key in hits:
                assert gg[key] == hits.pop(key), key
    if 'f64' in hits:
        h = hits.pop('f64')
        assert h.pop('rows_ragged') == (nrows % g1['rows'] != 0)
        for key, v in h.items():
            assert g1[key] == v, key
    if 'ragged' in hits:
        assert hits.pop('ragged') == (nrows % GR.GRB != 0)
    if hits.pop('off_grid', False):
        # pgl_set_time_range refuses a t_lo off the 16-bin tile grid (the sweep asserts the refusal): off the 256 grid, t_hi off both
        assert t_lo % 16 == 0 and t_lo % 256 != 0 and t_hi % 16 != 0 and (t_hi - t_lo) % 256 != 0
    if 'pre_before' in hits:
        n, a, b = hits.pop('pre_before')
        assert a == t_lo - R and b == t_lo and n in c['pre'] and len(GR.events(p, n, a, b)[0]) >= 2
        assert p.S[t_lo - 1, n] > 0                                 # lag 0 into the first bin of the range
    if 'post_edges' in hits:
        n = hits.pop('post_edges')
        assert n in c['cols'] and all(p.S[t, n] > 0 for t in (t_lo - 1, t_lo, t_hi - 1, t_hi))
    if hits.pop('repeated', False):
        assert len(set(zip(c['cols'], c['pre']))) < len(c['cols'])
    if hits.pop('pre_eq_post', False):
        assert c['cols'] == c['pre']
    if 'K' in hits:
        assert len(c['w']) == hits.pop('K')
    if 'xs' in hits:
        assert 16 * -(-p.N // 16) == hits.pop('xs') == 48
        assert {n // 16 for n in c['cols']} == {0, 1, 2}            # columns from all three post tiles
    if 'win' in hits:
        n = hits.pop('win')
        assert n in (GR.GECAP_R, GR.GECAP_R + 1) and GR.window_counts(c, GR.GRB) == n     # the last staged count, the first that is not
        assert not g['same_pre']                                    # the event loop runs, not the filtered train
    if hits.pop('win_over', False):
        assert GR.window_counts(c, GR.GRB) > GR.GECAP_R and not g['same_pre']          # regime path: the global-memory walk
    if 'win_f64' in hits:
        n = hits.pop('win_f64')
        assert GR.window_counts(c, g1['rows']) == n and n in (GR.GECAP, GR.GECAP + 1)
    if 'lags' in hits:
        n, ts = hits.pop('lags')
        assert n in c['pre'] and [t % GR.GRB for t in ts] == [0, GR.GRB - 1]
        for t in ts:
            assert p.S[t - 1, n] > 0 and p.S[t - R, n] > 0 and p.S[t - R - 1, n] > 0     # d = 0, R - 1 and R
        s = GR.events(p, n)[0]
        assert len(s) == 3 * len(ts)
        beta = p.theta[c['cols'][0], 1 + n * p.B:1 + (n + 1) * p.B]
        assert abs(p.ibasis[R - 1].dot(beta)) > 1e-6                 # the last tap carries weight: dropping it shows
    if 'max_ev' in hits:
        assert GR.max_events(c, c['cols'], t_lo, t_hi) == hits.pop('max_ev')
    if 'counts' in hits:
        for n, a, b in hits.pop('counts'):
            assert (n in c['pre'] or n in c['cols']) and np.any(p.S[t_lo:t_hi, n] == a) and np.any(p.S[t_lo:t_hi, n] == b)
    ref = GR.reference(c, *_call(c))
    if 'regime' in hits:
        x = _x(c)
        af = np.abs(x).astype(np.float32)
        r = hits.pop('regime')
        if r == 'pos':
            assert np.all(x >= 12.0) and np.all(af >= 12.0)          # 100 % single-precision regime, above
        elif r == 'neg':
            assert np.all(x <= -12.0) and np.all(af >= 12.0)         # 100 % single-precision regime, below
        elif r == 'band':
            assert np.all(af < 12.0)                                 # 0 %: everything through the f64 queue
        else:
            ncols, _, K = x.shape
            nfull = nrows // 64
            fast = (af >= 12.0)[:, :nfull * 64].reshape(ncols, nfull, 64, K)
            mixed = fast.any(axis=2) & ~fast.all(axis=2)
            assert mixed.mean() > 0.25                                # waves with both regimes among their 64 lanes
            assert np.any(x >= 12.0) and np.any(x <= -12.0)
    if hits.pop('E_zero', False):
        assert np.all(ref[2] == 0.0)
    if 'silent' in hits:
        for n in hits.pop('silent'):
            assert n in c['cols'] and not p.S[:, n].any()
    if hits.pop('silent_neg', False):
        x = _x(c)
        i = c['cols'].index(0)
        assert np.all(x[i] <= -12.0)
        b = GR.bound(ref)[i]
        assert np.all(ref[2][i] > 0.9 * b)                          # E IS the bound here: a total of negligible rates
    if 'careful' in hits:
        want = sorted(map(tuple, hits.pop('careful')))
        assert g['nsplit'] == 1
        ws = GR.case_weights(c)
        got = []
        for i, (n, j) in enumerate(zip(c['cols'], c['pre'])):
            ic = GR.pair_current(c, n, j, np.float64)[t_lo:t_hi]
            x0 = _x(c)[i][:, 0] - ws[i, 0] * ic
            bad = ~(np.max(np.abs(ws[i])) * np.abs(ic) + np.abs(x0) < 699.0)
            assert not np.any(np.abs(np.max(np.abs(ws[i])) * np.abs(ic) + np.abs(x0) - 699.0) < 1e-6)   # no near miss
            got += [(i, sb) for sb in range(g['nsub']) if bad[sb * GR.GRB:(sb + 1) * GR.GRB].any()]
        assert sorted(got) == want and len(want) < len(c['cols']) * g['nsub']
    nan_want = sorted(map(tuple, hits.pop('nan', [])))
    assert sorted(zip(*map(list, np.nonzero(ref[3])))) == nan_want
    if nan_want:
        x = _x(c)
        assert all(np.min(x[i, :, k]) < GR.X_NAN for i, k in nan_want)
    if 'upd_nblk' in hits:
        assert -(-nrows // 1024) == hits.pop('upd_nblk')
        d = c['update']['delta']
        assert len(d) == len(c['cols']) and (len(d) == 1 or 0.0 in d) and max(map(abs, d)) >= 50.0
        assert len(set(c['cols'])) == len(c['cols'])
    if p.kind == 'exp' or c['hits'].get('E_zero'):
        assert np.all(ref[2] == 0.0)
    assert np.all(GR.reference(c, *_call(c), opt_gibbs=1)[2] == 0.0)
    assert not hits, hits                                            # every stated hit has a check above


def test_table_covers_the_issue_list():
    g = dict((c['name'], GR.case_geometry(c)) for c in LL_CASES if c['form'] == 'cols')
    assert {v['nsplit'] for v in g.values() if v['path'] == 'regime'} == {1, 2, 4}
    assert {v['sblk'] for v in g.values() if v['path'] == 'regime'} == {1, 2}
    assert {len(c['cols']) for c in LL_CASES} >= {1, 2, 3, 8, 9, 17}
    assert {len(c['w']) for c in LL_CASES} >= {1, 2, 15, 16, 23}
    assert {c['nloop'] for c in LL_CASES} >= {0, 1, 2, 3, 8, 16}
    assert sorted(c['name'] for c in CASES if c['problem']['N'] > 17) == ['N40_three_tiles', 'update_N40_three_tiles']
    assert {GR.case_range(c)[1] - GR.case_range(c)[0] for c in LL_CASES} >= {37, 256, 257, 768, 1892}
    f = [GR.case_geometry(c, 1) for c in LL_CASES if 'f64' in c['hits']]
    assert {v['gtb'] for v in f} == {32, 64, 256} and {v['TS'] == 1 for v in f} == {True, False}
    assert {v['CP'] for v in f} >= {1, 5, 16, 17} and {v['ygroups'] for v in f} == {1, 2}
    upd = [c for c in CASES if c['update'] is not None]
    assert {len(c['cols']) for c in upd} >= {1, 9, 17}
    assert {GR.case_range(c)[1] - GR.case_range(c)[0] for c in upd} >= {1023, 1024, 1025}


def test_forced_loop_word_is_decoded_as_the_host_does():
    for n in range(1, 17):
        assert GR.dbg_nloop(GR.dbg_word(n)) == n and GR.dbg_word(n) & 0xffff == 0      # clear of the kernels' debug bits
        assert GR.geometry(9, 11, range(9), 1892, 30, 'explinear', opt_dbg=GR.dbg_word(n))['nloop'] == n
    for n in range(1, 16):
        assert GR.dbg_nloop(n << 8) == n
    # the older field is four bits wide: 16 << 8 is the same_pre switch and forces nothing
    g = GR.geometry(9, 11, [4] * 9, 1892, 30, 'explinear', opt_dbg=16 << 8)
    assert GR.dbg_nloop(16 << 8) == 0 and g['nloop'] == 1 and g['nblk'] == 8 and not g['same_pre']
    assert GR.geometry(9, 11, [4] * 9, 1892, 30, 'explinear', opt_dbg=GR.dbg_word(16))['same_pre']
    assert GR.geometry(9, 11, range(9), 1892, 30, 'explinear', opt_dbg=31 << 16)['nloop'] == GR.GNL


WORST = {}


@pytest.mark.parametrize('c', [c for c in LL_CASES if c['problem']['kind'] == 'explinear' and c['form'] == 'cols'],
                         ids=lambda c: c['name'])
def test_regime_split_mirror_is_within_the_bound(c):
    call = _call(c)
    ref = GR.reference(c, *call)
    r = GR.ratio(GR.mirror(c, *call, nloop=c['nloop']), ref)
    WORST[c['name']] = r
    print('mirror ratio %-24s %.3g' % (c['name'], r))
    assert r <= 1.0


@pytest.mark.parametrize('c', LL_CASES, ids=lambda c: c['name'])
def test_f64_mirror_is_within_the_bound(c):
    call = _call(c)
    r = GR.ratio(GR.mirror_f64(c, *call), GR.reference(c, *call, opt_gibbs=1))
    print('f64 mirror ratio %-24s %.3g' % (c['name'], r))
    assert r <= 1.0


REJECTS = {'f32_from_8': 'regime_all_band', 'drop_ragged': 'nrows_257', 'drop_last_lag': 'lags_0_R-1_R', 'drop_21st': 'window_21_events',
           'swap_1_8': 'K_16', 'spikes_from_256': 'post_events_257', 'no_aw': 'ncols_3'}


@pytest.mark.parametrize('defect', GR.DEFECTS)
def test_bound_rejects_defect(defect):
    c = BY_NAME[REJECTS[defect]]
    call = _call(c)
    ref = GR.reference(c, *call)
    assert GR.ratio(GR.mirror(c, *call, nloop=c['nloop']), ref) <= 1.0
    r = GR.ratio(GR.mirror(c, *call, nloop=c['nloop'], defect=defect), ref)
    print('defect %-16s on %-20s ratio %.3g' % (defect, c['name'], r))
    assert r > 1.0


def test_ratio_counts_every_entry():
    c = BY_NAME['nan_column']
    call = _call(c)
    ref = GR.reference(c, *call)
    m = GR.mirror(c, *call)
    assert GR.ratio(m, ref) <= 1.0 and np.isnan(m[0, 0])
    bad = m.copy()
    bad[0, 0] = ref[0][0, 1]                                        # finite where the reference is NaN
    assert GR.ratio(bad, ref) == np.inf
    bad = m.copy()
    bad[1, 1] = np.nan                                              # NaN where the reference is finite
    assert GR.ratio(bad, ref) == np.inf
    assert GR.ratio(m[:, :2], ref) == np.inf


@pytest.mark.parametrize('c', [c for c in CASES if c['update'] is not None], ids=lambda c: c['name'])
def test_update_bound_holds_for_a_float64_update(c):
    """a float64 statement of base + delta ic stays inside updated_currents' bound when the base is its own GX, and inside
    bound + forward_bound against the longdouble GX; a dropped update does neither"""
    d = c['update']['delta']
    GX = GR._xtot(GR._key(c))[1]
    base = GX[:, c['cols']]
    x, bd = GR.updated_currents(c, c['cols'], c['pre'], d, base=base)
    xl, bdl = GR.updated_currents(c, c['cols'], c['pre'], d)
    fwd = GR.forward_bound(c, c['cols'])
    worst = 0.0
    for i, (n, j) in enumerate(zip(c['cols'], c['pre'])):
        got = GX[:, n] + d[i] * GR.pair_current(c, n, j, np.float64)
        assert np.all(np.abs(got - x[:, i]) <= bd[:, i])
        assert np.all(np.abs(got - xl[:, i]) <= bdl[:, i] + fwd[:, i])
        with np.errstate(all='ignore'):
            worst = max(worst, float(np.nanmax(np.abs(got - xl[:, i]).astype(float) / bdl[:, i])))
        if d[i] != 0.0:
            assert np.any(np.abs(GX[:, n] - x[:, i]) > bd[:, i] + fwd[:, i])
    print('float64 update against the longdouble GX, bound without the forward term: ratio %.3g' % worst)
