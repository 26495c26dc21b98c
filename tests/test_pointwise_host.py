"""The pointwise log-likelihood path without a GPU: the case table of the sweep (tests/pointwise_cases.json) reaches what it
claims; the sweep's bound holds for a float64 numpy mirror of the chunk -> block decomposition and fails for three emulated
defects of it (tail rows not masked, the last short block dropped, blocks cut on the grid from bin 0 when t_lo > 0); the
accumulation rule of csrc/pglm_pointwise.h, built for the host, agrees with longdouble numpy on random and adversarial
sequences; the two WAIC routes of inference/model_compare.py are the same algebra and reach the closed form of Gaussian
terms; the draws of the GPU accumulator test spread enough for its M2 bound."""
import numpy as np
import pytest

from tests import pointwise_reference as PR
from tests import rescale_reference as RR
from theano_pyglm_amd.inference import model_compare as MC

L = PR.L
MARGIN = 0.5
NEEDED = {'single-short-chunk', 'exact-multiple', 'events-on-chunk-edge', 'ragged-tail', 't_lo-off-chunk-grid',
          'events-behind-t_hi', 'bc=1', 'bc=2-short-last', 'bc=3-short-last', 'single-block', 'silent', 'dense-3',
          'N=1', 'N=16', 'N=17', 'xs=48', 'N>64', 'regime-tail+', 'regime-tail-', 'regime-mid', 'regime-small', 'regime-mixed',
          'exp'}
CASES = PR.load_cases()
RANGES = [(c, lo, hi, bcs, hits) for c in CASES for lo, hi, bcs, hits in PR.ranges(c)]
longdouble = pytest.mark.skipif(np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps,
                                reason="numpy.longdouble is float64 here")


def _class(lo, hi):
    if lo >= RR.VOTE_TAIL + MARGIN:
        return 'tail'
    if lo >= RR.VOTE_MID + MARGIN and hi <= RR.VOTE_TAIL - MARGIN:
        return 'mid'
    if hi <= RR.VOTE_MID - MARGIN:
        return 'small'
    return None


def _holds(tag, c, t_lo, t_hi, bcs):
    p = PR.problem(c)
    S, N = p.S, c['N']
    n = t_hi - t_lo
    nchunks, _, last = PR.geometry(t_lo, t_hi, 1)
    if tag == 'single-short-chunk':
        return nchunks == 1 and n < L
    if tag == 'exact-multiple':
        return n % L == 0 and nchunks > 1
    if tag == 'events-on-chunk-edge':
        edges = np.arange(t_lo + L, t_hi, L)
        return bool(np.all(np.any((S[edges - 1] > 0) & (S[edges] > 0), axis=1)))
    if tag == 'ragged-tail':
        return last % PR.UNROLL != 0
    if tag == 't_lo-off-chunk-grid':
        return t_lo % 16 == 0 and t_lo % L != 0
    if tag == 'events-behind-t_hi':
        return any(S[t_hi - 1, m] and S[t_hi, m] and S[t_hi + 1, m] for m in range(N))
    if tag == 'bc=1':
        return 1 in bcs and nchunks > 1
    if tag in ('bc=2-short-last', 'bc=3-short-last'):
        k = int(tag[3])
        return k in bcs and nchunks > k and nchunks % k != 0
    if tag == 'single-block':
        return any(b >= nchunks for b in bcs)
    if tag == 'silent':
        return bool(np.any(S[t_lo:t_hi].sum(axis=0) == 0))
    if tag == 'dense-3':
        return any(np.all(S[t_lo + 300:t_lo + 900, m] > 0) and S[t_lo:t_hi, m].max() == 3 for m in range(N))
    if tag in ('N=1', 'N=16', 'N=17'):
        return N == int(tag[2:])
    if tag == 'xs=48':
        return RR.xs_of(N) == 48
    if tag == 'N>64':
        return N > 64 and RR.xs_of(N) // 16 >= 5
    if tag == 'exp':
        b = p.theta[:, 0]
        return c['kind'] == 'exp' and b.min() <= -19.0 and b.max() >= 7.0
    if tag.startswith('regime-'):
        if not (c['kind'] == 'explinear' and N == 16):
            return False
        x = np.vstack((PR.currents(c, t_lo, t_hi), p.theta[:, 0][None, :]))       # (the rows past the end run at the bias)
        sign = np.where(np.all(x > 0, axis=0), 1, np.where(np.all(x < 0, axis=0), -1, 0))
        cls = [_class(a, b) for a, b in zip(np.abs(x).min(axis=0), np.abs(x).max(axis=0))]
        if tag == 'regime-tail+':
            return all(k == 'tail' for k in cls) and np.all(sign == 1)
        if tag == 'regime-tail-':
            return all(k == 'tail' for k in cls) and np.all(sign == -1)
        if tag == 'regime-mid':
            return all(k == 'mid' for k in cls) and np.any(sign == 1) and np.any(sign == -1)
        if tag == 'regime-small':
            return all(k == 'small' for k in cls) and np.any(x > 0) and np.any(x < 0)
        if tag == 'regime-mixed':
            return None not in cls and {'tail', 'mid', 'small'} <= set(cls) and \
                all(cls[i] != cls[i + 1] for i in range(N - 1)) and np.any(sign == 1) and np.any(sign == -1)
    raise AssertionError("unknown tag %r" % tag)


def test_case_table_is_well_formed_and_hits_what_it_claims():
    assert len(set(c['name'] for c in CASES)) == len(CASES)
    for c, t_lo, t_hi, bcs, hits in RANGES:
        assert 0 <= t_lo < t_hi <= c['nT'] and t_lo % 16 == 0, c['name']
        assert c['kind'] in ('explinear', 'exp') and c['nT'] * c['N'] <= 1600 * 70, c['name']      # (quick on the device)
        assert all(b >= 1 for b in bcs) and bcs == sorted(set(bcs))
        assert np.all(np.abs(PR.currents(c)) <= 600.0), c['name']
    bad = [(c['name'], (t_lo, t_hi), t) for c, t_lo, t_hi, bcs, hits in RANGES for t in hits if not _holds(t, c, t_lo, t_hi, bcs)]
    assert not bad, "claimed but not reached: %s" % bad
    reached = set(t for _, _, _, _, hits in RANGES for t in hits)
    assert NEEDED <= reached, "no case for: %s" % sorted(NEEDED - reached)
    assert any(PR.problem(c).S.max() == 3 for c in CASES)


def test_block_sums_of_the_reference_add_up():
    """the blocks of every block length partition the range: their sums agree with the one-block sum"""
    for c, t_lo, t_hi, bcs, hits in RANGES:
        nchunks = PR.geometry(t_lo, t_hi, 1)[0]
        whole = PR.reference(c, t_lo, t_hi, nchunks)
        assert whole[0].shape == (1, c['N'])
        for bc in bcs:
            ll, A = PR.reference(c, t_lo, t_hi, bc)
            assert ll.shape == (PR.geometry(t_lo, t_hi, bc)[1], c['N'])
            assert np.all(np.abs(ll.sum(axis=0) - whole[0][0]) <= 1e-13 * whole[1][0]), (c['name'], bc)
            assert np.all(np.abs(ll) <= A * (1 + 1e-15))


@longdouble
def test_mirror_meets_the_bound_and_every_fault_leaves_it():
    caught = dict((f, []) for f in PR.FAULTS)
    for c, t_lo, t_hi, bcs, hits in RANGES:
        for bc in bcs:
            ref = PR.reference(c, t_lo, t_hi, bc)
            r = PR.ratio(PR.mirror(c, t_lo, t_hi, bc), ref)
            print("%-17s [%5d, %5d) block_chunks %2d: float64 mirror %.2e of the bound" % (c['name'], t_lo, t_hi, bc, r))
            assert r <= 1.0, (c['name'], bc, r)
            for f in PR.FAULTS:
                if PR.ratio(PR.mirror(c, t_lo, t_hi, bc, f), ref) > 1.0:
                    caught[f].append((c['name'], t_lo, bc))
    for f in PR.FAULTS:
        print(f, caught[f])
        assert caught[f], "no case notices the fault %r" % f
    names = lambda f: set(n for n, _, _ in caught[f])
    assert {'one_short_chunk', 'ragged_tail', 'n1', 'mid_both_signs'} <= names('no_tail_mask')
    assert 'exact_chunks' not in names('no_tail_mask')                     # a last chunk of 8 k bins cannot see that one
    assert {'exact_chunks', 'ragged_tail', 'n17', 'tail_neg'} <= names('drop_short_block')
    assert all(bc > 1 for _, _, bc in caught['drop_short_block'])
    assert set((n, lo) for n, lo, _ in caught['grid_from_zero']) == {('ragged_tail', 1616)}
    assert set(bc for _, _, bc in caught['grid_from_zero']) == {1, 2}      # (one block holds the range on either grid)


def test_dry_run_names_the_two_launches():
    import __graft_entry__ as ge
    ge.build_hip()
    from theano_pyglm_amd import _lib
    for c in CASES:
        names = _lib.plan_kernels(c['N'], B=5, R=32, Dstim=0, nT=c['nT'], n_lo=0, count=c['N'], path=7)
        assert names[-2:] == ['k_pw_chunk<0>', 'k_pw_block'], (c['name'], names)
        assert names[:-2] == _lib.plan_kernels(c['N'], B=5, R=32, Dstim=0, nT=c['nT'], n_lo=0, count=c['N'], path=2)


# ---- the accumulation rule -----------------------------------------------------------------------------------------------
def _check_state(ll, rel=1e-12):
    """m exact, e in [1, S], m + log e and the mean to 1e-12 relative.  M2: a Welford step forms d = l - mean and
    d (l - mean') from operands of size max |l|, so each carries an absolute error of a few u max|l| |d|; over the draws
    that is at most  4 u max|l| sum_s |d_s| <= 4 u max|l| sqrt(S M2), next to 64 S u M2 for the additions themselves."""
    S = ll.shape[0]
    u = np.finfo(np.float64).eps / 2
    acc = PR.host_accumulate(ll)
    lse, mean, m2 = PR.accumulate_longdouble(ll)
    bad = np.isnan(np.asarray(lse, dtype=float))
    assert np.array_equal(np.isnan(acc), np.broadcast_to(bad, acc.shape))
    ok = ~bad
    got = acc[0] + np.log(acc[1])
    assert np.all(acc[0][ok] == ll[:, ok].max(axis=0))
    assert np.all((acc[1][ok] >= 1.0) & (acc[1][ok] <= S))
    assert np.all(np.abs(got[ok] - lse[ok]) <= rel * np.abs(lse[ok]))
    assert np.all(np.abs(acc[2][ok] - mean[ok]) <= rel * np.abs(mean[ok]) + 1e-300)
    big = np.abs(ll[:, ok]).max(axis=0)
    m2f = np.asarray(m2[ok], dtype=float)
    assert np.all(np.abs(acc[3][ok] - m2[ok]) <= 64 * S * u * m2f + 4 * u * big * np.sqrt(S * m2f))
    return acc


@longdouble
def test_accumulator_against_longdouble_numpy():
    rng = np.random.default_rng(11)
    # random: terms of the size the blocks have, spread over draws from 1e-3 to 1 of the mean
    mu = -np.exp(rng.uniform(0.0, 8.0, size=(5, 7)))
    ll = mu[None] * (1.0 + np.exp(rng.uniform(np.log(1e-3), 0.0, size=(5, 7)))[None] * rng.standard_normal((200, 5, 7)))
    _check_state(ll)
    # a new maximum at every draw: e is rescaled every time; far steps underflow the old sum to 0
    up = np.cumsum(np.abs(rng.standard_normal((64, 6))) * np.array([1e-3, 1.0, 30.0, 800.0, 1e-9, 5.0]), axis=0) - 1000.0
    acc = _check_state(up)
    assert np.all(acc[0] == up[-1])
    assert acc[1][3] == 1.0                                       # steps of ~800: exp(-800) = 0, the newest term alone
    # the same values in falling order: the maximum never moves
    acc = _check_state(up[::-1].copy())
    assert np.all(acc[0] == up[-1])
    # equal values: e = S exactly, M2 = 0 exactly
    eq = np.full((33, 4), -123.456)
    acc = PR.host_accumulate(eq)
    assert np.all(acc[0] == -123.456) and np.all(acc[1] == 33.0) and np.all(acc[2] == -123.456) and np.all(acc[3] == 0.0)
    # one NaN (and one -inf, one +inf): that element's state is NaN from there on, the others are untouched
    ll = rng.standard_normal((20, 5)) - 50.0
    clean = PR.host_accumulate(ll)
    ll2 = ll.copy()
    ll2[7, 1], ll2[0, 2], ll2[19, 3] = np.nan, -np.inf, np.inf
    acc = _check_state(ll2)
    assert np.all(np.isnan(acc[:, 1:4])) and np.array_equal(acc[:, [0, 4]], clean[:, [0, 4]])
    # draw 0 initialises: the state before it does not matter
    assert np.array_equal(PR.host_accumulate(ll, garbage=True), PR.host_accumulate(ll, garbage=False))
    # folding one draw at a time is the run
    st = np.full((4, 5), 7.0)
    for s in range(20):
        PR.lib().pw_fold(np.ascontiguousarray(ll[s]).ctypes.data, 5, s, st.ctypes.data)
    assert np.array_equal(st, clean)


# ---- WAIC ----------------------------------------------------------------------------------------------------------------
def test_waic_from_accumulators_is_waic_from_pointwise():
    rng = np.random.default_rng(5)
    ll = -40.0 + 3.0 * rng.standard_normal((1, 9, 4)) + np.array([0.01, 0.3, 1.0, 2.0]) * rng.standard_normal((257, 9, 4))
    a = MC.waic_from_accumulators(PR.host_accumulate(ll), ll.shape[0])
    b = MC.waic_from_pointwise(ll)
    for k in ('elpd_waic', 'p_waic', 'lppd', 'waic', 'se'):
        assert np.all(np.abs(a[k] - b[k]) <= 1e-11 * np.abs(b[k])), k
    assert np.array_equal(a['n_high_var'], b['n_high_var']) and a['n_blocks'] == b['n_blocks'] == 9
    assert a['n_high_var'][0] == 0 and a['n_high_var'][3] == 9
    assert np.allclose(a['waic'], -2.0 * (a['lppd'] - a['p_waic']), rtol=1e-13)
    # a NaN block poisons its neuron alone
    ll[3, 2, 1] = np.nan
    a = MC.waic_from_accumulators(PR.host_accumulate(ll), ll.shape[0])
    assert np.isnan(a['waic'][1]) and np.all(np.isfinite(a['waic'][[0, 2, 3]]))
    with pytest.raises(ValueError):
        MC.waic_from_accumulators(np.zeros((4, 3, 2)), 1)
    print(MC.format_table(dict(b, block_bins=256)))


def test_waic_reaches_the_closed_form_of_gaussian_terms():
    """l_sb ~ N(mu_b, sigma_b^2) over the draws: lppd_b -> mu_b + sigma_b^2 / 2 and p_b -> sigma_b^2, so lppd_b - p_b ->
    mu_b - sigma_b^2 / 2.  Standard errors at S draws: var(lppd_b) ~ (exp(sigma^2) - 1) / S (delta method on the mean of
    exp), var(p_b) = 2 sigma^4 / (S - 1); the two estimates are taken as independent or worse (errors added)."""
    S, nb = 4096, 12
    rng = np.random.default_rng(2024)
    mu = -np.linspace(5.0, 300.0, nb)
    sg = np.linspace(0.05, 1.0, nb)
    ll = (mu + sg * rng.standard_normal((S, nb)))[:, :, None]
    res = MC.waic_from_accumulators(PR.host_accumulate(ll), S)
    acc = PR.host_accumulate(ll)
    el = (np.log(acc[1] / S) + acc[0] - acc[3] / (S - 1.0))[:, 0]
    se = np.sqrt(np.expm1(sg ** 2) / S) + np.sqrt(2.0 * sg ** 4 / (S - 1.0))
    z = (el - (mu - 0.5 * sg ** 2)) / se
    print("closed form: worst |z| = %.2f" % np.max(np.abs(z)))
    assert np.all(np.abs(z) <= 3.0)
    assert abs(res['elpd_waic'][0] - np.sum(mu - 0.5 * sg ** 2)) <= 3.0 * np.sqrt(np.sum(se ** 2))
    assert abs(res['p_waic'][0] - np.sum(sg ** 2)) <= 3.0 * np.sqrt(np.sum(2.0 * sg ** 4 / (S - 1.0)))


def test_heldout_table_and_log_mean_exp():
    tr = np.array([[-1000.0, -3.0], [-1001.0, -3.0], [-999.0, -3.0]])
    lme = MC.log_mean_exp(tr)
    assert abs(lme[0] - (-999.0 + np.log((1 + np.exp(-1) + np.exp(-2)) / 3))) < 1e-12 and lme[1] == -3.0
    txt = MC.format_table({'lpd': lme, 'trace': tr, 'n_draws': 3})
    assert 'held-out' in txt and len(txt.splitlines()) == 5
    for bad in ([[1.0, 2.0]], np.zeros((3, 2, 4)), np.zeros((0, 2, 5)), np.zeros((3, 0, 5))):      # not (S, M, P = 5): before any device work
        with pytest.raises(ValueError, match="samples"):
            MC._draws(bad, 5)
    assert MC._draws([[[0.0] * 5] * 2] * 3, 5)[0].shape == (3, 2, 5) and MC._draws(np.zeros((2, 3, 1, 5)), 5)[0].shape == (6, 1, 5)
    doc = MC.__doc__
    assert 'conditionally independent' in doc and 'depends on the block length' in doc and 'PSIS-LOO' in doc


# ---- the draws of the GPU accumulator test ---------------------------------------------------------------------------------
@longdouble
def test_draws_of_the_gpu_test_spread_enough():
    """every block's sd over the 33 draws is at least 1e-3 of its |mean| (Welford's M2 then loses at most ~S u 1e3 ~ 4e-12
    relative: the GPU test's 1e-9 leaves two orders), on the first range and the smallest block of every case"""
    for c in CASES:
        t_lo, t_hi, bcs, _ = PR.ranges(c)[0]
        th = PR.draws(c)
        assert th.shape == (PR.N_DRAWS, c['N'], 1 + c['N'] * 5) and np.all(np.isfinite(th))
        for bc in sorted(set((bcs[0], bcs[min(1, len(bcs) - 1)], bcs[-1]))):     # (the second is the GPU test's)
            ll = PR.draw_blocks(c, t_lo, t_hi, bc)
            assert np.all(np.isfinite(ll)), c['name']
            spread = ll.std(axis=0, ddof=1) / np.abs(ll.mean(axis=0))
            print("%-17s block_chunks %2d: smallest sd / |mean| over the draws %.2e" % (c['name'], bc, spread.min()))
            assert spread.min() >= PR.SPREAD, (c['name'], bc, spread.min())
