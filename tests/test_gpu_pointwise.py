"""k_pw_chunk / k_pw_block (pgl_pointwise_dev) over the shapes where their geometry can break -- tests/pointwise_cases.json,
one case per edge: a single short chunk, whole chunks with events on their edges, last chunks that are no multiple of the
8-row unroll, t_lo > 0 off the 256-bin grid with events right behind t_hi, block_chunks = 1, 2, 3 with a short last block
and one value >= nchunks, a silent neuron, a dense neuron with up to 3 spikes per bin, N = 1 / 16 / 17 / 40 (xs = 48) / 70,
and at N = 16 currents wholly inside each series of pgl_lambda_only (both signs), mixed, and exp with biases from -20 to 8.
tests/test_pointwise_host.py proves on the CPU that each case reaches what it names and that the bound below rejects three
emulated defects of the decomposition.

Per (case, range, block_chunks): NaN-filled output, two calls with identical bits, nothing left NaN; the recorded launches
end in the two kernels and equal the dry run of path 7; |l_dev - l_ref| <= 1e-10 |l_ref| + 1e-12 A_b against
tests/pointwise_reference.reference (longdouble on the oracle's features); sum_b l_dev = pgl_ll_grad_dev's ll within
1e-10 sum_b A_b.  Per case: 33 jittered draws folded into the device accumulator, against the host build of the rule fed
the device's own per-draw values (1e-12 on m + log e and the mean, 1e-9 on M2), one draw with a NaN bias.
One end-to-end run: 64 HMC draws at N = 2, WAIC by both routes and the held-out density against compute_ll_vector.

Worst ratio per case on the MI355X: docs/NOTEBOOK.md, "Pointwise log-likelihood sweep"."""
import numpy as np
import pytest

from tests import pointwise_reference as PR
from theano_pyglm_amd import _lib

pytestmark = pytest.mark.gpu

CASES = PR.load_cases()


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _run_twice(d, d_th, d_W, bc, nb, N):
    import torch
    outs = []
    for _ in range(2):
        d_ll = torch.full((nb, N), float('nan'), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        d.pointwise_dev(d_th.data_ptr(), d_W.data_ptr(), bc, d_ll.data_ptr())
        d.sync()
        outs.append(d_ll.cpu().numpy().copy())
    return outs


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_pointwise_case(c):
    import torch
    p = PR.problem(c)
    N = p.N
    d = p.device(0)
    try:
        d.set_option(_lib.OPT_RECORD_KERNELS, 1)
        d_th, d_W = _t(p.theta), _t(p.Weff)
        plan = _lib.plan_kernels(N, B=p.B, R=p.R, Dstim=0, nT=p.nT, n_lo=0, count=N, path=7)
        chunk = 'k_pw_chunk<%d>' % (c['kind'] == 'explinear')
        worst = 0.0
        for t_lo, t_hi, bcs, hits in PR.ranges(c):
            d.set_time_range(t_lo, t_hi)
            d_llg = torch.full((N,), float('nan'), dtype=torch.float64, device='cuda')
            torch.cuda.synchronize()
            d.ll_grad_dev(d_th.data_ptr(), d_W.data_ptr(), d_llg.data_ptr(), 0)
            d.sync()
            ll_fused = d_llg.cpu().numpy()
            for bc in bcs:
                label = "%s [%d, %d) block_chunks %d" % (c['name'], t_lo, t_hi, bc)
                ref = PR.reference(c, t_lo, t_hi, bc)
                nb = d.pointwise_count(bc)
                assert nb == ref[0].shape[0] == PR.geometry(t_lo, t_hi, bc)[1], label
                ll, ll2 = _run_twice(d, d_th, d_W, bc, nb, N)
                names = d.last_kernels()
                assert names[-2:] == [chunk, 'k_pw_block'], names
                # (the dry run's context has the whole recording and nlin = exp)
                assert plan[-2:] == ['k_pw_chunk<0>', 'k_pw_block'], plan
                if (t_lo, t_hi) == (0, p.nT):
                    assert names[:-2] == plan[:-2], (names, plan)
                assert ll.tobytes() == ll2.tobytes(), label + ": two calls differ"
                assert np.all(np.isfinite(ll)), label + ": an output was never written"
                r = PR.ratio(ll, ref)
                tot = float(np.max(np.abs(ll.sum(axis=0) - ll_fused) / (1e-10 * ref[1].sum(axis=0))))
                print("%s: worst |dl| / (1e-10 |l| + 1e-12 A) = %.3e, worst |sum_b l - ll| / (1e-10 sum_b A) = %.3e  (%d blocks)"
                      % (label, r, tot, nb))
                worst = max(worst, r)
                assert r <= 1.0, label
                assert tot <= 1.0, label
                assert np.array_equal(d.pointwise(p.theta, p.Weff, bc), ll), label     # the host-pointer form is the same call
        print("%s: worst ratio of the case %.3e" % (c['name'], worst))
    finally:
        d.close()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_accumulator_over_draws(c):
    """33 jittered draws (tests/pointwise_reference.draws: every block's sd over the draws >= 1e-3 of its |mean|, checked
    on the CPU) folded in on the device, each draw's block sums requested too; the final state against the host build of
    the rule fed those sums.  M2: Welford's error is about S u kappa with kappa <= 1e3 by the spread condition, ~4e-12;
    1e-9 leaves two orders.  Draw 5 carries a NaN bias in neuron 1: that neuron's states are NaN, nothing else is."""
    import torch
    p = PR.problem(c)
    N = p.N
    t_lo, t_hi, bcs, _ = PR.ranges(c)[0]
    bc = bcs[min(1, len(bcs) - 1)]
    sp, jp = PR.poisoned(c)
    S = PR.N_DRAWS
    d = p.device(0)

    def fold(th, fill, want_ll):
        d_th = _t(th)
        d_acc = torch.full((4, nb, N), fill, dtype=torch.float64, device='cuda')      # (draw 0 must initialise it)
        d_ll = torch.full((S, nb, N), float('nan'), dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
        for s in range(S):
            d.pointwise_dev(d_th[s].data_ptr(), d_W.data_ptr(), bc, d_ll[s].data_ptr() if want_ll else 0, d_acc.data_ptr(), s)
        d.sync()
        return d_acc.cpu().numpy(), d_ll.cpu().numpy()

    try:
        d.set_time_range(t_lo, t_hi)
        nb = d.pointwise_count(bc)
        d_W = _t(p.Weff)
        th = np.array(PR.draws(c))
        th[sp, jp, 0] = np.nan
        acc, ll = fold(th, 4321.5, True)
        assert fold(th, -1.0, False)[0].tobytes() == acc.tobytes()       # the accumulator alone (d_ll_blk NULL): the same state
        bad = np.zeros((nb, N), dtype=bool)
        bad[:, jp] = True
        assert np.array_equal(np.isnan(ll), np.broadcast_to(bad[None] & (np.arange(S) == sp)[:, None, None], ll.shape))
        assert np.array_equal(np.isnan(acc), np.broadcast_to(bad[None], acc.shape)), "NaN states beyond the poisoned neuron"
        if N == 1:                                               # nothing finite is left to compare: the clean draws too
            acc, ll = fold(PR.draws(c), 4321.5, True)
            bad[:] = False
            assert np.all(np.isfinite(acc)) and np.all(np.isfinite(ll))
    finally:
        d.close()
    host = PR.host_accumulate(ll)
    assert np.array_equal(np.isnan(host), np.isnan(acc))
    ok = ~bad
    rel = lambda a, b: float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))
    r_lse = rel(acc[0] + np.log(acc[1]), host[0] + np.log(host[1]))
    r_mean, r_m2 = rel(acc[2], host[2]), rel(acc[3], host[3])
    spread = float(np.min((np.sqrt(host[3] / (S - 1.0)) / np.abs(host[2]))[ok]))
    print("%s block_chunks %d: m + log e %.2e, mean %.2e, M2 %.2e relative to the host mirror; smallest sd / |mean| %.2e"
          % (c['name'], bc, r_lse, r_mean, r_m2, spread))
    assert spread >= PR.SPREAD
    assert np.array_equal(acc[0][ok], host[0][ok])
    assert r_lse <= 1e-12 and r_mean <= 1e-12
    assert r_m2 <= 1e-9


def test_argument_and_state_errors():
    import torch
    d = _lib.DeviceGlm(4, 600, 5, 32, 'explinear', 0.001, 0)
    try:
        buf = torch.zeros(4 * 200, dtype=torch.float64, device='cuda')
        with pytest.raises(_lib.PglError, match="pgl_set_spikes"):
            d.pointwise_dev(buf.data_ptr(), buf.data_ptr(), 1, buf.data_ptr())
        with pytest.raises(_lib.PglError, match="pgl_set_spikes"):
            d.pointwise(np.zeros((4, 21)), np.zeros((4, 4)), 1)
    finally:
        d.close()
    c = CASES[0]
    p = PR.problem(c)
    d = p.device(0)
    try:
        d_th, d_W = _t(p.theta), _t(p.Weff)
        out = torch.zeros((4, 2, p.N), dtype=torch.float64, device='cuda')
        with pytest.raises(_lib.PglError, match="block_chunks"):
            d.pointwise_dev(d_th.data_ptr(), d_W.data_ptr(), 0, out.data_ptr())
        with pytest.raises(_lib.PglError, match="block_chunks"):
            d.pointwise_count(0)
        with pytest.raises(_lib.PglError, match="neither"):
            d.pointwise_dev(d_th.data_ptr(), d_W.data_ptr(), 1, 0, 0)
        with pytest.raises(_lib.PglError, match="draw"):
            d.pointwise_dev(d_th.data_ptr(), d_W.data_ptr(), 1, 0, out.data_ptr(), -1)
        with pytest.raises(_lib.PglError, match="null"):
            d.pointwise_dev(0, d_W.data_ptr(), 1, out.data_ptr())
        assert d.pointwise_count(1) == 1 and d.pointwise_count(1 << 30) == 1
    finally:
        d.close()


def test_waic_and_heldout_density_end_to_end():
    """64 HMC draws at N = 2, nT = 2048 (8 chunks): waic_glms = waic_from_pointwise of the pointwise matrix to 1e-9, the matrix
    of a draw = Population.compute_pointwise_ll of that draw, and with one block heldout_lpd on the same data = logsumexp of
    the per-draw compute_ll_vector values - log S to 1e-10."""
    from tests.test_gpu_hvp import _std_population
    from theano_pyglm_amd.inference import batched_hmc as B
    from theano_pyglm_amd.inference import model_compare as MC
    popn = _std_population(2, 2.048, 31, nlin='exp', bias_mu=3.0)
    try:
        x = popn.sample(np.random.RandomState(97))
        S = 64
        out = B.sample_glms_hmc(popn, x, S, n_warmup=20, n_leapfrog=4, step_sz=0.02, seed=3)
        smp = out['samples']
        assert smp.shape == (S, 2, popn.glm.P) and np.std(smp[:, 0, 0]) > 0
        bc = 3                                                    # 8 chunks: blocks of 3, 3 and 2
        res = MC.waic_glms(popn, x, smp, block_chunks=bc)
        r = MC.pointwise_ll_draws(popn, x, smp, block_chunks=bc, pointwise=True)
        assert r['ll'].shape == (S, 3, 2) and r['acc'].shape == (4, 3, 2) and r['blocks_per_sequence'] == [3]
        ref = MC.waic_from_pointwise(r['ll'])
        print(MC.format_table(res))
        for k in ('elpd_waic', 'p_waic', 'lppd', 'waic', 'se'):
            assert np.all(np.abs(res[k] - ref[k]) <= 1e-9 * np.abs(ref[k])), (k, res[k], ref[k])
        assert np.array_equal(res['n_high_var'], ref['n_high_var']) and res['n_blocks'] == 3 and res['block_bins'] == 768
        for i in (0, S - 1):
            xi = dict(x, glms=B.samples_to_states(popn, x, smp, i))
            assert np.array_equal(popn.compute_pointwise_ll(xi, bc), r['ll'][i])
        # a range of neurons, from a device tensor with a chain axis: the same numbers
        import torch
        sub = MC.pointwise_ll_draws(popn, x, torch.tensor(smp[:, 1:2], device='cuda').reshape(2, S // 2, 1, -1), bc, n_lo=1,
                                    pointwise=True)
        assert np.array_equal(sub['ll'], r['ll'][:, :, 1:2]) and np.array_equal(sub['acc'], r['acc'][:, :, 1:2])
        held = MC.heldout_lpd(popn, x, smp)
        lls = np.array([popn.compute_ll_vector(dict(x, glms=B.samples_to_states(popn, x, smp, i))) for i in range(S)])
        m = lls.max(axis=0)
        want = np.log(np.sum(np.exp(lls - m), axis=0)) + m - np.log(S)
        print(MC.format_table(held))
        print("held-out lpd %s, from compute_ll_vector %s" % (held['lpd'], want))
        assert held['trace'].shape == (S, 2)
        assert np.all(np.abs(held['lpd'] - want) <= 1e-10 * np.abs(want))
        popn.set_time_shard(0, 2)
        try:
            with pytest.raises(ValueError, match="time-sharded"):
                popn.compute_pointwise_ll(x)
            with pytest.raises(ValueError, match="time-sharded"):
                MC.waic_glms(popn, x, smp)
        finally:
            popn.set_time_shard(None)
    finally:
        popn.release_data()
