"""GPU tests of the lock-step Newton-CG sweep (inference/batched_newton_cg.py on the pgl_ncg_* row kernels): every row
reaches the optimum of the sequential fit_glm(use_rop=True) fit of the same commit from the same start, the rows run in
lock step (one product launch per CG iteration of the slowest row, finished rows frozen), and coord_descent's
use_rop + batched='torch' path."""
import copy

import numpy as np
import pytest

from tests.test_gpu_hvp import _std_population

pytestmark = pytest.mark.gpu


def _sequential(popn, x0, neurons):
    """fit_glm(use_rop=True) per neuron from x0: {n: (result, slack)}, the slack measured by restarting the fit from its
    own optimum (at least one f64 spacing of the objective), as test_newton_cg_fit_reaches_the_bfgs_optimum does."""
    from theano_pyglm_amd.inference import coord_descent as cd
    prms = cd.prep_first_order_glm_inference(popn)
    hessp = cd.prep_second_order_glm_inference(popn)
    out = {}
    for n in neurons:
        nv = popn.extract_vars(copy.deepcopy(x0), n)
        res = cd.fit_glm(nv, n, prms, use_rop=True, hessp=hessp)
        res2 = cd.fit_glm(nv, n, prms, use_rop=True, hessp=hessp)      # restart from the fit's own optimum
        out[n] = (res, max(res.fun - res2.fun, np.spacing(abs(res.fun))))
    return out


def _compare(popn, x0, neurons, label):
    from theano_pyglm_amd.inference import batched_newton_cg as B
    x = copy.deepcopy(x0)
    fun, nit, nfev, nhev, status = B.fit_glms_newton_cg_torch(popn, x)
    seq = _sequential(popn, x0, neurons)
    for n in neurons:
        res, slack = seq[n]
        print("%s neuron %d: lock-step nlp %.12g nit %d nhev %d status %d | sequential nlp %.12g nit %d nhev %d status %d "
              "| difference %.3e slack %.3e" % (label, n, fun[n], nit[n], nhev[n], status[n], res.fun, res.nit, res.nhev,
                                                res.status, fun[n] - res.fun, slack))
    print("%s launches: %s" % (label, dict((k, v) for k, v in popn.last_fit_stats.items() if k != 'per_neuron')))
    assert np.all(status == 0), dict(zip(*np.unique(status, return_counts=True)))
    for n in neurons:
        res, slack = seq[n]
        assert fun[n] <= res.fun + 10.0 * slack
    return x, fun, seq


def test_lockstep_reaches_the_sequential_optimum_n4():
    """Issue item 4: N = 4, 60 s, exp, the population of test_newton_cg_fit_reaches_the_bfgs_optimum."""
    popn = _std_population(4, 60.0, 89, nlin='exp', bias_mu=3.0)
    try:
        x0 = popn.sample(np.random.RandomState(97))
        _compare(popn, x0, range(4), "N=4")
    finally:
        popn.release_data()


def test_lockstep_reaches_the_sequential_optimum_n128_fused_apply():
    """N = 128 with a short recording: the product of all rows runs k_hvp5 + pass 2 of k_fused5; sequential fits of a
    seeded subset of 8 neurons.  120 s of spikes: 2 400 per neuron for its 641 parameters, so that the data and not the
    kink of the group lasso at a zero group decide where a fit ends.  Measured on the MI355X at 120 s: 6 of the 8 rows take
    the sequential fit's nit and nhev exactly or within one product, all end within the bound (largest excess over the
    sequential objective 5.8e-7 against a slack of 9.4e-8; one sequential fit stops 3e-2 early and is beaten by that).
    Shorter recordings do not pose the comparison: at 30 s the sequential fits' own slack ranges from 5e-13 to 2e-2 and
    the two fits of a neuron stop up to 6 outer iterations apart (differences -2e-2 .. +6e-3); at 3 s both wander through
    4 000 .. 12 000 products per neuron and stop 0.1 .. 1 apart in either direction -- two rounding histories of an
    ill-posed problem (independent Poisson spikes: every impulse group's optimum is next to zero, where the group-lasso
    Hessian grows like 1 / |w_g|), not two optimisers."""
    from theano_pyglm_amd import _lib
    popn = _std_population(128, 120.0, 101, nlin='exp', bias_mu=3.0)
    try:
        for data in popn.data_sequences:
            popn.set_data(data)
            popn._handle(data).set_option(_lib.OPT_RECORD_KERNELS, 1)
        x0 = popn.sample(np.random.RandomState(103))
        neurons = sorted(np.random.default_rng(107).choice(128, size=8, replace=False).tolist())
        _compare(popn, x0, neurons, "N=128")
        names = popn.last_fit_stats['apply_kernels']
        print("apply kernels:", names)
        assert names and names[0].startswith('k_hvp5<') and any(k.startswith('k_fused5<') for k in names[1:])
    finally:
        popn.release_data()


def test_lockstep_group_lasso_start_with_a_zero_group_n32():
    """N = 32, group-lasso prior, a start that holds an exactly zero group in some rows: the prior's gradient and product
    are NaN there and fit_glm's rules (gradient -> 0, product -> 0) run on the device."""
    popn = _std_population(32, 6.0, 109, nlin='exp', bias_mu=3.0)
    try:
        from theano_pyglm_amd.components.priors import GroupLasso
        assert isinstance(popn.glm.imp_model.prior, GroupLasso)
        x0 = popn.sample(np.random.RandomState(113))
        B = popn.glm.imp_model.B
        for n in (3, 17):
            w = np.array(x0['glms'][n]['imp']['w_ir'], dtype=float).reshape(-1)
            w[5 * B:6 * B] = 0.0
            x0['glms'][n]['imp']['w_ir'] = w.reshape(np.shape(x0['glms'][n]['imp']['w_ir']))
        _compare(popn, x0, [0, 3, 9, 17, 31], "N=32 group lasso")
    finally:
        popn.release_data()


def test_lockstep_means_lockstep():
    """Rows that converge at different outer iterations (row 2 starts at the optimum of a previous fit): a finished row's
    parameters stay bit-identical while the others go on, and the sweep makes one product launch per CG iteration of
    the SLOWEST active row of each outer iteration -- the sum of the per-iteration maxima, not the sum over rows."""
    from theano_pyglm_amd.inference import batched_newton_cg as B
    popn = _std_population(4, 60.0, 89, nlin='exp', bias_mu=3.0)
    try:
        x0 = popn.sample(np.random.RandomState(97))
        x1 = copy.deepcopy(x0)
        B.fit_glms_newton_cg_torch(popn, x1)
        x0['glms'][2] = copy.deepcopy(x1['glms'][2])
        trace = []
        x = copy.deepcopy(x0)
        fun, nit, nfev, nhev, status = B.fit_glms_newton_cg_torch(popn, x, on_outer=lambda k, info: trace.append(info))
        print("nit", nit, "nhev", nhev, "status", status)
        assert np.all(status == 0)
        assert nit[2] < nit.max()
        stats = popn.last_fit_stats
        prev = np.zeros(4, dtype=int)
        expected = 0
        for info in trace:
            expected += int((info['nhev'] - prev).max())
            prev = info['nhev']
        print("apply launches %d, sum of per-iteration maxima %d, sum over rows %d" % (stats['apply_launches'], expected, nhev.sum()))
        assert stats['apply_launches'] == expected == sum(stats['cg_lengths'])
        assert expected < nhev.sum()
        for r in range(4):                                     # frozen from the iteration in which the row finished
            first = next(k for k, info in enumerate(trace) if info['status'][r] >= 0)
            for info in trace[first:]:
                assert np.array_equal(info['X'][r], trace[first]['X'][r])
                assert info['nhev'][r] == trace[first]['nhev'][r] and info['nit'][r] == trace[first]['nit'][r]
            assert np.array_equal(trace[-1]['X'][r], trace[first]['X'][r])
        assert next(k for k, info in enumerate(trace) if info['status'][2] >= 0) < len(trace) - 1
    finally:
        popn.release_data()


def test_coord_descent_use_rop_batched_torch():
    from theano_pyglm_amd.inference import coord_descent as cd
    from theano_pyglm_amd.models.model_factory import make_model
    from theano_pyglm_amd.population import Population
    popn = _std_population(4, 60.0, 89, nlin='exp', bias_mu=3.0)
    try:
        x0 = popn.sample(np.random.RandomState(97))
        xs = cd.coord_descent(popn, copy.deepcopy(x0), maxiter=1, use_rop=True)
        xl = cd.coord_descent(popn, copy.deepcopy(x0), maxiter=1, use_rop=True, batched='torch')
        # (coord_descent initialises from the data before the sweep: the slack is measured from that start)
        from theano_pyglm_amd.inference.smart_init import initialize_with_data
        xi = copy.deepcopy(x0)
        initialize_with_data(popn, popn.data_sequences[-1], xi)
        slack = sum(s for _, s in _sequential(popn, xi, range(4)).values())
        lps, lpl = popn.compute_log_p(xs), popn.compute_log_p(xl)
        print("coord_descent: sequential log p %.12g, lock-step %.12g, summed slack %.3e" % (lps, lpl, slack))
        assert lpl >= lps - 10.0 * slack
        with pytest.raises(ValueError, match="use_rop"):
            cd.coord_descent(popn, copy.deepcopy(x0), maxiter=1, use_rop=True, batched=True)
        popn.set_time_shard(0, 2)
        try:
            with pytest.raises(ValueError, match="time-sharded"):
                cd.coord_descent(popn, copy.deepcopy(x0), maxiter=1, use_rop=True, batched='torch')
        finally:
            popn.set_time_shard(None)
    finally:
        popn.release_data()
    for name in ('spatiotemporal_glm', 'sparse_weighted_model'):
        p2 = Population(make_model(name, N=2, dt=0.001))
        with pytest.raises(ValueError, match="Impulses|Stimulus"):
            cd.coord_descent(p2, p2.sample(np.random.RandomState(1)), maxiter=1, use_rop=True, batched='torch')
