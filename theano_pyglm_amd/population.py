"""
Population -- connected GLMs (counterpart of pyglm/population.py).

Same construction and method surface as the reference (`Population(model)`, `add_data`,
`set_data`, `sample`, `extract_vars`, `compute_log_p`, `compute_log_prior`, `compute_ll`,
`eval_state`, `simulate`) plus the gradient entry points the reference builds with
T.grad inside its inference code (coord_descent.py:27-30): `compute_ll_grad` (all
neurons in one fused device pass) and `compute_grad(vars, n)`.

Every data sequence is uploaded to the GPU once (spike counts as uint8 + the
spike-event index, the interpolated impulse basis, dense stimulus features) and stays
resident; `set_data` only switches the current handle -- the reference re-copies the
whole feature tensor into Theano shared variables on every evaluation
(coord_descent.py:52-57, glm.py:99-110).  There is no CPU fallback.
"""
import os

import numpy as np

from theano_pyglm_amd import _lib
from theano_pyglm_amd.components.latent import LatentVariables
from theano_pyglm_amd.components.network import Network
from theano_pyglm_amd.glm import Glm
from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars
from theano_pyglm_amd.utils.syms import from_shapes, differentiable, check_bound, compile_bound, compile_paths, check_paths


class Population(object):
    def __init__(self, model, device=None):
        """population.py:12-32."""
        self.model = model
        self.N = model['N']
        self.data_sequences = []
        self.latent = LatentVariables(model)
        self.network = Network(model, self.latent)
        self.glm = Glm(model, self.network, self.latent)
        self.device = int(os.environ.get('PYGLM_DEVICE', '0')) if device is None else int(device)
        self._handles = []        # (data dict, _lib.DeviceGlm) pairs: the pair keeps the dict alive, so a
                                  # recycled id() can never alias a stale handle; lookup is by identity
        self._current = None      # data dict conditioned on (set_data)
        self._time_shard = None   # (rank, world): every handle evaluates only its share of the bins

    # -- variables ------------------------------------------------------------
    def get_variables(self):
        """population.py:133-140."""
        return {'latent': {},
                'net': from_shapes(self.network.get_variables(), int_keys=('A',)),
                'glm': self.glm.get_variables()}

    def set_hyperparameters(self, model):
        """population.py:142-147."""
        self.network.set_hyperparameters(model)
        self.glm.set_hyperparameters(model)

    def sample(self, rng=None):
        """population.py:149-162: latent -> net -> glms[0..N-1]."""
        v = {'latent': {}}
        v['net'] = self.network.sample(v, rng=rng)
        v['glms'] = []
        for n in range(self.N):
            xn = self.glm.sample(v, rng=rng)
            xn['n'] = n
            v['glms'].append(xn)
        return v

    def shape_vars(self):
        """A value dictionary laid out like sample() with zeros of every symbol's shape -- for callers that need the
        packing shapes only (the reference draws a sample for that, coord_descent.py:24-26, 93-95; here the shapes come from
        the symbol table: 2 x 2.5 ms of Python per sweep at N = 128, and no random numbers consumed)."""
        def zeros(syms):
            out = {}
            for k, v in syms.items():
                out[k] = zeros(v) if isinstance(v, dict) else np.zeros(v.shape, dtype=v.dtype)
            return out
        syms = self.get_variables()
        v = {'latent': {}, 'net': zeros(syms['net']), 'glms': []}
        z = zeros(dict((k, s) for k, s in syms['glm'].items() if k != 'n'))
        for n in range(self.N):
            xn = dict(z)                                      # (the neurons share the zero arrays: shapes are all that is read)
            xn['n'] = n
            v['glms'].append(xn)
        return v

    def extract_vars(self, vals, n):
        """population.py:164-175."""
        out = {}
        for k, v in vals.items():
            if k == 'glms':
                out['glm'] = v[n]
            else:
                out[k] = v
        return out

    # -- data -------------------------------------------------------------------
    def preprocess_data(self, data):
        """population.py:187-196 (the impulse features fS are NOT materialised)."""
        assert isinstance(data, dict), 'Data must be a dictionary'
        self.glm.preprocess_data(data)
        data['preprocessed'] = True
        return data

    def add_data(self, data, set_as_current_data=True):
        """population.py:198-221."""
        assert isinstance(data, dict), 'Data must be a dictionary'
        assert 'S' in data, 'Data must contain an array of spike times'
        assert isinstance(data['S'], np.ndarray), 'Spike times must be a numpy array'
        if 'preprocessed' not in data or not data['preprocessed']:
            data = self.preprocess_data(data)
        self.data_sequences.append(data)
        if set_as_current_data:
            self.set_data(data)

    def _find_handle(self, data):
        for d, h in self._handles:
            if d is data:
                return h
        return None

    def _handle(self, data):
        h = self._find_handle(data)
        if h is None:
            S = np.asarray(data['S'])
            nT, N = S.shape
            assert N == self.N, "ERROR: Spike train must be (TxN) dimensional where N=%d" % self.N
            imp = self.glm.imp_model
            h = _lib.DeviceGlm(N, nT, imp.B, imp.ibasis.shape[0], self.glm.nlin_model.kind,
                               self.glm.dt, device=self.device)
            h.set_spikes(S)
            h.set_basis(imp.ibasis)
            # no per-evaluation HIP events on the product path: an event between two kernels of a stream idles the GPU
            # for ~6 us (pgl_last_timing is for the measurement tools, which drive DeviceGlm directly)
            h.set_option(_lib.OPT_TIMING, 0)
            if self.glm.Dstim > 0:
                if data.get('fstim', None) is not None:
                    if getattr(self.glm.bkgd_model, 'separable', False):
                        raise ValueError("data['fstim'] (dense stimulus features) cannot be used with the separable "
                                         "stimulus path: theta rows carry [w_t, w_x] there; drop 'fstim' (the features are "
                                         "built from data['stim'] on the device) or set model['bkgd']['separable'] = False")
                    h.set_stim_features(data['fstim'])      # caller-supplied dense features
                else:
                    self.glm.bkgd_model.upload(h, data)     # built on the device from data['stim']
            if self._time_shard is not None:
                self._apply_time_shard(h)
            self._handles.append((data, h))
        return h

    def _apply_time_shard(self, h):
        from theano_pyglm_amd.parallel import time_shard_bounds
        if self._time_shard is None:
            h.set_time_range(0, h.nT)
        else:
            rank, world = self._time_shard
            h.set_time_range(*time_shard_bounds(h.nT, rank, world))

    def set_time_shard(self, rank=None, world=None):
        """Restrict every data sequence to the bins of time shard `rank` of `world` (boundaries on the
        kernels' 16-bin tile grid; the likelihood is additive over time segments, population.py:41-43, so
        the partial (ll, grad) of the shards all-reduce to the full evaluation).  None: the whole
        recording.  Used by the time-sharded multi-GPU MAP (inference/parallel_coord_descent.py)."""
        self._time_shard = None if rank is None or world in (None, 1) else (int(rank), int(world))
        for _, h in self._handles:
            self._apply_time_shard(h)

    def set_data(self, data):
        """population.py:223-231: condition on `data` (switches the device-resident handle)."""
        assert 'preprocessed' in data and data['preprocessed'] == True, \
            'Data must be preprocessed before it can be set'
        self._handle(data)
        self._current = data

    def stim_features(self, data=None):
        """The dense stimulus feature columns `fstim` (nT, Dstim) of a data sequence (the reference
        keeps them in data['fstim'], bkgd.py:154 / 340); here they live on the device and are
        copied out on request."""
        data = self._current if data is None else data
        if self.glm.Dstim == 0:
            return None
        if getattr(self.glm.bkgd_model, 'separable', False):     # no dense matrix on the device: host twin
            return self.glm.bkgd_model.host_features(data, np.asarray(data['S']).shape[0])
        return self._handle(data).get_stim_features()

    def release_data(self, data=None):
        """Free the device buffers of one data sequence (or of all of them).

        Ownership: the population keeps a strong reference to every data dict it has been conditioned on
        (`add_data`, `set_data`, and internally every evaluation on a held-out dict) together with its device
        handle -- spikes, event index and up to three sets of resident feature tiles (3 GB at N=128, T=600 s) --
        until this method is called; the reference's shared variables are simply overwritten by the next
        set_data (glm.py:99-110).  Transient data sets (cross-validation splits, initialisation populations)
        should be released explicitly, as harness/synth_map_with_xv.py and inference/gibbs.py do."""
        keep = []
        for d, h in self._handles:
            if data is None or d is data:
                h.close()
                if self._current is d:
                    self._current = None
            else:
                keep.append((d, h))
        self._handles = keep

    # -- parameters -> device layout ----------------------------------------------
    def theta_matrix(self, vars, n_lo=0, n_hi=None):
        n_hi = self.N if n_hi is None else n_hi
        return self.glm.theta_rows([vars['glms'][n] for n in range(n_lo, n_hi)])

    def W_eff(self, vars):
        return self.network.W_eff(vars['net'])

    def _check_vars(self, vars, n=None):
        """Mirror of seval's binding check (theano_func_wrapper.py:69-105): every symbol of the network and of the listed
        neuron's GLM (n None: of every neuron) must have a value.  The symbol tables are those of the model and do not
        change: built once."""
        cache = getattr(self, '_bound_syms', None)
        if cache is None:
            syms = self.get_variables()
            net_tree = compile_bound({'net': syms['net']})
            glm_tree = compile_bound(dict((k, v) for k, v in syms['glm'].items() if k != 'n'))
            cache = (net_tree, compile_paths(net_tree), glm_tree, compile_paths(glm_tree))
            self._bound_syms = cache
        net_tree, net_paths, glm_tree, glm_paths = cache
        check_paths(net_paths, net_tree, vars)
        glms = vars['glms']
        for m in (range(self.N) if n is None else (n,)):
            check_paths(glm_paths, glm_tree, glms[m])

    # -- log probability ---------------------------------------------------------------
    def compute_log_prior(self, vars):
        """population.py:47-69: latent + network + sum_n glm.log_prior."""
        self._check_vars(vars)
        return self._log_prior(vars)

    def _log_prior(self, vars):
        lp = 0.0
        lp += self.latent.log_p(vars.get('latent', {}))
        lp += self.network.log_p(vars['net'])
        lp += self.glm.log_prior_all([vars['glms'][n] for n in range(self.N)])
        return lp

    def compute_ll_vector(self, vars, n_lo=0, n_hi=None):
        """Per-neuron ll of the CURRENT data sequence for neurons [n_lo, n_hi)."""
        n_hi = self.N if n_hi is None else n_hi
        if self._current is None:
            raise Exception("No data sequence has been set")
        h = self._handle(self._current)
        ll, _ = h.ll_grad(self.theta_matrix(vars, n_lo, n_hi), self.W_eff(vars), n_lo, n_hi,
                          want_grad=False)
        return ll

    def compute_ll(self, vars):
        """population.py:71-86: sum over neurons of glm.ll on the current data."""
        self._check_vars(vars)
        return float(np.sum(self.compute_ll_vector(vars)))

    def compute_log_p(self, vars):
        """population.py:34-45 (lkhd_scale is not applied here, like the reference).  The variables are checked once for
        the prior and all data sequences."""
        self._check_vars(vars)
        lp = 0.0
        lp += self._log_prior(vars)
        for data in self.data_sequences:
            self.set_data(data)
            lp += float(np.sum(self.compute_ll_vector(vars)))
        return lp

    # -- gradients (the reference: T.grad in coord_descent.py:27-30) --------------------
    def compute_ll_grad(self, vars, n_lo=0, n_hi=None):
        """ll_n and d ll_n / d(flat feature weights) for n in [n_lo,n_hi) on the current data:
        returns (ll (npost,), g_theta (npost,P)) straight from the fused device pass."""
        n_hi = self.N if n_hi is None else n_hi
        h = self._handle(self._current)
        return h.ll_grad(self.theta_matrix(vars, n_lo, n_hi), self.W_eff(vars), n_lo, n_hi)

    def glm_syms(self):
        """differentiable(syms['glm']) (coord_descent.py:24)."""
        return differentiable(self.get_variables()['glm'])

    def compute_lp_grad_packed(self, vars, n_lo=0, n_hi=None, include_prior=True):
        """For every neuron n in [n_lo,n_hi): log posterior of its GLM parameters
        (log_prior_n + sum_data ll_n) and the gradient w.r.t. the packed per-neuron vector
        (layout = packdict of the differentiable GLM variables).
        Returns (lp (npost,), grads (npost, P_packed))."""
        n_hi = self.N if n_hi is None else n_hi
        syms = self.glm_syms()
        lps = np.zeros(n_hi - n_lo)
        grads = None
        for data in self.data_sequences:
            self.set_data(data)
            ll, g_theta = self.compute_ll_grad(vars, n_lo, n_hi)
            lps += ll
            for i, n in enumerate(range(n_lo, n_hi)):
                xn = vars['glms'][n]
                gd = self.glm.chain_grad(xn, g_theta[i])
                gv, _ = packdict(get_vars(syms, gd))
                if grads is None:
                    grads = np.zeros((n_hi - n_lo, gv.size))
                grads[i] += gv
        if include_prior:
            for i, n in enumerate(range(n_lo, n_hi)):
                xn = vars['glms'][n]
                lps[i] += self.glm.log_prior(xn)
                gv, _ = packdict(get_vars(syms, self.glm.grad_log_prior(xn)))
                grads[i] += gv
        return lps, grads

    def compute_hvp_packed(self, vars, V, n_lo=0, n_hi=None, include_prior=True):
        """For every neuron n in [n_lo, n_hi): the Hessian of (log_prior_n + sum_data ll_n) w.r.t. its packed parameter
        vector, times row n of V (npost, P_packed) -- hessian_rop_wrt_list (grads.py:68-95) for all neurons of the range,
        one curvature pass and one product on the device per data sequence.  Served where the packed vector is a
        permutation of the theta row (Glm.hvp_packing); other packings raise ValueError."""
        bad = self.glm.hvp_packing()
        if bad is not None:
            raise ValueError("Hessian-vector products are not implemented for the %s packing" % bad)
        n_hi = self.N if n_hi is None else n_hi
        syms = self.glm_syms()
        V = np.asarray(V, dtype=float)
        _, shapes = packdict(get_vars(syms, vars['glms'][n_lo]))
        vds = [unpackdict(V[i], shapes) for i in range(n_hi - n_lo)]
        # the packing is linear: the theta row of the direction is the direction in the device's layout
        v_theta = self.glm.theta_rows(vds)
        theta = self.theta_matrix(vars, n_lo, n_hi)
        Weff = self.W_eff(vars)
        out = np.zeros(V.shape)
        for data in self.data_sequences:
            self.set_data(data)
            hv = self._handle(self._current).hvp(theta, v_theta, Weff, n_lo, n_hi)
            for i, n in enumerate(range(n_lo, n_hi)):
                out[i] += packdict(get_vars(syms, self.glm.chain_grad(vars['glms'][n], hv[i])))[0]
        if include_prior:
            for i, n in enumerate(range(n_lo, n_hi)):
                out[i] += packdict(get_vars(syms, self.glm.hess_log_prior_vec(vars['glms'][n], vds[i])))[0]
        return out

    def compute_hvp(self, vars, n, v):
        """Hessian of (glm.log_prior + sum_data glm.ll) of neuron n w.r.t. its packed parameter vector, times the packed
        vector v -- the counterpart of compute_grad (minus coord_descent's hessp)."""
        return self.compute_hvp_packed(vars, np.asarray(v, dtype=float)[None, :], n, n + 1)[0]

    def compute_hessian_packed(self, vars, n_lo=0, n_hi=None, include_prior=True):
        """For every neuron n in [n_lo, n_hi): the dense Hessian of (log_prior_n + sum_data ll_n) w.r.t. its packed parameter
        vector, (npost, P, P) -- hessian_wrt_list (grads.py:30-66), the default of the reference's parallel driver
        (parallel_coord_descent.py:62).  One curvature pass and one Gram contraction on the device per data sequence
        (pgl_hess); the priors' Hessian is added on the host.  Served for the packings of compute_hvp_packed."""
        bad = self.glm.hvp_packing()
        if bad is not None:
            raise ValueError("Hessian-vector products are not implemented for the %s packing" % bad)
        n_hi = self.N if n_hi is None else n_hi
        syms = self.glm_syms()
        w0, shapes = packdict(get_vars(syms, vars['glms'][n_lo]))
        P = w0.size
        # the packed vector is a permutation of the theta row: packed position of every theta column
        pi = np.rint(self.glm.theta_row(unpackdict(np.arange(P, dtype=float), shapes))).astype(int)
        if P != self.glm.P or not np.array_equal(np.sort(pi), np.arange(P)):
            raise ValueError("the packed vector is not a permutation of the theta row")
        theta = self.theta_matrix(vars, n_lo, n_hi)
        Weff = self.W_eff(vars)
        out = np.zeros((n_hi - n_lo, P, P))
        for data in self.data_sequences:
            self.set_data(data)
            out[:, pi[:, None], pi[None, :]] += self._handle(self._current).hessian(theta, Weff, n_lo, n_hi)
        if include_prior:
            for i, n in enumerate(range(n_lo, n_hi)):
                out[i] += self.glm.hess_log_prior(vars['glms'][n])
        return out

    def compute_hessian(self, vars, n):
        """Dense Hessian of (glm.log_prior + sum_data glm.ll) of neuron n w.r.t. its packed parameter vector, (P, P): the
        matrix whose columns compute_hvp gives one at a time."""
        return self.compute_hessian_packed(vars, n, n + 1)[0]

    def compute_grad(self, vars, n):
        """Gradient of (glm.log_prior + sum_data glm.ll) of neuron n w.r.t. its packed
        parameter vector -- minus coord_descent.grad_nlp (coord_descent.py:61-80)."""
        return self.compute_lp_grad_packed(vars, n, n + 1)[1][0]

    def _per_sequence(self, vars, what, call):
        """[call(handle, theta, Weff) of every data sequence] at the whole population's theta_matrix and W_eff under `vars`;
        `what` names the quantity where a time-sharded population is turned down."""
        if self._time_shard is not None:
            raise ValueError("%s of a time-sharded population %s not implemented" % what)
        self._check_vars(vars)
        theta = self.theta_matrix(vars)
        Weff = self.W_eff(vars)
        out = []
        for data in self.data_sequences:
            self.set_data(data)
            out.append(call(self._handle(self._current), theta, Weff))
        return out

    # -- goodness of fit -------------------------------------------------------------------
    def compute_rescaled_intervals(self, vars, correct=False, seed=0, draw=0):
        """Time rescaling (Brown et al. 2002) of every neuron's spike train under `vars`: the integrated rate between
        consecutive event bins, Exp(1) under the true model.  One forward pass and one segmented sum on the device per data
        sequence (pgl_rescale); no rate array comes back to the host.  Returns (taus, stats): taus[n] the intervals of
        neuron n, the data sequences one after the other (the interval before the first event of a sequence is censored);
        stats (N, 4) summed over the sequences: expected count, event bins, event bins holding more than one spike, 0.
        A bin with several spikes is one event.  correct=True applies the discrete-time correction of Haslinger et al.
        (2010) to the event bin's term (pgl_rescale_corr) at the uniforms of (seed, draw): the intervals are then a random
        function of seed, the same bits for the same seed and draw; the default is the uncorrected sum."""
        parts = [[] for _ in range(self.N)]
        stats = np.zeros((self.N, 4))
        what = ("rescaled intervals", "are")
        for tau, off, st in self._per_sequence(vars, what, (lambda h, theta, Weff: h.rescale_corr(theta, Weff, seed, draw)) if correct else
                                              (lambda h, theta, Weff: h.rescale(theta, Weff))):
            for n in range(self.N):
                parts[n].append(tau[off[n]:off[n + 1]])
            stats += st
        return [np.concatenate(p) if p else np.zeros(0) for p in parts], stats

    # -- model comparison ------------------------------------------------------------------
    def compute_pointwise_ll(self, vars, block_chunks=1):
        """The log-likelihood of every neuron under `vars` resolved in time: sums of -dt lam_t + S[t,n] log lam_t over blocks
        of block_chunks * 256 consecutive bins (the last block of a sequence may be short), one forward pass and one
        segmented sum on the device per data sequence (pgl_pointwise).  Returns (n_blocks_total, N), the data sequences one
        after the other; a column sums to that neuron's ll.  Given the spike history the blocks are conditionally
        independent terms: the pointwise values of inference/model_compare.py."""
        parts = self._per_sequence(vars, ("the pointwise log-likelihood", "is"),
                                   lambda h, theta, Weff: h.pointwise(theta, Weff, block_chunks))
        return np.concatenate(parts, axis=0) if parts else np.zeros((0, self.N))

    # -- firing rates in time ----------------------------------------------------------------
    def compute_expected_counts(self, vars, win):
        """Expected and observed spike counts of every neuron under `vars` over windows of `win` consecutive bins (counted
        from the start of each data sequence; the last window of a sequence may be short): Lam = dt * sum of the rate over
        the window, obs = the recorded spikes in it.  One forward pass and one windowed sum on the device per data sequence
        (pgl_rate_windows); no rate array comes back to the host.  Returns (Lam, obs), each (n_win_total, N), the data
        sequences one after the other.  Lam / (win dt) is the firing rate plot_firing_rate draws from eval_state."""
        pairs = self._per_sequence(vars, ("the expected counts", "are"),
                                   lambda h, theta, Weff: h.rate_windows(theta, Weff, win))
        if not pairs:
            return np.zeros((0, self.N)), np.zeros((0, self.N))
        return np.concatenate([lam for lam, _ in pairs], axis=0), np.concatenate([obs for _, obs in pairs], axis=0)

    # -- stimulus decoding -------------------------------------------------------------------
    def _decode_point(self, vars, stim, mu, sigma, rho):
        """The device handle of the current data prepared at `vars` and evaluated at the stimulus `stim` (Tu, D)."""
        from theano_pyglm_amd.inference.decode import _served
        bk, data, q = _served(self)
        self._check_vars(vars)
        stim = self._stimulus_array(stim, bk.n_vars // bk.B, 'stim')
        h = self._handle(data)
        h.decode_prepare(self.theta_matrix(vars), self.W_eff(vars))
        return h, h.decode_eval(stim, q, (mu, sigma, rho))

    @staticmethod
    def _stimulus_array(a, D, name):
        """a as a float (Tu, D) array; a vector is one stimulus dimension.  ValueError where its columns are not the model's D."""
        a = np.asarray(a, dtype=float)
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2 or a.shape[1] != D:
            raise ValueError("%s must be (Tu, D) with D = %d stimulus dimensions, got %s" % (name, D, a.shape))
        return a

    def compute_stimulus_ll_grad(self, vars, stim, mu=0.0, sigma=1.0, rho=np.inf):
        """The decoding objective of the current data at the stimulus `stim` (Tu, D) on the stimulus grid, the spikes and `vars`
        fixed: returns (F (3,): log posterior of the stimulus up to a constant, log likelihood, log prior; its gradient with
        respect to the stimulus (Tu, D)), computed on the device (pgl_decode_eval).  The prior per stimulus dimension is
        Gaussian with mean mu and precision I / sigma^2 + Dt^T Dt / rho^2.  A 'basis' stimulus with dt_stim an integer
        multiple of dt only; other backgrounds and a time-sharded population raise ValueError."""
        return self._decode_point(vars, stim, mu, sigma, rho)[1]

    def compute_stimulus_hvp(self, vars, stim, v, mu=0.0, sigma=1.0, rho=np.inf):
        """The Hessian of that objective at `stim` times the direction v (Tu, D) (pgl_decode_hvp)."""
        from theano_pyglm_amd.inference.decode import _served
        bk = _served(self)[0]
        v = self._stimulus_array(v, bk.n_vars // bk.B, 'v')
        h, _ = self._decode_point(vars, stim, mu, sigma, rho)
        return h.decode_hvp(v)

    # -- state ---------------------------------------------------------------------------
    def eval_state(self, vars):
        """population.py:88-120: rates, currents and component state of every neuron."""
        state = {'latent': {}, 'net': self.network.get_state(vars['net'])}
        h = self._handle(self._current)
        W = self.W_eff(vars)
        glm_states = []
        for n in range(self.N):
            xn = vars['glms'][n]
            st = self.glm.get_state(xn)
            lam, inet, istim = h.state(n, self.glm.theta_row(xn), W[:, n])
            st['lam'] = lam
            st['I_bias'] = self.glm.bias_model.I_bias(xn['bias'])
            st['I_bkgd'] = istim if self.glm.Dstim > 0 else 0.0
            st['I_net'] = inet
            glm_states.append(st)
        state['glms'] = glm_states
        state['logprior'] = self.compute_log_prior(vars)
        state['ll'] = self.compute_ll(vars)
        state['logp'] = state['ll'] + state['logprior']
        return state

    # -- simulation ------------------------------------------------------------------------
    def _simulation_inputs(self, vars, T_range, dt, stim, dt_stim, nT=None):
        """population.py:252-282, shared by simulate and simulate_batch: X (nT, N) bias + stimulus current and
        AW (n_pre, n_post, R) = A * W * impulse.  nT: the number of bins where the caller knows it (a recording's length);
        default the reference's len(arange(T_start, T_stop, dt))."""
        T_start, T_stop = T_range
        N = self.N
        if nT is None:
            nT = len(np.arange(T_start, T_stop, dt))
        X = np.zeros((nT, N))
        for n in range(N):
            X[:, n] = self.glm.bias_model.I_bias(vars['glms'][n]['bias'])
        if self.glm.Dstim > 0:
            tmp = {'S': np.zeros((nT, N)), 'stim': stim, 'dt_stim': dt_stim, 'T': float(T_stop - T_start),
                   'dt': dt}
            fst = self.glm.bkgd_model.host_features(tmp, nT)
            for n in range(N):
                X[:, n] += fst.dot(self.glm.bkgd_model.dense_weights(vars['glms'][n]['bkgd']))
        # imps[n_pre, n_post, :] (population.py:275-282)
        imps = np.array([self.glm.imp_model.impulse(vars['glms'][n]['imp']) for n in range(N)])
        imps = np.transpose(imps, axes=[1, 0, 2])
        AW = self.W_eff(vars)[:, :, None] * imps              # (n_pre, n_post, R)
        return X, AW

    def simulate_batch(self, vars, T_range, dt, stim, dt_stim, n_rep, seed=0, rep0=0, spikes=True, currents=False,
                       device=True):
        """n_rep independent spike trains of the model at `vars`: simulate's algorithm on per-neuron threshold streams
        (the rule: include/pyglm_hip.h), one workgroup per replicate on the device (pgl_simulate_batch).  Replicate i
        uses stream index rep0 + i, so a batch equals its replicates run one at a time.  Returns a dict: S
        (n_rep, nT, N) uint8 (None unless spikes), X (n_rep, nT, N) total currents (None unless currents), counts
        (n_rep, N) spikes per neuron, exceptions (n_rep).  device=False loops the host reference pgl_simulate_streams.
        simulate keeps the reference's draw order; the two do not produce the same trains."""
        X0, AW = self._simulation_inputs(vars, T_range, dt, stim, dt_stim)
        AW = np.ascontiguousarray(np.transpose(AW, (0, 2, 1)))
        kind = self.glm.nlin_model.kind
        if device:
            return _lib.simulate_batch(X0, AW, kind, dt, n_rep, seed=seed, rep0=rep0, spikes=spikes, currents=currents,
                                       device=self.device)
        nT, N = X0.shape
        out = {'S': np.empty((n_rep, nT, N), dtype=np.uint8) if spikes else None,
               'X': np.empty((n_rep, nT, N)) if currents else None,
               'counts': np.empty((n_rep, N), dtype=np.int64), 'exceptions': np.empty(n_rep, dtype=np.int64)}
        for i in range(n_rep):
            S, X, n_exc, _ = _lib.simulate_streams(X0, AW, kind, dt, rep=rep0 + i, seed=seed)
            if spikes:
                out['S'][i] = S
            if currents:
                out['X'][i] = X
            out['counts'][i] = S.sum(axis=0, dtype=np.int64)
            out['exceptions'][i] = n_exc
        return out

    def simulate(self, vars, T_range, dt, stim, dt_stim, rng=None, verbose=False, native=True):
        """population.py:233-389: integrate-and-fire thinning with exponential thresholds;
        every spike adds A*W*impulse to X[t+1 : t+R+1] (351-353); <= 10 spikes per bin.
        Seeded (the reference uses the global np.random).  native=True runs the time loop in the
        C++ library (pgl_simulate, ~100x the Python loop, same draw order); native=False is the
        line-by-line Python restatement kept for cross-checking."""
        from theano_pyglm_amd.components.priors import _rng
        r = _rng(rng)
        N = self.N
        X, AW = self._simulation_inputs(vars, T_range, dt, stim, dt_stim)
        nT = X.shape[0]
        T_imp = AW.shape[2]
        if native:
            # uniforms in the reference's draw order come from `rng`; the library continues with
            # its own generator if the pre-drawn stream runs out
            n_draw = int(N + 4 * max(1.0, np.sum(self.glm.nlin_model.f_nlin(X)) * dt) + 1000)
            u = r.random_sample(min(n_draw, 50000000))
            seed = int(r.randint(0, 2 ** 31 - 1))
            S, X, n_exc = _lib.simulate(X, np.ascontiguousarray(np.transpose(AW, (0, 2, 1))),
                                        self.glm.nlin_model.kind, dt, uniforms=u, seed=seed)
            if verbose:
                print("Number of exceptions arising from multiple spikes per bin: %d" % n_exc)
            return S, X
        f_nlin = self.glm.nlin_model.f_nlin
        S = np.zeros((nT, N))
        acc = np.zeros(N)
        thr = -np.log(r.random_sample(N))
        n_exceptions = 0
        for t in range(nT):
            acc = acc + f_nlin(X[t, :]) * dt
            i_spk = acc > thr
            S[t, i_spk] += 1
            n_spk = int(np.sum(i_spk))
            t_imp = min(nT - t - 1, T_imp)
            while n_spk > 0:
                if np.any(S[t, :] >= 10):
                    n_exceptions += 1
                    break
                X[t + 1:t + t_imp + 1, :] += np.sum(AW[i_spk, :, :t_imp], 0).T
                acc -= thr * i_spk
                acc[acc < 0] = 0
                thr[i_spk] = -np.log(r.random_sample(n_spk))
                i_spk = acc > thr
                S[t, i_spk] += 1
                n_spk = int(np.sum(i_spk))
        if verbose:
            print("Number of exceptions arising from multiple spikes per bin: %d" % n_exceptions)
        return S, X
