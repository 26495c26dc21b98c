"""
Glm -- one generalized linear model shared by all neurons (counterpart of pyglm/glm.py).

    x_t   = I_bias + I_stim[t] + sum_n' W_eff[n',n] * I_imp[t,n']      glm.py:39-45
    ll_n  = sum_t( -dt*nlin(x_t) + log(nlin(x_t)) * S[t,n] )           glm.py:52
    log_p = lkhd_scale * ll + log_prior                                  glm.py:55-63

The reference builds these as Theano expressions; here the data-dependent part (ll and
its gradient) is evaluated by the HIP kernels on the flat feature-weight row `theta_row`
and everything that only touches <= N*B numbers (priors, chain rules) is numpy.
"""
import numpy as np

from theano_pyglm_amd.components.component import Component
from theano_pyglm_amd.components.bias import create_bias_component
from theano_pyglm_amd.components.bkgd import create_bkgd_component
from theano_pyglm_amd.components.impulse import create_impulse_component
from theano_pyglm_amd.components.nlin import create_nlin_component
from theano_pyglm_amd.utils.syms import Sym, from_shapes

_PARTS = ('bias', 'bkgd', 'imp', 'nlin')


class Glm(Component):
    def __init__(self, model, network, latent):
        self.model = model
        self.network = network
        self.dt = model['dt']                      # glm.py:16 (KeyError without dt, like the reference)
        self.N = model['N']
        self.bias_model = create_bias_component(model, self, latent)
        self.bkgd_model = create_bkgd_component(model, self, latent)
        self.imp_model = create_impulse_component(model, self, latent)
        self.nlin_model = create_nlin_component(model)
        self.lkhd_scale = 1.0

    def _part(self, key):
        return {'bias': self.bias_model, 'bkgd': self.bkgd_model, 'imp': self.imp_model,
                'nlin': self.nlin_model}[key]

    # -- variables ----------------------------------------------------------
    def get_variables(self):
        """glm.py:65-73."""
        v = {'n': Sym('n', (), 'int64')}
        for k in _PARTS:
            v[k] = from_shapes(self._part(k).get_variables())
        return v

    def sample(self, acc, rng=None):
        """glm.py:119-129."""
        v = {'n': -1}
        for k in _PARTS:
            v[k] = self._part(k).sample(acc, rng=rng)
        return v

    def set_hyperparameters(self, model):
        """glm.py:112-117."""
        self.bkgd_model.set_hyperparameters(model['bkgd'])
        self.imp_model.set_hyperparameters(model['impulse'])
        self.bias_model.set_hyperparameters(model['bias'])

    def preprocess_data(self, data):
        for k in _PARTS:
            self._part(k).preprocess_data(data)

    # -- host-side pieces ---------------------------------------------------
    def log_prior(self, xn):
        """glm.py:55-59 on the per-neuron dict xn = {'bias':..,'bkgd':..,'imp':..,'nlin':..}."""
        return (self.bias_model.log_p(xn['bias']) + self.bkgd_model.log_p(xn['bkgd']) +
                self.imp_model.log_p(xn['imp']) + self.nlin_model.log_p(xn.get('nlin', {})))

    def log_prior_all(self, glms):
        """sum_n log_prior(glms[n]) with every component evaluated over all neurons at once (rounding order differs from the
        per-neuron sum by a few ulp)."""
        return (self.bias_model.log_p_all([g['bias'] for g in glms]) + self.bkgd_model.log_p_all([g['bkgd'] for g in glms]) +
                self.imp_model.log_p_all([g['imp'] for g in glms]) + self.nlin_model.log_p_all([g.get('nlin', {}) for g in glms]))

    def grad_log_prior(self, xn):
        return {'n': {}, 'bias': self.bias_model.grad_log_p(xn['bias']),
                'bkgd': self.bkgd_model.grad_log_p(xn['bkgd']),
                'imp': self.imp_model.grad_log_p(xn['imp']), 'nlin': {}}

    def hvp_packing(self):
        """None when Hessian-vector products are served for this model: the packed per-neuron vector is a permutation of
        the device's theta row (constant bias, no or basis stimulus, linear-basis impulses under a Gaussian or
        group-lasso prior).  Else the name of the packing that is not -- its second-order chain terms (w_t (x) w_x,
        |g| / sum|g|) are not implemented."""
        from theano_pyglm_amd.components.bias import ConstantBias
        from theano_pyglm_amd.components.bkgd import NoStimulus, BasisStimulus
        from theano_pyglm_amd.components.impulse import LinearBasisImpulses
        from theano_pyglm_amd.components.priors import Gaussian, GroupLasso
        if not isinstance(self.bias_model, ConstantBias):
            return type(self.bias_model).__name__
        if not isinstance(self.bkgd_model, (NoStimulus, BasisStimulus)):
            return type(self.bkgd_model).__name__
        if not isinstance(self.imp_model, LinearBasisImpulses):
            return type(self.imp_model).__name__
        if not isinstance(self.imp_model.prior, (Gaussian, GroupLasso)):
            return type(self.imp_model.prior).__name__
        return None

    def hess_log_prior_vec(self, xn, v):
        """Hessian of log_prior(xn) times v (a dict shaped like the differentiable part of xn), shaped like
        grad_log_prior; the counterpart of the prior terms inside hessian_rop_wrt_list (grads.py:68-95)."""
        return {'n': {}, 'bias': self.bias_model.hess_log_p_vec(xn['bias'], v['bias']),
                'bkgd': self.bkgd_model.hess_log_p_vec(xn['bkgd'], v.get('bkgd', {})),
                'imp': self.imp_model.hess_log_p_vec(xn['imp'], v['imp']), 'nlin': {}}

    def hess_log_prior(self, xn):
        """Dense Hessian of log_prior(xn) w.r.t. the packed per-neuron vector, (P, P): the matrix whose columns are
        hess_log_prior_vec of the unit vectors (the prior terms inside hessian_wrt_list, grads.py:30-66).  The served priors
        are sums over single weights and over the B-weight groups of the impulse model, so B products recover every
        column: product k probes element k of every impulse group (and, k = 0, every other weight) at once."""
        from theano_pyglm_amd.utils.packvec import packdict, unpackdict, get_vars
        from theano_pyglm_amd.utils.syms import differentiable
        bad = self.hvp_packing()
        if bad is not None:
            raise ValueError("Hessian-vector products are not implemented for the %s packing" % bad)
        syms =differentiable(self.get_variables())
        w0, shapes = packdict(get_vars(syms, xn))
        P = w0.size
        where = unpackdict(np.arange(P), shapes)                # packed position of every variable's elements
        imp = np.asarray(where['imp']['w_ir']).reshape(self.N, self.imp_model.B)
        rest = np.setdiff1d(np.arange(P), imp.reshape(-1))
        H = np.zeros((P, P))
        for k in range(self.imp_model.B):
            v = np.zeros(P)
            v[imp[:, k]] = 1.0
            if k == 0:
                v[rest] = 1.0
            hv = packdict(get_vars(syms, self.hess_log_prior_vec(xn, unpackdict(v, shapes))))[0]
            H[imp, imp[:, k][:, None]] = hv[imp]                # rows of each group, column = its probed element
            if k == 0:
                H[rest, rest] = hv[rest]
        return H

    @property
    def Dstim(self):
        return self.bkgd_model.n_features

    @property
    def P(self):
        return 1 + self.Dstim + self.N * self.imp_model.B

    def theta_row(self, xn):
        """Flat feature weights [bias, w_stim, w_imp] consumed by the device (pyglm_hip.h)."""
        return np.concatenate(([self.bias_model.I_bias(xn['bias'])],
                               self.bkgd_model.flat_weights(xn['bkgd']),
                               self.imp_model.flat_weights(xn['imp'])))

    def theta_rows(self, glms):
        """theta_row of every listed neuron as one (n, P) matrix, filled by column blocks."""
        D = self.Dstim
        th = np.empty((len(glms), self.P))
        for i, g in enumerate(glms):
            th[i, 0] = self.bias_model.I_bias(g['bias'])
            if D:
                th[i, 1:1 + D] = self.bkgd_model.flat_weights(g['bkgd'])
            th[i, 1 + D:] = self.imp_model.flat_weights(g['imp'])
        return th

    def chain_grad(self, xn, g_theta):
        """Flat-weight gradient of ll (from the device) -> gradient w.r.t. the model's own
        variables, as a nested dict shaped like the differentiable part of xn."""
        D = self.Dstim
        return {'n': {}, 'bias': {'bias': np.array([g_theta[0]])},
                'bkgd': self.bkgd_model.chain_grad(xn['bkgd'], g_theta[1:1 + D]),
                'imp': self.imp_model.chain_grad(xn['imp'], g_theta[1 + D:]),
                'nlin': {}}

    def get_state(self, xn=None):
        """glm.py:75-91 (the time series lam / I_net / I_bkgd are filled in by Population)."""
        return {'bias': self.bias_model.get_state(None if xn is None else xn['bias']),
                'bkgd': self.bkgd_model.get_state(None if xn is None else xn['bkgd']),
                'imp': self.imp_model.get_state(None if xn is None else xn['imp']),
                'nlin': {}}
