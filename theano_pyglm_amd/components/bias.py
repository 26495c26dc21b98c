"""Bias current of a GLM neuron: a single scalar with a Gaussian prior
(behavioural counterpart of pyglm/components/bias.py: I_bias = bias[0], :32;
log p = -(bias - mu)^2 / (2 sigma^2), :33; sample = mu + sigma * randn(1), :51-56)."""
import numpy as np

from theano_pyglm_amd.components.component import Component
from theano_pyglm_amd.components.priors import _rng


class ConstantBias(Component):
    def __init__(self, model):
        self.set_hyperparameters(model['bias'])

    def set_hyperparameters(self, model):
        self.mu_bias, self.sig_bias = model['mu'], model['sigma']

    def get_variables(self):
        return {'bias': (1,)}

    @staticmethod
    def I_bias(vars):
        b = vars['bias']
        try:
            return float(b[0])
        except (TypeError, IndexError):
            return float(np.ravel(b)[0])

    def _z(self, vars):
        return (self.I_bias(vars) - self.mu_bias) / self.sig_bias

    def log_p(self, vars):
        return -0.5 * self._z(vars) ** 2

    def log_p_all(self, vars_list):
        z = (np.array([self.I_bias(v) for v in vars_list]) - self.mu_bias) / self.sig_bias
        return float(-0.5 * np.sum(z ** 2))

    def grad_log_p(self, vars):
        return {'bias': np.array([-self._z(vars) / self.sig_bias])}

    def hess_log_p_vec(self, vars, v):
        """Hessian of log_p (bias.py:33) times v = {'bias': ..}: -v / sig_bias^2."""
        return {'bias': -np.asarray(v['bias'], dtype=float).reshape(-1) / self.sig_bias ** 2}

    def get_state(self, vars=None):
        return {'bias': vars['bias']} if vars is not None else {}

    def sample(self, acc, rng=None):
        return {'bias': self.mu_bias + self.sig_bias * _rng(rng).standard_normal(1)}


def create_bias_component(model, glm, latent):
    kind = model['bias']['type'].lower()
    if kind != 'constant':
        raise Exception("Unrecognized bias model: %s" % kind)
    return ConstantBias(model)
