"""Stimulus decoding: the most probable stimulus given a fitted population and its recorded spikes (the decoding half of Pillow
et al., Nature 454 (2008) 995-999).  The reference has no counterpart: its graph has no derivative with respect to the stimulus.

The rule (include/pyglm_hip.h, "Stimulus decoding"; csrc/pglm_decode.h).  The unknown u (Tu, D) lives on the stimulus grid,
dt_stim = q dt.  s = L u is np.interp onto the bin grid, K[tau, d, n] = sum_b basis[tau, b] w_stim[n, d B + b] the filters,
I = K * s the strictly causal stimulus current, x = c + I with c = bias + the currents of the recorded spikes, and
    F(u)   = sum_t sum_n [S log lam(x) - dt lam(x)] + log p(u)
    grad F = L^T K^T r + grad log p(u),         r  = S (log lam)'(x) - dt lam'(x)
    H v    = L^T K^T (cc o (K L v)) + hess log p . v,   cc = S (log lam)''(x) - dt lam''(x)
with a Gaussian prior per stimulus dimension: mean mu, precision I / sigma^2 + Dt^T Dt / rho^2 (Dt: first differences in time;
rho = inf: iid).  DecodeProblem is the readable numpy statement of that rule; decode_stimulus maximises F with scipy's
Newton-CG on the device's gradient and Hessian-vector products (pgl_decode_eval / pgl_decode_hvp): only u and the results
cross to the device and back per iteration.

Served: the 'basis' stimulus (BasisStimulus), exp and explinear, the current data sequence, dt_stim an integer multiple of dt.
Not built: the posterior covariance of the decoded stimulus (a banded Cholesky of -H), 'spatiotemporal' stimuli, non-integer
dt_stim / dt, a frame-rate filter that folds L into K for large q, several data sequences at once."""
import numpy as np


def frames_per_bin(dt_stim, dt):
    """q = dt_stim / dt where it is an integer >= 1; ValueError otherwise."""
    ratio = float(dt_stim) / float(dt)
    q = int(round(ratio))
    if q < 1 or abs(ratio - q) > 1e-9 * max(ratio, 1.0):
        raise ValueError("stimulus decoding needs dt_stim to be an integer multiple of dt (dt_stim / dt = %r)" % ratio)
    return q


class DecodeProblem(object):
    """The numpy statement.  c, S (nT, N); basis (Rt, B); w_stim (N, D B) with column d B + b; prior (mu, sigma, rho)."""

    def __init__(self, c, S, basis, w_stim, D, nlin, dt, q, mu=0.0, sigma=1.0, rho=np.inf):
        if nlin not in ('exp', 'explinear'):
            raise ValueError("stimulus decoding: unknown nonlinearity %r" % (nlin,))
        self.c = np.asarray(c, dtype=float)
        self.S = np.asarray(S, dtype=float)
        self.nT, self.N = self.c.shape
        basis = np.asarray(basis, dtype=float)
        self.Rt, B = basis.shape
        self.D, self.nlin, self.dt, self.q = int(D), nlin, float(dt), int(q)
        self.K = np.einsum('tb,ndb->tdn', basis, np.asarray(w_stim, dtype=float).reshape(self.N, self.D, B))
        self.mu, self.a = float(mu), 1.0 / float(sigma) ** 2
        self.b = 1.0 / float(rho) ** 2 if np.isfinite(rho) and rho > 0 else 0.0
        self.cc = None

    # -- L and L^T: np.interp of the frames onto the bins, clamped behind the last frame
    def _plan(self, Tu):
        t = np.arange(self.nT)
        i, r = t // self.q, t % self.q
        clamp = i >= Tu - 1
        w1 = np.where(clamp, 0.0, r / float(self.q))
        return np.where(clamp, Tu - 1, i), np.where(clamp, Tu - 1, i + 1), 1.0 - w1, w1

    def L(self, u):
        i0, i1, w0, w1 = self._plan(u.shape[0])
        return w0[:, None] * u[i0] + w1[:, None] * u[i1]

    def Lt(self, g, Tu):
        i0, i1, w0, w1 = self._plan(Tu)
        out = np.zeros((Tu, g.shape[1]))
        np.add.at(out, i0, w0[:, None] * g)
        np.add.at(out, i1, w1[:, None] * g)
        return out

    # -- K * and K^T: strictly causal, s = 0 before bin 0, rows past nT zero
    def conv(self, s):
        I = np.zeros((self.nT, self.N))
        for tau in range(min(self.Rt, self.nT - 1)):
            I[tau + 1:] += s[:self.nT - 1 - tau] @ self.K[tau]
        return I

    def corr(self, y):
        g = np.zeros((self.nT, self.D))
        for tau in range(min(self.Rt, self.nT - 1)):
            g[:self.nT - 1 - tau] += y[tau + 1:] @ self.K[tau].T
        return g

    def rate(self, x):
        return np.exp(x) if self.nlin == 'exp' else np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))

    def _point(self, x):
        """ll terms, r and cc of every element"""
        S, dt = self.S, self.dt
        if self.nlin == 'exp':
            lam = np.exp(x)
            return S * x - dt * lam, S - dt * lam, -dt * lam
        e = np.exp(-np.abs(x))
        lam = np.maximum(x, 0.0) + np.log1p(e)
        sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        d2 = e / (1.0 + e) ** 2                                   # lam'' = sig (1 - sig)
        # (log lam)'' = sig / lam^2 ((1 - sig) lam - sig); for x < 0, (1 - sig) lam - sig = (log1p(z) - z) / (1 + z), z = e^x
        z = np.where(x < 0, e, 0.0)
        ser = np.zeros_like(z)
        for k in range(12, 1, -1):
            ser = (-1.0) ** (k + 1) / k + z * ser
        lm = np.where(z < 0.05, z * z * ser, np.log1p(z) - z)
        inner = np.where(x >= 0, e / (1.0 + e) * lam - sig, lm / (1.0 + e))
        with np.errstate(divide='ignore', invalid='ignore'):
            loglam = np.where(S > 0, np.log(lam), 0.0)
            h = sig / (lam * lam) * inner
        return S * loglam - dt * lam, (S / lam - dt) * sig, np.where(S > 0, S * h, 0.0) - dt * d2

    def _prior(self, u, center):
        """(log p terms summed, the linear part: gradient at center = mu, product at center = 0)"""
        dev = u - center
        diff = u[1:] - u[:-1]
        lin = -self.a * dev
        lin[1:] -= self.b * diff
        lin[:-1] += self.b * diff
        return -0.5 * self.a * np.sum(dev * dev) - 0.5 * self.b * np.sum(diff * diff), lin

    def eval(self, u, want_grad=True):
        """((F, log likelihood, log prior), grad (Tu, D) or None) at u (Tu, D)"""
        u = np.asarray(u, dtype=float)
        term, r, self.cc = self._point(self.c + self.conv(self.L(u)))
        ll = float(np.sum(term))
        lp, lin = self._prior(u, self.mu)
        g = self.Lt(self.corr(r), u.shape[0]) + lin if want_grad else None
        return np.array([ll + lp, ll, lp]), g

    def hvp(self, v):
        """H v at the point of the last eval"""
        v = np.asarray(v, dtype=float)
        _, lin = self._prior(v, 0.0)
        return self.Lt(self.corr(self.cc * self.conv(self.L(v))), v.shape[0]) + lin


def _served(population):
    """(BasisStimulus model, current data, q) or ValueError, worded like the other drivers"""
    from theano_pyglm_amd.components.bkgd import BasisStimulus
    bk = population.glm.bkgd_model
    if getattr(population, '_time_shard', None) is not None:
        raise ValueError("stimulus decoding of a time-sharded population is not implemented")
    if not isinstance(bk, BasisStimulus):
        raise ValueError("stimulus decoding is not implemented for the %s background (it needs the 'basis' stimulus)"
                         % type(bk).__name__)
    data = population._current
    if data is None:
        raise ValueError("stimulus decoding: no data sequence has been set")
    if data.get('fstim', None) is not None:
        raise ValueError("stimulus decoding is not implemented for caller-supplied stimulus features (data['fstim'])")
    q = frames_per_bin(bk.bkgd_model.get('dt_stim', data['dt_stim']), population.glm.dt)
    return bk, data, q


def numpy_problem(population, vars, mu=0.0, sigma=1.0, rho=np.inf):
    """The DecodeProblem of the population's current data under `vars`: the offset c from eval_state-free host arithmetic
    (bias + the coupling currents of the recorded spikes through convolve_with_basis)."""
    from theano_pyglm_amd.utils import basis as bs
    bk, data, q = _served(population)
    theta = population.theta_matrix(vars)
    Weff = population.W_eff(vars)
    S = np.asarray(data['S'], dtype=float)
    nT, N = S.shape
    imp = population.glm.imp_model
    Dst = bk.n_vars
    fS = bs.convolve_with_basis(S, imp.ibasis)                                   # (nT, N, B)
    W = theta[:, 1 + Dst:].reshape(N, N, imp.B) * Weff.T[:, :, None]             # [n, n', b]
    c = theta[None, :, 0] + np.einsum('tmb,nmb->tn', fS, W)
    D = Dst // bk.B
    return DecodeProblem(c, S, bk.ibasis, theta[:, 1:1 + Dst], D, population.glm.nlin_model.kind, population.glm.dt, q, mu, sigma,
                         rho), data, D


def decode_stimulus(population, x, stim0=None, mu=0.0, sigma=1.0, rho=np.inf, method='newton-cg', maxiter=200, gtol=1e-5,
                    device=True):
    """The MAP stimulus of the population's current data sequence given its spikes and the parameters x.  Maximises F with
    scipy's Newton-CG (method='newton-cg': the driver of fit_glm(use_rop=True)) or L-BFGS ('l-bfgs') on the device's gradient
    and Hessian-vector products (device=True: pgl_decode_eval / pgl_decode_hvp) or on the numpy statement (device=False).
    stim0 (Tu, D): the start, default the prior mean.  Returns a dict: 'stim' (Tu, D), 'F', 'log_lik', 'log_prior',
    'grad_max' (max |grad F| at the result), 'n_eval', 'n_hvp', 'status' (0: grad_max <= gtol) and 'route'."""
    import scipy.optimize as opt
    if method not in ('newton-cg', 'l-bfgs'):
        raise ValueError("decode_stimulus: method must be 'newton-cg' or 'l-bfgs'")
    bk, data, q = _served(population)
    Tu = int(np.asarray(data['stim']).shape[0])
    D = bk.n_vars // bk.B
    prior = (float(mu), float(sigma), float(rho))
    if device:
        h = population._handle(data)
        h.decode_prepare(population.theta_matrix(x), population.W_eff(x))
        evaluate = lambda u, want_grad=True: h.decode_eval(u, q, prior, want_grad)
        product = h.decode_hvp
        route = 'device (pgl_decode_eval, pgl_decode_hvp)'
    else:
        prob, _, _ = numpy_problem(population, x, mu, sigma, rho)
        evaluate, product = prob.eval, prob.hvp
        route = 'numpy'
    counts = {'eval': 0, 'hvp': 0}
    point = {'z': None}                               # where r and cc of the last evaluation stand

    def at(z, want_grad=True):
        counts['eval'] += 1
        point['z'] = np.array(z, dtype=float)
        return evaluate(z.reshape(Tu, D), want_grad)

    def fun(z):                                       # scipy minimises: -F and -grad F
        F, g = at(z)
        return -F[0], -g.ravel()

    def hessp(z, v):                                  # the products are taken at the point of the last evaluation: where scipy
        if point['z'] is None or not np.array_equal(point['z'], z):     # asks at another point, that point is evaluated first
            at(z, want_grad=False)
        counts['hvp'] += 1
        return -product(v.reshape(Tu, D)).ravel()

    if stim0 is None:
        z = np.full(Tu * D, float(mu))
    else:
        z = np.array(stim0, dtype=float)
        if z.shape != (Tu, D) and not (D == 1 and z.shape == (Tu,)):
            raise ValueError("decode_stimulus: stim0 must be (Tu, D) = (%d, %d), got %s" % (Tu, D, z.shape))
        z = z.reshape(Tu * D)
    F, g = at(z)
    # Newton-CG stops on the step length, not on the gradient: rounds with a tighter xtol until max |grad| <= gtol
    xtol = 1e-8
    left = int(maxiter)
    while np.max(np.abs(g)) > gtol and left > 0:
        if method == 'newton-cg':
            res = opt.minimize(fun, z, jac=True, hessp=hessp, method='Newton-CG', options={'xtol': xtol, 'maxiter': left})
        else:
            res = opt.minimize(fun, z, jac=True, method='L-BFGS-B', options={'gtol': gtol * 0.5, 'ftol': 0.0, 'maxiter': left,
                                                                            'maxcor': 20})
        left -= max(int(res.nit), 1)
        z = res.x
        F, g = at(z)
        xtol *= 1e-3
        if xtol < 1e-16:
            break
    grad_max = float(np.max(np.abs(g)))
    return {'stim': z.reshape(Tu, D).copy(), 'F': float(F[0]), 'log_lik': float(F[1]), 'log_prior': float(F[2]), 'grad_max': grad_max,
            'n_eval': counts['eval'], 'n_hvp': counts['hvp'], 'status': 0 if grad_max <= gtol else 1, 'route': route}
