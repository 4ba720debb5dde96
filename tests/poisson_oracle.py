"""NumPy restatement of the Poisson likelihood with a log link and an exposure
offset on a centred design with an intercept column: what csrc/poisson.hip is
tested against.  The design tuple D and its products are those of
tests/logit_oracle.py; `OracleModel` has the method names of the device models
(bayesbridge_amd.model._DeviceHamiltonian), so that the host logic of hmc.py,
nuts.py and the Gibbs driver can run on it unchanged."""
import math

import numpy as np

import logit_oracle as lo
import nuts_oracle as no
from logit_oracle import design, dot, tdot, trajectory  # noqa: F401


def loglik_grad(D, y, log_exposure, beta):
    """sum y eta - mu and X~^T (y - mu), mu = exp(eta + log_exposure); the
    terms constant in beta (sum y o - log y!) are dropped."""
    eta = dot(D, beta)
    with np.errstate(over='ignore', invalid='ignore'):
        mu = np.exp(eta + log_exposure)
        loglik = np.sum(y * eta - mu)
        grad = tdot(D, y - mu)
    return float(loglik), grad


def hessian_matvec(D, y, log_exposure, beta, v):
    with np.errstate(over='ignore'):
        mu = np.exp(dot(D, beta) + log_exposure)
    return tdot(D, -(mu * dot(D, v)))


def precond_f(D, y, log_exposure, scale, prior_prec):
    """f(q) of the preconditioned coordinates (reg_coef_sampler.py:259-279) on
    the oracle likelihood; no gradient where logp is not finite."""
    def f(q):
        ll, g = loglik_grad(D, y, log_exposure, q * scale)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def newton_mle(D, y, log_exposure, n_iter=50):
    """The maximum-likelihood coefficients and the inverse of the observed
    information there, by Newton iterations from the intercept-only fit."""
    P = D[0].shape[1] + int(D[2])
    eye = np.eye(P)
    beta = np.zeros(P)
    if D[2]:
        beta[0] = math.log(y.sum() / np.exp(log_exposure).sum())
    for _ in range(n_iter):
        _, grad = loglik_grad(D, y, log_exposure, beta)
        info = -np.column_stack([
            hessian_matvec(D, y, log_exposure, beta, e) for e in eye])
        step = np.linalg.solve(info, grad)
        beta = beta + step
        if np.abs(step).max() < 1e-13:
            break
    return beta, np.linalg.inv(info)


class _NoGradient(Exception):
    """A leapfrog step was asked for from a state without a gradient."""


class _Missing():
    """Stands for the gradient where logp is not finite."""

    def __rmul__(self, other):
        raise _NoGradient()


class OracleModel():
    """The Poisson model on the host.  `design` is only handed on (the Gibbs
    driver reads its shape and its intercept flag); every likelihood value
    comes from D = lo.design(...)."""
    name = 'poisson'

    def __init__(self, D, y, log_exposure, design=None):
        self.D = D
        self.y = np.asarray(y, dtype=np.float64)
        self.log_exposure = np.asarray(log_exposure, dtype=np.float64)
        self.design = design
        self.n_obs = D[0].shape[0]
        self.n_pred = D[0].shape[1] + int(D[2])
        self.intercept_added = D[2]

    def calc_intercept_mle(self):
        return np.log(self.y.sum() / np.exp(self.log_exposure).sum())

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = loglik_grad(self.D, self.y, self.log_exposure,
                               np.asarray(beta, dtype=np.float64))
        if ll == -math.inf:
            return -math.inf, None
        return ll, (None if loglik_only else grad)

    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        beta = np.array(beta, dtype=np.float64)
        return lambda v: hessian_matvec(self.D, self.y, self.log_exposure,
                                        beta, np.ravel(v))

    def _f(self, scale, prior_prec):
        return precond_f(self.D, self.y, self.log_exposure,
                         np.asarray(scale, dtype=np.float64),
                         np.asarray(prior_prec, dtype=np.float64))

    def hmc_trajectory(self, dt, n_step, precond_scale, prior_prec, q0, p0,
                       logp0, grad0, hamiltonian_tol=100.):
        f = self._f(precond_scale, prior_prec)
        q, p, logp, grad, n_grad, instab, h0, h1 = lo.trajectory(
            f, dt, n_step, np.asarray(q0, dtype=np.float64),
            np.asarray(p0, dtype=np.float64), logp0,
            np.asarray(grad0, dtype=np.float64), hamiltonian_tol)
        return {'q': q, 'p': p, 'logp': logp,
                'grad': grad if math.isfinite(logp) else None,
                'n_steps': n_grad, 'instability': bool(instab),
                'hamiltonian': np.array([h0, h1])}

    # The tree of nuts_oracle on f.  Where the likelihood overflows there is
    # no gradient to take the next step with: the device ends the half-tree
    # there as unstable (max H = inf reaches the main tree, the doubling is
    # rejected); an overflow at the last step of a subtree is merged as usual
    # and terminates that subtree through max H = inf.
    def nuts_begin(self, precond_scale, prior_prec, q0, p0, logp0, grad0,
                   joint_logp0, joint_logp_threshold, hamiltonian_tol=100.):
        base = self._f(precond_scale, prior_prec)

        def f(q):
            logp, grad = base(q)
            return logp, (_Missing() if grad is None else grad)

        self._sh = no.Shared(f, None, joint_logp0, joint_logp_threshold,
                             hamiltonian_tol, None)
        self._tree = no.Tree(
            self._sh, np.array(q0, dtype=np.float64),
            np.array(p0, dtype=np.float64), logp0,
            np.array(grad0, dtype=np.float64), joint_logp0)

    def nuts_doubling(self, dt, direction, height, uniforms):
        sh, tree = self._sh, self._tree
        pool = list(uniforms)
        assert len(pool) == 2 ** height
        sh.dt, sh.uniform = dt, lambda: pool.pop(0)
        sh.n_step = sh.n_uniform = 0
        try:
            rejected = tree.double(height, direction)
        except _NoGradient:
            tree.hmax, rejected = math.inf, True
        return {'n_uniform': sh.n_uniform, 'n_steps': sh.n_step,
                'u_turn_detected': bool(tree.u_turn),
                'instability_detected': bool(tree.unstable),
                'doubling_rejected': bool(rejected),
                'height': tree.height, 'n_acceptable_state': tree.n_acc,
                'ave_hamiltonian_error': float(tree.err),
                'ave_accept_prob': float(tree.acc)}

    def nuts_sample(self):
        q, logp, grad = self._tree.sample
        return q, logp, grad
