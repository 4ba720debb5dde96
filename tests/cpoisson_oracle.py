"""NumPy restatement of the conditional Poisson likelihood (counts with one
nuisance baseline rate per stratum, conditioned on the stratum totals) on a
design without an intercept column: what csrc/cpoisson.hip is tested against.
Rows are stratum-major, stratum s is rows stratum_ptr[s] .. stratum_ptr[s + 1]
- 1.  The design tuple D and its products are those of tests/logit_oracle.py;
`OracleModel` has the method names of the device models
(bayesbridge_amd.model._DeviceHamiltonian), so that the host logic of hmc.py,
nuts.py and the Gibbs driver can run on it unchanged.

    a_i = eta_i + o_i,  L_s = log sum_{j in s} exp(a_j),  N_s = sum_{i in s} y_i
    ll = sum_i y_i (a_i - L_s(i)),  pi_i = exp(a_i - L_s),  w_i = y_i - N_s pi_i
"""
import math

import numpy as np

import poisson_oracle as po
from logit_oracle import design, dot, tdot, trajectory  # noqa: F401


def stratum_ptr_of(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def _per_row(values, sptr):
    return np.repeat(values, np.diff(sptr))


def _pieces(D, y, log_exposure, sptr, beta):
    """a, L_s per row and N_s per row."""
    a = dot(D, beta) + log_exposure
    with np.errstate(invalid='ignore'):
        lse = np.logaddexp.reduceat(a, sptr[:-1])
    total = np.add.reduceat(y, sptr[:-1])
    return a, _per_row(lse, sptr), _per_row(total, sptr)


def loglik_grad(D, y, log_exposure, sptr, beta):
    """sum y (a - L_s) and X~^T (y - N_s pi); the multinomial coefficient is
    dropped.  The log-sum-exp is taken stratum by stratum (np.logaddexp), so
    there is no overflow case."""
    a, lse, total = _pieces(D, y, log_exposure, sptr, beta)
    with np.errstate(invalid='ignore'):
        loglik = np.sum(y * (a - lse))
        grad = tdot(D, y - total * np.exp(a - lse))
    return float(loglik), grad


def hessian_matvec(D, y, log_exposure, sptr, beta, v):
    """X~^T (-(N_s pi (u - ubar_s))), u = X~ v, ubar_s = sum_s pi u."""
    a, lse, total = _pieces(D, y, log_exposure, sptr, beta)
    pi = np.exp(a - lse)
    u = dot(D, v)
    ubar = _per_row(np.add.reduceat(pi * u, sptr[:-1]), sptr)
    return tdot(D, -(total * pi * (u - ubar)))


def loglik_grad_global_max(D, y, log_exposure, sptr, beta):
    """The mutant of the shift test: ONE max over all rows instead of one per
    stratum.  A stratum far below the top one has every exp equal to 0."""
    a = dot(D, beta) + log_exposure
    total = _per_row(np.add.reduceat(y, sptr[:-1]), sptr)
    with np.errstate(all='ignore'):
        h = np.exp(a - a.max())
        s = _per_row(np.add.reduceat(h, sptr[:-1]), sptr)
        loglik = np.sum(y * ((a - a.max()) - np.log(s)))
        grad = tdot(D, y - total * (h / s))
    return float(loglik), grad


def precond_f(D, y, log_exposure, sptr, scale, prior_prec):
    """f(q) of the preconditioned coordinates (reg_coef_sampler.py:259-279) on
    the oracle likelihood; no gradient where logp is not finite."""
    def f(q):
        ll, g = loglik_grad(D, y, log_exposure, sptr, q * scale)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def newton_mle(D, y, log_exposure, sptr, n_iter=50):
    """The conditional maximum-likelihood coefficients and the inverse of the
    observed information there, by Newton iterations from 0."""
    assert not D[2]
    P = D[0].shape[1]
    eye = np.eye(P)
    beta = np.zeros(P)
    for _ in range(n_iter):
        _, grad = loglik_grad(D, y, log_exposure, sptr, beta)
        info = -np.column_stack([
            hessian_matvec(D, y, log_exposure, sptr, beta, e) for e in eye])
        step = np.linalg.solve(info, grad)
        beta = beta + step
        if np.abs(step).max() < 1e-13:
            break
    return beta, np.linalg.inv(info)


class OracleModel(po.OracleModel):
    """The conditional Poisson model on the host: poisson_oracle.OracleModel
    (its trajectory and its tree) on this file's likelihood."""

    def __init__(self, D, y, log_exposure, stratum_ptr, design=None):
        assert not D[2]
        super().__init__(D, y, log_exposure, design=design)
        self.stratum_ptr = np.asarray(stratum_ptr, dtype=np.int64)

    def calc_intercept_mle(self):
        raise NotImplementedError("the model has no intercept")

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = loglik_grad(self.D, self.y, self.log_exposure,
                               self.stratum_ptr,
                               np.asarray(beta, dtype=np.float64))
        return ll, (None if loglik_only else grad)

    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        beta = np.array(beta, dtype=np.float64)
        return lambda v: hessian_matvec(self.D, self.y, self.log_exposure,
                                        self.stratum_ptr, beta, np.ravel(v))

    def _f(self, scale, prior_prec):
        return precond_f(self.D, self.y, self.log_exposure, self.stratum_ptr,
                         np.asarray(scale, dtype=np.float64),
                         np.asarray(prior_prec, dtype=np.float64))
