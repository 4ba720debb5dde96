"""NumPy restatement of the binomial-logit likelihood on a centred design with
an intercept column (model/logistic_model.py:49-74, the design of
design_matrix/abstract_matrix.py): what csrc/logit.hip is tested against.

A design is the tuple D = (X, offset, intercept): X the host matrix (NumPy or
SciPy; for float32 storage the rounded matrix), offset the column means that
centre it (None: not centred), intercept whether X~ has a leading column of
ones."""
import math

import numpy as np


def design(X, center=True, intercept=True, offset=None):
    if center and offset is None:
        offset = np.asarray(X.mean(axis=0), dtype=np.float64).ravel()
    return X, (offset if center else None), bool(intercept)


def dot(D, beta):
    X, offset, intercept = D
    b = beta[1:] if intercept else beta
    out = np.asarray(X.dot(b), dtype=np.float64).ravel()
    if offset is not None:
        out = out - np.dot(offset, b)
    if intercept:
        out = out + beta[0]
    return out


def tdot(D, w):
    X, offset, intercept = D
    out = np.asarray(X.T.dot(w), dtype=np.float64).ravel()
    if offset is not None:
        out = out - offset * np.sum(w)
    if intercept:
        out = np.concatenate(([np.sum(w)], out))
    return out


def loglik_grad(D, n_success, n_trial, beta):
    eta = dot(D, beta)
    with np.errstate(over='ignore'):
        loglik = np.sum(n_success * eta - n_trial * np.logaddexp(0, eta))
        prob = 1 / (1 + np.exp(-eta))
    return float(loglik), tdot(D, n_success - n_trial * prob)


def hessian_matvec(D, n_success, n_trial, beta, v):
    with np.errstate(over='ignore'):
        prob = 1 / (1 + np.exp(-dot(D, beta)))
    weight = prob * (1 - prob)
    return -tdot(D, n_trial * weight * dot(D, v))


def precond_f(D, n_success, n_trial, scale, prior_prec):
    """f(q) of reg_coef_sampler.py:259-279 on the oracle likelihood."""
    def f(q):
        ll, g = loglik_grad(D, n_success, n_trial, q * scale)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def trajectory(f, dt, n_step, q0, p0, logp0, grad0, tol=100.):
    """simulate_dynamics (hmc.py:137-174) with velocity_verlet: returns q, p,
    logp, grad, n_grad_evals, instability and the first / last Hamiltonian."""
    def ham(logp, p):
        return -logp + 0.5 * np.dot(p, p)
    q, p, logp, grad = q0, p0, logp0, grad0
    h0 = ham(logp0, p0)
    hmin = hmax = h0
    n_grad, instab, hcur = 0, False, h0
    for _ in range(n_step):
        p = p + 0.5 * dt * grad
        q = q + dt * p
        logp, g = f(q)
        if math.isfinite(logp):
            grad = g
            p = p + 0.5 * dt * grad
        hcur = ham(logp, p)
        hmin, hmax = min(hmin, hcur), max(hmax, hcur)
        n_grad += 1
        instab = math.isinf(logp) or (hmax - hmin) > tol
        if instab:
            break
    return q, p, logp, grad, n_grad, instab, h0, hcur
