"""NumPy restatement of the negative-binomial likelihood with a log link, an
exposure offset and a dispersion ("size") r on a centred design with an
intercept column: what csrc/negbin.hip is tested against.  The design tuple D
and its products are those of tests/logit_oracle.py; `OracleModel` has the
method names of the device model (bayesbridge_amd.model.NegBinModel), so that
the host logic of hmc.py, nuts.py, dispersion.py and the Gibbs driver can run
on it unchanged.

With t = eta + o - log r:
  ll_i    = G(y, r) - log y! + y t - (y + r) softplus(t)
  w_i     = y - (y + r) sigma(t)
  omega_i = (y + r) sigma(t) (1 - sigma(t))
  G(y, r) = sum_{j < y} log(r + j), here a long-double sum of logs."""
import math

import numpy as np

import poisson_oracle as po
from logit_oracle import design, dot, tdot, trajectory  # noqa: F401

LD = np.longdouble


def _fn(name, x):
    """np.<name>(x); on an object array (mpmath numbers: the limit test needs
    more digits than a long double has) mpmath's function of that name."""
    x = np.asarray(x)
    if x.dtype == object:
        import mpmath
        return np.frompyfunc(getattr(mpmath, name), 1, 1)(x)
    return getattr(np, name)(x)


def softplus(x):
    return np.maximum(x, 0) + _fn('log1p', _fn('exp', -np.abs(x)))


def sigma(x):
    e = _fn('exp', -np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def row_weights(eta_o, y, r):
    """w = y - (y + r) sigma(t), t = eta_o - log r, in the precision of its
    arguments."""
    t = eta_o - _fn('log', r)
    return y - (y + r) * sigma(t)


def G(y, r):
    """sum_{j < y} log(r + j) per row in long double, rounded once at the
    end; r a scalar."""
    y = np.asarray(y, dtype=np.float64)
    r = LD(r)
    top = int(y.max()) if y.size else 0
    logs = np.log(r + np.arange(top, dtype=LD))
    cum = np.concatenate(([LD(0)], np.cumsum(logs)))
    return cum[y.astype(np.intp)]


def _t(D, log_exposure, beta, r):
    return (dot(D, beta) + log_exposure) - math.log(r)


def beta_part(D, y, log_exposure, beta, r):
    """y t - (y + r) softplus(t) per row."""
    with np.errstate(invalid='ignore', over='ignore'):
        t = _t(D, log_exposure, beta, r)
        return y * t - (y + r) * softplus(t)


def loglik_grad(D, y, log_exposure, beta, r):
    """The part of the log-likelihood that depends on beta, and its
    gradient."""
    with np.errstate(invalid='ignore', over='ignore'):
        t = _t(D, log_exposure, beta, r)
        loglik = np.sum(y * t - (y + r) * softplus(t))
        grad = tdot(D, y - (y + r) * sigma(t))
    return float(loglik), grad


def hessian_matvec(D, y, log_exposure, beta, v, r):
    s = sigma(_t(D, log_exposure, beta, r))
    return tdot(D, -(((y + r) * (s * (1. - s))) * dot(D, v)))


def dispersion_loglik(D, y, log_exposure, beta, r):
    """L(r) = sum_i G(y_i, r) + y_i t_i - (y_i + r) softplus(t_i), summed in
    long double; r a scalar or an array."""
    eta_o = (dot(D, beta) + log_exposure).astype(LD)
    out = []
    for rk in np.atleast_1d(r):
        rk = LD(rk)
        t = eta_o - np.log(rk)
        sp = np.maximum(t, 0) + np.log1p(np.exp(-np.abs(t)))
        out.append(float(np.sum(G(y, rk) + y * t - (y + rk) * sp)))
    return out[0] if np.ndim(r) == 0 else np.array(out)


def full_loglik_rows(eta_o, y, r):
    """Every term of a row's log density, in long double: eta_o = eta + o."""
    from scipy.special import gammaln
    eta_o = np.asarray(eta_o, dtype=LD)
    r = LD(r)
    t = eta_o - np.log(r)
    sp = np.maximum(t, 0) + np.log1p(np.exp(-np.abs(t)))
    return G(y, r) - gammaln(y + 1.).astype(LD) + y * t - (y + r) * sp


def precond_f(D, y, log_exposure, scale, prior_prec, r):
    """f(q) of the preconditioned coordinates (reg_coef_sampler.py:259-279) on
    the oracle likelihood; no gradient where logp is not finite."""
    def f(q):
        ll, g = loglik_grad(D, y, log_exposure, q * scale, r)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def newton_mle(D, y, log_exposure, r, n_iter=100):
    """The maximum-likelihood coefficients at a fixed r and the inverse of the
    observed information there."""
    P = D[0].shape[1] + int(D[2])
    eye = np.eye(P)
    beta = np.zeros(P)
    if D[2]:
        beta[0] = math.log(y.sum() / np.exp(log_exposure).sum())
    ll, grad = loglik_grad(D, y, log_exposure, beta, r)
    for _ in range(n_iter):
        info = -np.column_stack([
            hessian_matvec(D, y, log_exposure, beta, e, r) for e in eye])
        step = np.linalg.solve(info, grad)
        # the likelihood is concave in beta: halve a step that overshoots
        for _ in range(40):
            new_ll, new_grad = loglik_grad(D, y, log_exposure, beta + step, r)
            if new_ll >= ll or np.abs(step).max() < 1e-13:
                break
            step = step / 2
        beta, ll, grad = beta + step, new_ll, new_grad
        if np.abs(step).max() < 1e-13:
            break
    return beta, np.linalg.inv(info)


class OracleModel(po.OracleModel):
    """The negative-binomial model on the host.  `design` is only handed on
    (the Gibbs driver reads its shape and its intercept flag).  `perturb`: a
    relative perturbation of the likelihood, the gradient and L(r), for the
    choice of chain seeds whose path does not hang on the last bits."""
    name = 'negbin'

    def __init__(self, D, y, log_exposure, design=None, dispersion=None,
                 dispersion_prior=None, perturb=0.):
        super().__init__(D, y, log_exposure, design)
        self.dispersion_fixed = dispersion is not None
        self.dispersion = 1. if dispersion is None else float(dispersion)
        self.dispersion_prior = dispersion_prior or {'shape': 2., 'rate': .1}
        self.perturb = perturb
        self._beta = None

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = loglik_grad(self.D, self.y, self.log_exposure,
                               np.asarray(beta, dtype=np.float64),
                               self.dispersion)
        if ll == -math.inf:
            return -math.inf, None
        ll, grad = ll * (1. + self.perturb), grad * (1. + self.perturb)
        return ll, (None if loglik_only else grad)

    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        beta, r = np.array(beta, dtype=np.float64), self.dispersion
        return lambda v: hessian_matvec(self.D, self.y, self.log_exposure,
                                        beta, np.ravel(v), r)

    def dispersion_loglik(self, coef, r):
        if coef is not None:
            self._beta = np.array(coef, dtype=np.float64)
        out = dispersion_loglik(self.D, self.y, self.log_exposure, self._beta,
                                r)
        return out * (1. + self.perturb)

    def _f(self, scale, prior_prec):
        base = precond_f(self.D, self.y, self.log_exposure,
                         np.asarray(scale, dtype=np.float64),
                         np.asarray(prior_prec, dtype=np.float64),
                         self.dispersion)
        if not self.perturb:
            return base

        def f(q):
            logp, grad = base(q)
            return logp * (1. + self.perturb), \
                (None if grad is None else grad * (1. + self.perturb))
        return f


# ---- prediction: the forms of tests/predict_oracle.py for this family -------

def _predict_terms(Xt, coef, dispersion, y, offset, dtype):
    """(mu, ll or None), each (n, S): mu = exp(eta), ll the full log density
    with the dispersion of draw s."""
    from scipy.special import gammaln
    import predict_oracle as pro
    eta = pro._eta(Xt, coef, offset, dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        mu = np.exp(eta)
        if y is None:
            return mu, None
        y = np.asarray(y, dtype=np.float64)
        ll = np.empty(eta.shape, dtype=dtype)
        for s, r in enumerate(np.asarray(dispersion, dtype=np.float64)):
            r = dtype(r)
            t = eta[:, s] - np.log(r)
            sp = np.maximum(t, 0) + np.log1p(np.exp(-np.abs(t)))
            ll[:, s] = G(y, r).astype(dtype) + y * t - (y + r) * sp \
                + (-gammaln(y + 1.)).astype(dtype)
    return mu, ll


def predict_explicit(Xt, coef, dispersion, y=None, offset=None):
    """predict_oracle.explicit for the negative-binomial model."""
    mu, ll = _predict_terms(Xt, coef, dispersion, y, offset, LD)
    S = mu.shape[1]
    mean = mu.sum(axis=1) / S
    res = {'mean': mean, 'mu': mu,
           'sd': np.sqrt(((mu - mean[:, None]) ** 2).sum(axis=1) / S)}
    if ll is not None:
        top = ll.max(axis=1)
        res.update({
            'lpd': top + np.log(np.exp(ll - top[:, None]).sum(axis=1))
            - np.log(LD(S)),
            'loglik_mean': ll.sum(axis=1) / S,
            'loglik_var': ll.var(axis=1, ddof=1), 'll': ll})
    return res


def predict_recurrence(Xt, coef, dispersion, y=None, offset=None):
    """predict_oracle.recurrence for the negative-binomial model: the
    device's float64 updates, one per draw in draw order."""
    mu, ll = _predict_terms(Xt, coef, dispersion, y, offset, np.float64)
    n, S = mu.shape
    mean, m2 = np.zeros(n), np.zeros(n)
    lmean, lm2 = np.zeros(n), np.zeros(n)
    lmax, lsum = np.full(n, -np.inf), np.zeros(n)
    for s in range(S):
        k = float(s + 1)
        delta = mu[:, s] - mean
        mean = mean + delta / k
        m2 = m2 + delta * (mu[:, s] - mean)
        if ll is None:
            continue
        x = ll[:, s]
        delta = x - lmean
        lmean = lmean + delta / k
        lm2 = lm2 + delta * (x - lmean)
        up = x > lmax
        with np.errstate(over='ignore', invalid='ignore'):
            lsum = np.where(up, lsum * np.exp(lmax - x) + 1.,
                            lsum + np.exp(x - lmax))
        lmax = np.where(up, x, lmax)
    res = {'mean': mean, 'sd': np.sqrt(m2 / S), 'mu': mu}
    if ll is not None:
        res.update({'lpd': lmax + np.log(lsum) - math.log(S),
                    'loglik_mean': lmean, 'loglik_var': lm2 / (S - 1.),
                    'll': ll})
    return res
