"""NumPy restatement of the Weibull proportional-hazards likelihood of
right-censored times on a centred design with an intercept column: what
csrc/weibull.hip and csrc/weibull_predict.hip are tested against.  The design
tuple D and its products are those of tests/logit_oracle.py; `OracleModel`
has the method names of the device model (bayesbridge_amd.model.WeibullModel),
so that the host logic of hmc.py, nuts.py, weibull_shape.py and the Gibbs
driver can run on it unchanged.

Rows (d, lt): d = 1 for an event, lt = log t; shape k.  In the association
the device states (a product is rounded before the sum it enters):
  m    = exp(eta + (k * lt))
  ll   = (d * eta) - m                                  the beta-part
  w    = d - m
  full = d * ((log k + ((k - 1) * lt)) + eta) - m       the whole log density
  med  = exp((log(log 2) - eta) / k)                    the median time
Every function takes a dtype: np.float64 mirrors the device, np.longdouble is
the reference the tolerances are measured against."""
import math

import numpy as np

import poisson_oracle as po
from logit_oracle import design, dot, tdot, trajectory  # noqa: F401

LD = np.longdouble
LOG_LOG2 = math.log(math.log(2.))


def _rows(eta, d, lt, k, dtype):
    """(eta, d, lt, k, log k) in dtype; log k is the float64 log rounded as
    the device receives it when dtype is float64, and the long-double log
    otherwise."""
    k = dtype(k)
    logk = dtype(math.log(float(k))) if dtype is np.float64 else np.log(k)
    return (np.asarray(eta, dtype=dtype), np.asarray(d, dtype=dtype),
            np.asarray(lt, dtype=dtype), k, logk)


def row_m(eta, lt, k, dtype=np.float64):
    eta, _, lt, k, _ = _rows(eta, 0., lt, k, dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.exp(eta + (k * lt))


def row_beta_part(eta, d, lt, k, dtype=np.float64):
    """(ll, w) per row."""
    eta, d, lt, k, _ = _rows(eta, d, lt, k, dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        m = np.exp(eta + (k * lt))
        return d * eta - m, d - m


def row_full(eta, d, lt, k, dtype=np.float64):
    """The whole log density per row."""
    eta, d, lt, k, logk = _rows(eta, d, lt, k, dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        m = np.exp(eta + (k * lt))
        return d * ((logk + ((k - 1) * lt)) + eta) - m


def median(eta, k, dtype=np.float64):
    eta = np.asarray(eta, dtype=dtype)
    c = dtype(LOG_LOG2) if dtype is np.float64 else np.log(np.log(LD(2)))
    with np.errstate(over='ignore'):
        return np.exp((c - eta) / dtype(k))


def loglik_grad(D, d, lt, beta, k, dtype=np.float64):
    """The part of the log-likelihood that depends on beta, and its gradient
    (the products with the design are float64's; the rows' terms and their
    sums are in dtype)."""
    eta = dot(D, beta)
    ll, w = row_beta_part(eta, d, lt, k, dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        if dtype is np.float64:
            return float(np.sum(ll)), tdot(D, w)
        return np.sum(ll), _tdot_ld(D, w)


def _dense(D):
    """X~ as a long-double matrix (tests' sizes only)."""
    X, offset, intercept = D[0], D[1], D[2]
    A = np.asarray(X.todense() if hasattr(X, 'todense') else X, dtype=LD)
    if offset is not None:
        A = A - np.asarray(offset, dtype=LD)[None, :]
    if intercept:
        A = np.hstack((np.ones((A.shape[0], 1), dtype=LD), A))
    return A


def _tdot_ld(D, w):
    return _dense(D).T.dot(np.asarray(w, dtype=LD))


def eta_ld(D, beta):
    return _dense(D).dot(np.asarray(beta, dtype=LD))


def hessian_matvec(D, d, lt, beta, v, k, dtype=np.float64):
    if dtype is np.float64:
        m = row_m(dot(D, beta), lt, k)
        with np.errstate(over='ignore', invalid='ignore'):
            return tdot(D, -(m * dot(D, v)))
    m = row_m(eta_ld(D, beta), lt, k, LD)
    return _tdot_ld(D, -(m * eta_ld(D, v)))


def shape_loglik(D, d, lt, beta, k, dtype=np.float64, eta=None):
    """L(k) = sum_i full_i; k a scalar or an array."""
    if eta is None:
        eta = dot(D, beta)
    out = []
    for kj in np.atleast_1d(k):
        with np.errstate(over='ignore', invalid='ignore'):
            s = np.sum(row_full(eta, d, lt, kj, dtype))
        out.append(float(s) if dtype is np.float64 else s)
    if np.ndim(k) == 0:
        return out[0]
    return np.array(out, dtype=dtype)


def precond_f(D, d, lt, scale, prior_prec, k):
    """f(q) of the preconditioned coordinates (reg_coef_sampler.py:259-279) on
    the oracle likelihood; no gradient where logp is not finite."""
    def f(q):
        ll, g = loglik_grad(D, d, lt, q * scale, k)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def newton_mle(D, d, lt, k, n_iter=100):
    """The maximum-likelihood coefficients at a fixed k and the inverse of
    the observed information there."""
    P = D[0].shape[1] + int(D[2])
    eye = np.eye(P)
    beta = np.zeros(P)
    if D[2]:
        beta[0] = math.log(d.sum() / np.exp(k * lt).sum())
    ll, grad = loglik_grad(D, d, lt, beta, k)
    for _ in range(n_iter):
        info = -np.column_stack([
            hessian_matvec(D, d, lt, beta, e, k) for e in eye])
        step = np.linalg.solve(info, grad)
        # the likelihood is concave in beta: halve a step that overshoots
        for _ in range(40):
            new_ll, new_grad = loglik_grad(D, d, lt, beta + step, k)
            if new_ll >= ll or np.abs(step).max() < 1e-13:
                break
            step = step / 2
        beta, ll, grad = beta + step, new_ll, new_grad
        if np.abs(step).max() < 1e-13:
            break
    return beta, np.linalg.inv(info)


class OracleModel(po.OracleModel):
    """The Weibull model on the host.  `design` is only handed on (the Gibbs
    driver reads its shape and its intercept flag).  `perturb`: a relative
    perturbation of the likelihood, the gradient and L(k), for the choice of
    chain seeds whose path does not hang on the last bits."""
    name = 'weibull'

    def __init__(self, D, event, log_time, design=None, shape=None,
                 shape_prior=None, perturb=0.):
        super().__init__(D, event, log_time, design)
        self.event = self.y
        self.log_time = self.log_exposure
        self.time = np.exp(self.log_time)
        self.shape_fixed = shape is not None
        self.shape = 1. if shape is None else float(shape)
        self.shape_prior = shape_prior or {'shape': 2., 'rate': 1.}
        self.perturb = perturb
        self._beta = None

    def calc_intercept_mle(self):
        return math.log(self.event.sum() / np.sum(self.time ** self.shape))

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = loglik_grad(self.D, self.event, self.log_time,
                               np.asarray(beta, dtype=np.float64), self.shape)
        if ll == -math.inf:
            return -math.inf, None
        ll, grad = ll * (1. + self.perturb), grad * (1. + self.perturb)
        return ll, (None if loglik_only else grad)

    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        beta, k = np.array(beta, dtype=np.float64), self.shape
        return lambda v: hessian_matvec(self.D, self.event, self.log_time,
                                        beta, np.ravel(v), k)

    def shape_loglik(self, coef, k):
        if coef is not None:
            self._beta = np.array(coef, dtype=np.float64)
        out = shape_loglik(self.D, self.event, self.log_time, self._beta, k)
        return out * (1. + self.perturb)

    def _f(self, scale, prior_prec):
        base = precond_f(self.D, self.event, self.log_time,
                         np.asarray(scale, dtype=np.float64),
                         np.asarray(prior_prec, dtype=np.float64), self.shape)
        if not self.perturb:
            return base

        def f(q):
            logp, grad = base(q)
            return logp * (1. + self.perturb), \
                (None if grad is None else grad * (1. + self.perturb))
        return f


# ---- prediction -------------------------------------------------------------

def predict_terms(eta, shape, event=None, log_time=None, dtype=LD):
    """(median, ll or None), each (n, S), from eta (n, S) and one shape per
    draw."""
    eta = np.asarray(eta, dtype=dtype)
    med = np.empty(eta.shape, dtype=dtype)
    ll = None if event is None else np.empty(eta.shape, dtype=dtype)
    for s, k in enumerate(np.asarray(shape, dtype=np.float64)):
        med[:, s] = median(eta[:, s], k, dtype)
        if ll is not None:
            ll[:, s] = row_full(eta[:, s], event, log_time, k, dtype)
    return med, ll


def predict_explicit(eta, shape, event=None, log_time=None, dtype=LD):
    """mean, sd and, with an outcome, lpd, loglik_mean, loglik_var by their
    definitions (two passes) in dtype."""
    mu, ll = predict_terms(eta, shape, event, log_time, dtype)
    S = mu.shape[1]
    mean = mu.sum(axis=1) / S
    res = {'mean': mean, 'mu': mu,
           'sd': np.sqrt(((mu - mean[:, None]) ** 2).sum(axis=1) / S)}
    if ll is not None:
        top = ll.max(axis=1)
        res.update({
            'lpd': top + np.log(np.exp(ll - top[:, None]).sum(axis=1))
            - np.log(dtype(S)),
            'loglik_mean': ll.sum(axis=1) / S,
            'loglik_var': ll.var(axis=1, ddof=1), 'll': ll})
    return res


def survival(eta, shape, times, dtype=LD):
    """S[i][t][s] = exp(-exp(k_s log t + eta[i][s])), its mean and population
    sd over the draws; the exponent is the one sum (k_s log t) + eta, with
    k_s log t rounded to float64 first, as the host forms it."""
    eta = np.asarray(eta, dtype=dtype)
    lh = (np.asarray(shape, dtype=np.float64)[:, None]
          * np.log(np.asarray(times, dtype=np.float64))[None, :])   # (S, T)
    expo = lh.T.astype(dtype)[None, :, :] + eta[:, None, :]
    with np.errstate(over='ignore'):
        surv = np.exp(-np.exp(expo))
    mean = surv.sum(axis=2) / surv.shape[2]
    sd = np.sqrt(((surv - mean[:, :, None]) ** 2).sum(axis=2)
                 / surv.shape[2])
    return {'mean': mean, 'sd': sd, 'draws': surv}


def predict_recurrence(eta, shape, event=None, log_time=None):
    """The device's float64 updates, one per draw in draw order (the
    accumulators' contract of csrc/predict_summary.hpp)."""
    mu, ll = predict_terms(eta, shape, event, log_time, np.float64)
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
