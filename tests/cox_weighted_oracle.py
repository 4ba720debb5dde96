"""NumPy oracle of the Cox partial likelihood with case weights (Breslow's
rule for ties): what csrc/cox_weighted.hip is tested against.  Two forms:

  * `explicit`: the n_event x n risk-set matrix M[k, i] = [row i's event or
    censoring time >= t_k], defined from the times alone, and
        loglik = sum_k a_k ((eta_k - m) - log H_k),  H = M g,
        g = a exp(eta - m),
    everything after X beta and X v in np.longdouble (n <= 2049);
  * `scans`: the device's structure in linear time -- the suffix sum of g over
    the events, the prefix sum over the censored rows, q = a (1/H), c = cumsum q,
    z = a ((1/H) ((1/H) S)) -- in float64 or np.longdouble, for any n.

Rows are in cox_preprocess's order.  X is the raw host matrix: the partial
likelihood does not change when a column is centred.  idx = (n_event, start,
end, n_app, weights): cox_risk_sets' arrays and the weights in row order.
`OracleModel` has the method names of the device models
(bayesbridge_amd.model._DeviceHamiltonian), so that the host logic of hmc.py,
nuts.py and the Gibbs driver can run on it unchanged."""
import math

import numpy as np

import cox_interval_oracle as cio
from cox_oracle import risk_sums

LD = np.longdouble
EXPLICIT_MAX_N = 2049
_tdot_ld = cio._tdot_ld


def index_arrays(event_time, censoring_time, weights):
    """idx of sorted rows, by the package's own helper."""
    from bayesbridge_amd.model import cox_risk_sets
    n_event, start, end, n_app = cox_risk_sets(event_time, censoring_time)
    weights = np.asarray(weights, dtype=np.float64)
    assert weights.shape == (len(n_app),)
    return n_event, start, end, n_app, weights


def replicate(event_time, censoring_time, X, weights):
    """The rows written weights[i] times each (integer weights), still in the
    model's order: the copies of a row are adjacent and share its times."""
    rep = np.asarray(weights).astype(np.int64)
    assert np.array_equal(rep, weights) and rep.min() >= 1
    rows = np.repeat(np.arange(len(rep)), rep)
    return event_time[rows], censoring_time[rows], X[rows]


# ----------------------------------------------------------- explicit form
def _explicit(X, beta, event_time, censoring_time, weights):
    """(d = eta - m, g, M, H, a, is_event) in long double."""
    event_time = np.asarray(event_time, dtype=np.float64)
    x = np.minimum(event_time, np.asarray(censoring_time, dtype=np.float64))
    assert len(x) <= EXPLICIT_MAX_N
    is_event = np.isfinite(event_time)
    a = np.asarray(weights, dtype=np.float64).astype(LD)
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(LD)
    d = eta - np.max(eta)
    g = a * np.exp(d)
    M = (x[None, :] >= event_time[is_event][:, None]).astype(LD)
    return d, g, M, M @ g, a, is_event


def explicit_loglik(X, beta, event_time, censoring_time, weights):
    d, g, M, H, a, is_event = _explicit(X, beta, event_time, censoring_time,
                                        weights)
    if np.any(H == 0.):
        return -math.inf
    return float(np.sum(a[is_event] * (d[is_event] - np.log(H))))


def explicit_loglik_grad(X, beta, event_time, censoring_time, weights):
    d, g, M, H, a, is_event = _explicit(X, beta, event_time, censoring_time,
                                        weights)
    if np.any(H == 0.):
        return -math.inf, None
    ak = a[is_event]
    ll = np.sum(ak * (d[is_event] - np.log(H)))
    w = np.where(is_event, a, LD(0.)) - g * (M.T @ (ak / H))
    return float(ll), _tdot_ld(X, w)


def explicit_hessian_matvec(X, beta, v, event_time, censoring_time, weights):
    """-sum_k a_k X^T (diag(p_k) - p_k p_k^T) X v, p_k = M[k] g / H_k."""
    d, g, M, H, a, is_event = _explicit(X, beta, event_time, censoring_time,
                                        weights)
    ak = a[is_event]
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(LD)
    mean_u = (M @ (g * u)) / H                       # p_k . u
    r = g * u * (M.T @ (ak / H)) - g * (M.T @ (ak * mean_u / H))
    return _tdot_ld(X, -r)


# -------------------------------------------------------------- scan form
def scans_loglik_grad(X, beta, idx, dtype=np.float64):
    n_event, start, end, n_app, weights = idx
    a = weights.astype(dtype)
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    d = eta - np.max(eta)
    g = a * np.exp(d)
    H = risk_sums(g, n_event, start, end)
    if np.any(H == 0.):
        return -math.inf, None
    ak = a[:n_event]
    ll = np.sum(ak * (d[:n_event] - np.log(H)))
    c = np.cumsum(ak * (1. / H))
    w = -(c[n_app - 1] * g)
    w[:n_event] += ak
    if dtype is np.float64:
        grad = np.asarray(X.T @ w, dtype=np.float64).ravel()
    else:
        grad = _tdot_ld(X, w)
    return float(ll), grad


def scans_hessian_matvec(X, beta, v, idx, dtype=np.float64):
    n_event, start, end, n_app, weights = idx
    a = weights.astype(dtype)
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    g = a * np.exp(eta - np.max(eta))
    inv = 1. / risk_sums(g, n_event, start, end)
    ak = a[:n_event]
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(dtype)
    S = risk_sums(g * u, n_event, start, end)
    c = np.cumsum(ak * inv)
    cz = np.cumsum(ak * (inv * (inv * S)))
    k = n_app - 1
    r = (c[k] * g) * u - g * cz[k]
    if dtype is np.float64:
        return np.asarray(X.T @ (-r), dtype=np.float64).ravel()
    return _tdot_ld(X, -r)


def precond_f(X, scale, prior_prec, idx):
    """f(q) of the preconditioned coordinates (reg_coef_sampler.py:259-279) on
    the oracle likelihood; no gradient where logp is not finite."""
    def f(q):
        ll, g = scans_loglik_grad(X, q * scale, idx)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


class OracleModel(cio.OracleModel):
    """The weighted Cox model on the host: cox_interval_oracle's OracleModel
    (trajectory, tree) on this module's likelihood."""

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = scans_loglik_grad(self.X, np.asarray(beta,
                                                        dtype=np.float64),
                                     self.idx)
        if ll == -math.inf:
            return -math.inf, None
        return ll, (None if loglik_only else grad)

    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        beta = np.array(beta, dtype=np.float64)
        if self.compute_loglik_and_gradient(beta)[0] == -math.inf:
            raise ValueError('Hessian operator cannot be computed')
        return lambda v: scans_hessian_matvec(self.X, beta, np.ravel(v),
                                              self.idx)

    def _f(self, scale, prior_prec):
        return precond_f(self.X, np.asarray(scale, dtype=np.float64),
                         np.asarray(prior_prec, dtype=np.float64), self.idx)


# ---------------------------------------------------------------- test data
def make_times(X, seed=0, censor_frac=.4, n_grid=None):
    """Unsorted (event, censoring) for the rows of X: exponential times under
    a sparse true coefficient vector; with n_grid, on a grid of that many
    points, so that events tie and censoring times tie event times."""
    rs = np.random.RandomState(seed)
    n, p = X.shape
    beta = np.zeros(p)
    beta[:min(p, 5)] = rs.randn(min(p, 5)) * .5
    t = rs.exponential(np.exp(-np.asarray(X @ beta).ravel()))
    if n_grid:
        edges = np.quantile(t, np.linspace(0, 1, n_grid + 1)[1:])
        t = 1. + np.searchsorted(edges, t, side='left').clip(max=n_grid - 1)
    cens = rs.rand(n) < censor_frac
    return np.where(cens, np.inf, t), np.where(cens, t, np.inf)


def newton_mle(X, idx, n_iter=50):
    """The maximum-partial-likelihood coefficients by Newton iterations from
    0 (dense X, few columns)."""
    P = X.shape[1]
    beta = np.zeros(P)
    for _ in range(n_iter):
        _, grad = scans_loglik_grad(X, beta, idx)
        info = -np.column_stack([scans_hessian_matvec(X, beta, e, idx)
                                 for e in np.eye(P)])
        step = np.linalg.solve(info, grad)
        beta = beta + step
        if np.abs(step).max() < 1e-13:
            break
    return beta
