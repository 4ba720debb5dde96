"""NumPy oracle of the Cox partial likelihood with Efron's approximation for
tied event times: what csrc/cox_efron.hip is tested against.  Two forms:

  * `explicit`: a loop over the distinct event times with the set D of the
    events at t, the set R of the rows whose event or censoring time is >= t
    and the terms log(H - (l/d) T), l = 0 .. d-1 (H the hazard of R, T that of
    D), everything after the data in np.longdouble (n <= 2049);
  * `scans`: the device's structure in linear time -- the suffix sum E over
    the events, the prefix sum C over the censored rows, phi = R + a T, the
    cumulative sums c and cb -- in float64 or np.longdouble, for any n.

Rows are in cox_preprocess's order.  X is the raw host matrix: the partial
likelihood does not change when a column is centred.  idx = (n_event, start,
end, n_app, gsize): cox_risk_sets' arrays and cox_tie_groups' group sizes.
`OracleModel` has the method names of the device models
(bayesbridge_amd.model._DeviceHamiltonian), so that the host logic of hmc.py,
nuts.py and the Gibbs driver can run on it unchanged."""
import math

import numpy as np

import cox_interval_oracle as cio

LD = np.longdouble
EXPLICIT_MAX_N = 2049
_tdot_ld = cio._tdot_ld


def tie_groups_by_loops(event_time):
    """(gstart, gsize) of every event of sorted rows, from the definition;
    O(n_event^2)."""
    t = [x for x in np.asarray(event_time, dtype=np.float64)
         if math.isfinite(x)]
    gstart = [min(j for j in range(len(t)) if t[j] == tk) for tk in t]
    gsize = [sum(1 for tj in t if tj == tk) for tk in t]
    return np.array(gstart, dtype=np.int64), np.array(gsize, dtype=np.int64)


def index_arrays(event_time, censoring_time):
    """idx of sorted rows, by the package's own helpers."""
    from bayesbridge_amd.model import cox_risk_sets, cox_tie_groups
    n_event, start, end, n_app = cox_risk_sets(event_time, censoring_time)
    gstart, gsize = cox_tie_groups(event_time)
    assert np.array_equal(gstart, start)
    return n_event, start, end, n_app, gsize


# ----------------------------------------------------------- explicit form
def _explicit_terms(X, beta, event_time, censoring_time):
    """Yields (phi, weight) of every event, in long double: phi = H - (l/d) T
    and weight_i = the share of row i's hazard in phi (1 on R \\ D, 1 - l/d on
    D, 0 elsewhere), for l = 0 .. d-1 at every distinct event time."""
    event_time = np.asarray(event_time, dtype=np.float64)
    x = np.minimum(event_time, np.asarray(censoring_time, dtype=np.float64))
    assert len(x) <= EXPLICIT_MAX_N
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(LD)
    dev = eta - np.max(eta)
    h = np.exp(dev)
    for t in np.unique(event_time[np.isfinite(event_time)]):
        in_r = (x >= t).astype(LD)
        in_d = (event_time == t).astype(LD)
        d = int(in_d.sum())
        H, T = np.sum(in_r * h), np.sum(in_d * h)
        for l in range(d):
            frac = LD(l) / LD(d)
            yield H - frac * T, in_r - frac * in_d, h, dev


def explicit_loglik(X, beta, event_time, censoring_time):
    ll, dev = LD(0.), None
    for phi, _, _, dev in _explicit_terms(X, beta, event_time,
                                          censoring_time):
        if phi <= 0.:
            return -math.inf
        ll -= np.log(phi)
    ll += np.sum(dev[np.isfinite(np.asarray(event_time, dtype=np.float64))])
    return float(ll)


def explicit_loglik_grad(X, beta, event_time, censoring_time):
    ll = explicit_loglik(X, beta, event_time, censoring_time)
    if ll == -math.inf:
        return ll, None
    w = np.isfinite(np.asarray(event_time, dtype=np.float64)).astype(LD)
    for phi, weight, h, _ in _explicit_terms(X, beta, event_time,
                                             censoring_time):
        w = w - weight * h / phi
    return ll, _tdot_ld(X, w)


def explicit_hessian_matvec(X, beta, v, event_time, censoring_time):
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(LD)
    r = np.zeros(len(u), dtype=LD)
    for phi, weight, h, _ in _explicit_terms(X, beta, event_time,
                                             censoring_time):
        p = weight * h / phi
        r += p * u - p * np.sum(p * u)
    return _tdot_ld(X, -r)


# -------------------------------------------------------------- scan form
def _phi_sums(arr, idx, ties):
    """R_g + a_k T_g of every event from the two scans of arr (ties =
    'breslow': R_g + T_g)."""
    n_event, start, end, n_app, gsize = idx
    zero = arr.dtype.type(0)
    E = np.concatenate((np.cumsum(arr[:n_event][::-1])[::-1], [zero]))
    C = np.concatenate((np.zeros(n_event, dtype=arr.dtype),
                        np.cumsum(arr[n_event:])))
    nxt = start + gsize
    R = E[nxt] + np.where(end >= n_event, C[end], zero)
    T = E[start] - E[nxt]
    if ties == 'breslow':
        return R + T
    return R + (1. - _frac(idx, arr.dtype)) * T


def _frac(idx, dtype):
    n_event, start, end, n_app, gsize = idx
    return ((np.arange(n_event) - start).astype(dtype)
            / np.asarray(gsize).astype(dtype))


def _cum_at(inv, idx, ties):
    """A_i (or Z_i) of every row from inv (or z)."""
    n_event, start, end, n_app, gsize = idx
    A = np.cumsum(inv)[n_app - 1]
    if ties == 'efron':
        cb0 = np.concatenate(([inv.dtype.type(0)],
                              np.cumsum(_frac(idx, inv.dtype) * inv)))
        A[:n_event] = A[:n_event] - (cb0[start + gsize] - cb0[start])
    return A


def scans_loglik_grad(X, beta, idx, dtype=np.float64, ties='efron'):
    n_event = idx[0]
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    d = eta - np.max(eta)
    h = np.exp(d)
    phi = _phi_sums(h, idx, ties)
    if np.any(phi <= 0.):
        return -math.inf, None
    ll = np.sum(d[:n_event] - np.log(phi))
    w = -h * _cum_at(1. / phi, idx, ties)
    w[:n_event] += 1.
    if dtype is np.float64:
        grad = np.asarray(X.T @ w, dtype=np.float64).ravel()
    else:
        grad = _tdot_ld(X, w)
    return float(ll), grad


def scans_hessian_matvec(X, beta, v, idx, dtype=np.float64, ties='efron'):
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    h = np.exp(eta - np.max(eta))
    inv = 1. / _phi_sums(h, idx, ties)
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(dtype)
    z = inv * (inv * _phi_sums(h * u, idx, ties))
    r = (h * _cum_at(inv, idx, ties)) * u - h * _cum_at(z, idx, ties)
    if dtype is np.float64:
        return np.asarray(X.T @ (-r), dtype=np.float64).ravel()
    return _tdot_ld(X, -r)


def phi_ext(X, beta, idx):
    """phi of every event in long double."""
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(LD)
    return _phi_sums(np.exp(eta - np.max(eta)), idx, 'efron')


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
    """The Cox model with Efron ties on the host: cox_interval_oracle's
    OracleModel (trajectory, tree) on this module's likelihood."""

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
def grid_times(X, seed=0, n_grid=10, censor_frac=.4):
    """Unsorted (event, censoring) for the rows of X with times on a grid of
    n_grid points, so that events tie many deep and censoring times tie event
    times."""
    rs = np.random.RandomState(seed)
    n, p = X.shape
    beta = np.zeros(p)
    beta[:min(p, 5)] = rs.randn(min(p, 5)) * .5
    t = rs.exponential(np.exp(-np.asarray(X @ beta).ravel()))
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
