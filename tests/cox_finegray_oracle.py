"""NumPy oracle of the Fine-Gray subdistribution-hazard likelihood (competing
risks; Breslow ties): what csrc/cox_finegray.hip is tested against.  Every
row has an observed time T and is an event of interest, a competing event or
censored.  Row i is in the risk set of an event at t_k

  * with weight 1 if T_i >= t_k, whatever its status;
  * with weight G(t_k-) / G(T_i-) if it had a competing event at T_i < t_k;

G(s-) = prod_{c < s} (1 - m_c / Y(c)) over the distinct censoring times c,
m_c rows censored at c, Y(c) = #{i : T_i >= c} over rows of every status: the
Kaplan-Meier estimate of the censoring survivor function, from the left.  This
definition is what the tests pin; it is not checked against R's conventions.
Two forms:

  * `explicit`: the n_event x n weight matrix straight from the times and the
    statuses by the definition above (never from the index arrays),
    everything after X beta in np.longdouble (n <= 2049);
  * `scans`: the device's structure in linear time -- the suffix sums E over
    the rows, the prefix sums F of h / G over the competing rows,
    H_k = E[a_k] + g_k F[b_k - 1], the cumulative sum c of 1 / H and the suffix
    sum sg of g / H -- in float64 or np.longdouble, for any n.

Rows are in cox_preprocess_finegray's order.  X is the raw host matrix.
`OracleModel` has the method names of the device models, so that the host
logic of hmc.py, nuts.py and the Gibbs driver can run on it unchanged."""
import math

import numpy as np

import cox_interval_oracle as cio
from cox_interval_oracle import _tdot_ld

LD = np.longdouble
EXPLICIT_MAX_N = 2049
EVENT, COMPETING, CENSORED = 0, 1, 2


def times_and_status(event_time, censoring_time, competing_time):
    """(T, status) of rows with exactly one finite time each."""
    times = np.stack([np.asarray(t, dtype=np.float64) for t in
                      (event_time, competing_time, censoring_time)])
    assert np.all(np.sum(np.isfinite(times), axis=0) == 1)
    return np.min(times, axis=0), np.argmin(times, axis=0)


def censoring_survivor_left(s, T, status, dtype=LD):
    """G(s-) of the rows (T, status) at every time of s, by the definition: a
    loop over the distinct censoring times."""
    s = np.asarray(s, dtype=np.float64)
    G = np.ones(s.shape, dtype=dtype)
    for c in np.unique(T[status == CENSORED]):
        m = dtype(np.sum((T == c) & (status == CENSORED)))
        Y = dtype(np.sum(T >= c))
        G = np.where(c < s, G * (1 - m / Y), G)
    return G


def weight_matrix(event_time, censoring_time, competing_time, full=None):
    """(W[k, i] = the weight of row i in the risk set of event k, the rows of
    the events in time order), by the definition; O(n_event n).  full: the
    (event, censoring, competing) times G is estimated on, where they are more
    rows than these (rows that were dropped since)."""
    T, status = times_and_status(event_time, censoring_time, competing_time)
    assert len(T) <= EXPLICIT_MAX_N
    Tg, sg = (T, status) if full is None else times_and_status(*full)
    evrow = np.flatnonzero(status == EVENT)
    evrow = evrow[np.argsort(T[evrow], kind='stable')]
    t = T[evrow]
    g = censoring_survivor_left(t, Tg, sg)
    Gi = censoring_survivor_left(T, Tg, sg)
    assert np.all(Gi > 0) and np.all(g > 0)
    at_risk = T[None, :] >= t[:, None]
    stays = (status == COMPETING)[None, :] & (T[None, :] < t[:, None])
    W = np.where(at_risk, LD(1), np.where(stays, g[:, None] / Gi[None, :],
                                          LD(0)))
    return W, evrow


def index_arrays(event_time, censoring_time, competing_time, full=None):
    """idx = (n_event, evrow, a, b, p, comp_row, g, r) of sorted rows, each
    from its definition by loops; g and r in float64 from a float64 G."""
    T, status = times_and_status(event_time, censoring_time, competing_time)
    Tg, sg = (T, status) if full is None else times_and_status(*full)
    n = len(T)
    evrow = np.flatnonzero(status == EVENT)
    comp_row = np.flatnonzero(status == COMPETING)
    t = T[evrow]
    a = np.array([min(i for i in range(n) if T[i] >= tk) for tk in t],
                 dtype=np.int64)
    b = np.array([np.sum(comp_row < ak) for ak in a], dtype=np.int64)
    p = np.array([np.sum(t <= T[i]) for i in range(n)], dtype=np.int64)
    g = censoring_survivor_left(t, Tg, sg, np.float64)
    r = 1. / censoring_survivor_left(T[comp_row], Tg, sg, np.float64)
    return len(evrow), evrow, a, b, p, comp_row, g, r


def model_idx(model):
    """idx of a device model."""
    return (model.n_event, model.event_row, model.risk_set_start_index,
            model.n_competing_before, model.n_event_by_exit,
            model.competing_row, model.event_censoring_survivor,
            model.competing_inverse_survivor)


# ----------------------------------------------------------- explicit form
def _explicit(X, beta, W):
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(LD)
    d = eta - np.max(eta)
    h = np.exp(d)
    return d, h, W @ h


def explicit_loglik_grad(X, beta, W, evrow):
    d, h, H = _explicit(X, beta, W)
    if np.any(H == 0.):
        return -math.inf, None
    Wn = W * h[None, :] / H[:, None]
    delta = np.zeros(len(h), dtype=LD)
    delta[evrow] = 1.
    w = delta - Wn.sum(axis=0)
    return float(np.sum(d[evrow] - np.log(H))), _tdot_ld(X, w)


def explicit_hessian_matvec(X, beta, v, W, evrow):
    d, h, H = _explicit(X, beta, W)
    Wn = W * h[None, :] / H[:, None]
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(LD)
    r = Wn.sum(axis=0) * u - Wn.T @ (Wn @ u)
    return _tdot_ld(X, -r)


# -------------------------------------------------------------- scan form
def _risk_sums(arr, a, b, comp_row, g, r):
    E = np.cumsum(arr[::-1])[::-1]
    F0 = np.concatenate(([arr.dtype.type(0)],
                         np.cumsum(arr[comp_row] * r)))     # F0[j] = F[j - 1]
    return np.where(b > 0, E[a] + g * F0[b], E[a])


def _row_sums(inv, p, comp_row, g, r, n_event):
    """A_i from inv: c[p - 1] + [i competing] r sg[p]."""
    c0 = np.concatenate(([inv.dtype.type(0)], np.cumsum(inv)))
    sg = np.concatenate((np.cumsum((g * inv)[::-1])[::-1],
                         [inv.dtype.type(0)]))
    A = c0[p]
    A[comp_row] = A[comp_row] + r * sg[p[comp_row]]
    return A


def _typed(idx, dtype):
    n_event, evrow, a, b, p, comp_row, g, r = idx
    return (n_event, evrow, a, b, p, comp_row, np.asarray(g).astype(dtype),
            np.asarray(r).astype(dtype))


def scans_loglik_grad(X, beta, idx, dtype=np.float64):
    """idx = (n_event, evrow, a, b, p, comp_row, g, r)."""
    n_event, evrow, a, b, p, comp_row, g, r = _typed(idx, dtype)
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    d = eta - np.max(eta)
    h = np.exp(d)
    H = _risk_sums(h, a, b, comp_row, g, r)
    if np.any(H == 0.):
        return -math.inf, None
    ll = np.sum(d[evrow] - np.log(H))
    w = -h * _row_sums(1. / H, p, comp_row, g, r, n_event)
    w[evrow] += 1.
    if dtype is np.float64:
        grad = np.asarray(X.T @ w, dtype=np.float64).ravel()
    else:
        grad = _tdot_ld(X, w)
    return float(ll), grad


def scans_hessian_matvec(X, beta, v, idx, dtype=np.float64):
    n_event, evrow, a, b, p, comp_row, g, r = _typed(idx, dtype)
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    h = np.exp(eta - np.max(eta))
    H = _risk_sums(h, a, b, comp_row, g, r)
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(dtype)
    S = _risk_sums(h * u, a, b, comp_row, g, r)
    inv = 1. / H
    A = _row_sums(inv, p, comp_row, g, r, n_event)
    Z = _row_sums(inv * (inv * S), p, comp_row, g, r, n_event)
    rr = (h * A) * u - h * Z
    if dtype is np.float64:
        return np.asarray(X.T @ (-rr), dtype=np.float64).ravel()
    return _tdot_ld(X, -rr)


def precond_f(X, scale, prior_prec, idx):
    """f(q) of the preconditioned coordinates on the oracle likelihood; no
    gradient where logp is not finite."""
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
    """The Fine-Gray model on the host: the counting-process oracle's driver
    methods on this module's likelihood."""

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = scans_loglik_grad(
            self.X, np.asarray(beta, dtype=np.float64), self.idx)
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


# ---------------------------------------------------------------- test data
def split(t, status):
    """(event, censoring, competing) times from (T, status)."""
    inf = np.inf
    return (np.where(status == EVENT, t, inf),
            np.where(status == CENSORED, t, inf),
            np.where(status == COMPETING, t, inf))


def make_times(X, seed=0, n_grid=None, fracs=(1 / 3, 1 / 3)):
    """Unsorted (event, censoring, competing) for the rows of X: exponential
    times under a sparse true coefficient vector, the status drawn with
    probabilities fracs = (competing, censored); with n_grid, on a grid of
    that many points, so that times of all three kinds tie."""
    rs = np.random.RandomState(seed)
    n, p = X.shape
    beta = np.zeros(p)
    beta[:min(p, 5)] = rs.randn(min(p, 5)) * .5
    t = rs.exponential(np.exp(-np.asarray(X @ beta).ravel()))
    if n_grid:
        edges = np.quantile(t, np.linspace(0, 1, n_grid + 1)[1:])
        t = 1. + np.searchsorted(edges, t, side='left').clip(max=n_grid - 1)
    x = rs.rand(n)
    status = np.where(x < fracs[0], COMPETING,
                      np.where(x < fracs[0] + fracs[1], CENSORED, EVENT))
    return split(t, status)


def blocks_case(n_event, n_comp, n_cens, p=3, seed=0, where='mixed'):
    """Sorted rows with exactly these counts.  where: 'mixed' (the three kinds
    interleaved over a grid of times with ties), 'before' (every competing row
    before the first event: p_i = 0) or 'after' (every competing row after the
    last event).  No row is censored before the first event.  Returns (event,
    censoring, competing, X)."""
    rs = np.random.RandomState(seed)
    n = n_event + n_comp + n_cens
    status = np.concatenate((np.full(n_event, EVENT),
                             np.full(n_comp, COMPETING),
                             np.full(n_cens, CENSORED)))
    n_grid = max(2, n // 3)
    t = 10. + rs.randint(0, n_grid, n).astype(np.float64)
    if where == 'before':
        t[status == COMPETING] = rs.randint(1, 9, n_comp)
    elif where == 'after':
        t[status == COMPETING] = 20. + n_grid + rs.randint(0, 9, n_comp)
    else:
        # the earliest time is an event's, so that no censored row is dropped
        t[0] = 9.
    if where != 'mixed':
        t[status == CENSORED] = np.maximum(t[status == CENSORED],
                                           t[status == EVENT].min())
    order = np.lexsort((status, t))
    X = rs.randn(n, p)
    return split(t[order], status[order]) + (X,)
