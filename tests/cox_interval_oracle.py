"""NumPy oracle of the Cox partial likelihood in counting-process form (row i
is at risk on (entry_i, exit_i]; Breslow ties): what csrc/cox_interval.hip is
tested against.  Two forms:

  * `explicit`: the n_event x n risk-set matrix straight from the definition
    entry_i < t_k <= exit_i, everything after the data in np.longdouble
    (n <= 2049);
  * `scans`: the device's structure in linear time -- the suffix sums E in row
    order and F in entry order, H_k = E[a_k] - F[b_k], the cumulative sums
    c[p - 1] - c[q - 1] -- in float64 or np.longdouble, for any n.

Rows are in cox_preprocess_interval's order.  X is the raw host matrix: the
partial likelihood does not change when a column is centred.  `OracleModel`
has the method names of the device models
(bayesbridge_amd.model._DeviceHamiltonian), so that the host logic of hmc.py,
nuts.py and the Gibbs driver can run on it unchanged."""
import math

import numpy as np

import logit_oracle as lo
import nuts_oracle as no

LD = np.longdouble
EXPLICIT_MAX_N = 2049


def exit_time(event_time, censoring_time):
    return np.minimum(np.asarray(event_time, dtype=np.float64),
                      np.asarray(censoring_time, dtype=np.float64))


def risk_matrix(entry_time, event_time, censoring_time):
    """(mask[k, i] = row i is at risk at the time of event k, the rows of the
    events in time order), by definition; O(n_event n)."""
    entry_time = np.asarray(entry_time, dtype=np.float64)
    event_time = np.asarray(event_time, dtype=np.float64)
    x = exit_time(event_time, censoring_time)
    assert len(x) <= EXPLICIT_MAX_N
    evrow = np.flatnonzero(np.isfinite(event_time))
    evrow = evrow[np.argsort(event_time[evrow], kind='stable')]
    t = event_time[evrow]
    mask = (entry_time[None, :] < t[:, None]) & (t[:, None] <= x[None, :])
    return mask, evrow


def index_arrays_by_loops(entry_time, event_time, censoring_time):
    """(n_event, evrow, a, b, p, q, entry_perm) of sorted rows, each straight
    from its definition; O(n_event n)."""
    entry_time = np.asarray(entry_time, dtype=np.float64)
    event_time = np.asarray(event_time, dtype=np.float64)
    x = exit_time(event_time, censoring_time)
    n = len(x)
    evrow = np.array([i for i in range(n) if math.isfinite(event_time[i])],
                     dtype=np.int64)
    t = event_time[evrow]
    entry_perm = np.array(sorted(range(n), key=lambda i: entry_time[i]),
                          dtype=np.int64)      # sorted() is stable
    a = np.array([min([i for i in range(n) if x[i] >= tk]) for tk in t],
                 dtype=np.int64)
    b = np.array([min([j for j in range(n)
                       if entry_time[entry_perm[j]] >= tk] + [n]) for tk in t],
                 dtype=np.int64)
    p = np.array([np.sum(t <= x[i]) for i in range(n)], dtype=np.int64)
    q = np.array([np.sum(t <= entry_time[i]) for i in range(n)],
                 dtype=np.int64)
    return len(evrow), evrow, a, b, p, q, entry_perm


# ----------------------------------------------------------- explicit form
def _explicit(X, beta, mask, evrow):
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(LD)
    d = eta - np.max(eta)
    h = np.exp(d)
    M = mask.astype(LD)
    H = M @ h
    return d, h, M, H


def explicit_loglik_grad(X, beta, mask, evrow):
    d, h, M, H = _explicit(X, beta, mask, evrow)
    if np.any(H <= 0.):
        return -math.inf, None
    W = M * h[None, :] / H[:, None]
    delta = np.zeros(len(h), dtype=LD)
    delta[evrow] = 1.
    w = delta - W.sum(axis=0)
    ll = np.sum(d[evrow] - np.log(H))
    return float(ll), _tdot_ld(X, w)


def explicit_hessian_matvec(X, beta, v, mask, evrow):
    d, h, M, H = _explicit(X, beta, mask, evrow)
    W = M * h[None, :] / H[:, None]
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(LD)
    r = W.sum(axis=0) * u - W.T @ (W @ u)
    return _tdot_ld(X, -r)


def _tdot_ld(X, w):
    """X^T w with the sum in extended precision (X dense or SciPy sparse)."""
    if isinstance(X, np.ndarray):
        return np.asarray(X.T.astype(LD) @ w, dtype=np.float64)
    C = X.tocsc()
    out = np.zeros(C.shape[1], dtype=LD)
    for j in range(C.shape[1]):
        s = slice(C.indptr[j], C.indptr[j + 1])
        out[j] = np.sum(C.data[s].astype(LD) * w[C.indices[s]])
    return np.asarray(out, dtype=np.float64)


# -------------------------------------------------------------- scan form
def _suffix(x):
    return np.cumsum(x[::-1])[::-1]


def _risk_sums(arr, a, b, entry_perm):
    n = len(arr)
    E = _suffix(arr)
    F = np.concatenate((_suffix(arr[entry_perm]), [arr.dtype.type(0)]))
    late = b < n
    return np.where(late, E[a] - F[b], E[a])


def _cum_at(c, p, q):
    c0 = np.concatenate(([c.dtype.type(0)], c))     # c0[k] = c[k - 1]
    return c0[p] - c0[q]


def scans_loglik_grad(X, beta, idx, dtype=np.float64):
    """idx = (n_event, evrow, a, b, p, q, entry_perm)."""
    n_event, evrow, a, b, p, q, entry_perm = idx
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    d = eta - np.max(eta)
    h = np.exp(d)
    H = _risk_sums(h, a, b, entry_perm)
    if np.any(H <= 0.):
        return -math.inf, None
    ll = np.sum(d[evrow] - np.log(H))
    c = np.cumsum(1. / H)
    w = -h * _cum_at(c, p, q)
    w[evrow] += 1.
    if dtype is np.float64:
        grad = np.asarray(X.T @ w, dtype=np.float64).ravel()
    else:
        grad = _tdot_ld(X, w)
    return float(ll), grad


def scans_hessian_matvec(X, beta, v, idx, dtype=np.float64):
    n_event, evrow, a, b, p, q, entry_perm = idx
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(dtype)
    h = np.exp(eta - np.max(eta))
    H = _risk_sums(h, a, b, entry_perm)
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(dtype)
    S = _risk_sums(h * u, a, b, entry_perm)
    inv = 1. / H
    c = np.cumsum(inv)
    cz = np.cumsum(inv * (inv * S))
    r = (h * _cum_at(c, p, q)) * u - h * _cum_at(cz, p, q)
    if dtype is np.float64:
        return np.asarray(X.T @ (-r), dtype=np.float64).ravel()
    return _tdot_ld(X, -r)


def cancellation(X, beta, idx):
    """max_k E[a_k] / H_k: the factor by which the difference E - F amplifies
    the rounding of the two sums (1 where nothing is subtracted)."""
    n_event, evrow, a, b, p, q, entry_perm = idx
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(LD)
    h = np.exp(eta - np.max(eta))
    return float(np.max(_suffix(h)[a] / _risk_sums(h, a, b, entry_perm)))


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


class _NoGradient(Exception):
    """A leapfrog step was asked for from a state without a gradient."""


class _Missing():
    """Stands for the gradient where logp is not finite."""

    def __rmul__(self, other):
        raise _NoGradient()


class OracleModel():
    """The counting-process Cox model on the host.  `design` is only handed
    on (the Gibbs driver reads its shape and its intercept flag); every
    likelihood value comes from X and the index arrays."""
    name = 'cox'

    def __init__(self, X, idx, design=None):
        self.X, self.idx = X, idx
        self.design = design
        self.n_obs, self.n_pred = X.shape
        self.intercept_added = False

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = scans_loglik_grad(self.X, np.asarray(beta, dtype=np.float64),
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

    # The tree of nuts_oracle on f; where a risk-set sum is empty there is no
    # gradient to take the next step with, and the device ends the half-tree
    # there as unstable (tests/poisson_oracle.py has the same rule).
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


# ---------------------------------------------------------------- test data
def make_times(X, seed=0, entry_frac=.5, censor_frac=.4, ties=False):
    """Unsorted (entry, event, censoring) for the rows of X with real delayed
    entry: a fraction of the rows enters at a time drawn below its exit time
    (the others at -inf).  ties: times on a grid of 1/8, so that event times
    tie with each other, with censoring times and with entry times."""
    rs = np.random.RandomState(seed)
    n, p = X.shape
    beta = np.zeros(p)
    beta[:min(p, 5)] = rs.randn(min(p, 5)) * .5
    t = rs.exponential(np.exp(-np.asarray(X @ beta).ravel()))
    if ties:
        t = np.ceil(t * 8) / 8
    cens = rs.rand(n) < censor_frac
    event = np.where(cens, np.inf, t)
    censoring = np.where(cens, t, np.inf)
    entry = np.where(rs.rand(n) < entry_frac, t * rs.rand(n), -np.inf)
    if ties:
        entry = np.where(np.isfinite(entry), np.floor(entry * 8) / 8, entry)
        entry = np.where(entry < t, entry, -np.inf)
    return entry, event, censoring


def make_data(n, p, seed=0, **kw):
    """make_times on a dense standard-normal X: (entry, event, censoring, X)."""
    X = np.random.RandomState(seed + 1000).randn(n, p)
    return make_times(X, seed, **kw) + (X,)


def term_scales(X, beta, v, idx):
    """The sizes of the terms that the three results are sums of: sum_k
    |eta_k - m| + |log H_k|, |X|^T (delta + h dc) and |X|^T (|h dc u| +
    |h dcz|) -- what a relative tolerance refers to where the terms cancel
    (a likelihood whose risk sets are single rows is 0 for every beta)."""
    n_event, evrow, a, b, p, q, entry_perm = idx
    eta = np.asarray(X @ beta, dtype=np.float64).ravel().astype(LD)
    d = eta - np.max(eta)
    h = np.exp(d)
    H = _risk_sums(h, a, b, entry_perm)
    u = np.asarray(X @ v, dtype=np.float64).ravel().astype(LD)
    inv = 1. / H
    dc = _cum_at(np.cumsum(inv), p, q)
    S = _risk_sums(h * abs(u), a, b, entry_perm)
    dcz = _cum_at(np.cumsum(inv * (inv * S)), p, q)
    delta = np.zeros(len(h), dtype=LD)
    delta[evrow] = 1.
    A = abs(X)
    return (float(np.sum(abs(d[evrow]) + abs(np.log(H)))),
            np.asarray(A.T @ (delta + h * dc), dtype=np.float64).ravel(),
            np.asarray(A.T @ (h * dc * abs(u) + h * dcz),
                       dtype=np.float64).ravel())


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
