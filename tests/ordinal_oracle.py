"""NumPy restatement of the proportional-odds (cumulative logit) likelihood of
an ordered outcome with a per-row offset and K - 1 cutpoints on a centred
design without an intercept: what csrc/ordinal.hip is tested against.  The
design tuple D and its products are those of tests/logit_oracle.py;
`OracleModel` has the method names of the device model
(bayesbridge_amd.model.OrdinalModel), so that the host logic of hmc.py,
nuts.py, cutpoints.py and the Gibbs driver can run on it unchanged.

Written from the PRODUCT form.  With a = c_{y+1} - xo, b = c_y - xo, xo = eta +
o, c_0 = -inf, c_K = +inf and delta_k = c_{k+1} - c_k:
  ll = (g_y - softplus(-a)) - softplus(b)
  w  = sigma(b) - sigma(-a)
  d  = sigma(a) sigma(-a) + sigma(b) sigma(-b),  sigma(x) sigma(-x) = e/(1+e)^2
  g_k = log(1 - exp(-delta_k)) for 0 < k < K - 1, else 0
(log(sigma(a) - sigma(b)) as a difference of two sigmas is wrong from |eta| =
40 on and would bless a wrong kernel.)  Every function takes the precision it
computes in: np.longdouble is the oracle, np.float64 the "same formulas in
float64" whose distance from the oracle sets the device's tolerances."""
import math

import numpy as np

import poisson_oracle as po
from logit_oracle import design, dot, tdot, trajectory  # noqa: F401

LD = np.longdouble


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigma(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def sigma_sigma(x):
    """sigma(x) sigma(-x) = e / ((1 + e) (1 + e)), e = exp(-|x|)."""
    e = np.exp(-np.abs(x))
    q = 1 + e
    return e / (q * q)


def gap_terms(cuts, dtype=np.float64):
    """g_k for k = 0 ... K - 1: 0 for the two end categories."""
    cuts = np.asarray(cuts, dtype=dtype)
    delta = np.diff(cuts)
    with np.errstate(divide='ignore'):
        g = np.where(delta <= dtype(math.log(2.)), np.log(-np.expm1(-delta)),
                     np.log1p(-np.exp(-delta)))
    return np.concatenate(([dtype(0)], g, [dtype(0)])).astype(dtype)


def row_terms(xo, y, cuts, dtype=np.float64, gap_term=True):
    """(ll, w, d) per row in `dtype`; xo = eta + offset.  The end categories'
    infinite cutpoint is a select, as on the device: a = +inf for y = K - 1
    and b = -inf for y = 0 whatever xo holds."""
    xo = np.asarray(xo, dtype=dtype)
    cuts = np.asarray(cuts, dtype=dtype)
    y = np.asarray(y).astype(np.intp)
    K = len(cuts) + 1
    inf = dtype(np.inf)
    lower = np.concatenate(([-inf], cuts))[y]
    upper = np.concatenate((cuts, [inf]))[y]
    g = gap_terms(cuts, dtype)[y] if gap_term else dtype(0)
    with np.errstate(invalid='ignore', over='ignore'):
        neg_a = np.where(y == K - 1, -inf, -(upper - xo))
        b = np.where(y == 0, -inf, lower - xo)
        ll = (g - softplus(neg_a)) - softplus(b)
        w = sigma(b) - sigma(neg_a)
        d = sigma_sigma(neg_a) + sigma_sigma(b)
    return ll, w, d


def category_loglik(eta, k, cuts, dtype=LD):
    """ll of category k at every eta (the oracle's own checks)."""
    eta = np.asarray(eta, dtype=dtype)
    return row_terms(eta, np.full(eta.shape, k), cuts, dtype)[0]


def category_loglik_mp(eta, k, cuts, dps=400):
    """log(sigma(c_{k+1} - eta) - sigma(c_k - eta)) from the DIFFERENCE of two
    sigmas, in mpmath at `dps` digits: another formula than the oracle's, and
    enough digits for the difference to be exact to far below a long double
    at |eta| up to 300 (1 - exp(-300) alone needs 131)."""
    import mpmath
    with mpmath.workdps(dps):
        eta = mpmath.mpf(float(eta))
        K = len(cuts) + 1

        def cdf(j):       # P(y <= j - 1) = sigma(c_j - eta), c_0, c_K infinite
            if j == 0:
                return mpmath.mpf(0)
            if j == K:
                return mpmath.mpf(1)
            return 1 / (1 + mpmath.exp(-(mpmath.mpf(float(cuts[j - 1]))
                                         - eta)))
        return mpmath.log(cdf(k + 1) - cdf(k))


def _eta(D, beta, offset, dtype):
    """X~ beta + offset in `dtype`: the product itself is formed in it."""
    if dtype is np.float64:
        return dot(D, beta) + offset
    X, col_offset, intercept = D
    assert not intercept
    Xd = np.asarray(X.toarray() if hasattr(X, 'toarray') else X, dtype=dtype)
    beta = np.asarray(beta, dtype=dtype)
    out = Xd.dot(beta)
    if col_offset is not None:
        out = out - np.asarray(col_offset, dtype=dtype).dot(beta)
    return out + np.asarray(offset, dtype=dtype)


def _tdot(D, w, dtype):
    if dtype is np.float64:
        return tdot(D, w)
    X, col_offset, intercept = D
    Xd = np.asarray(X.toarray() if hasattr(X, 'toarray') else X, dtype=dtype)
    out = Xd.T.dot(w)
    if col_offset is not None:
        out = out - np.asarray(col_offset, dtype=dtype) * np.sum(w)
    return out


def loglik_grad(D, y, offset, beta, cuts, dtype=np.float64):
    """The whole log-likelihood and its gradient."""
    ll, w, _ = row_terms(_eta(D, beta, offset, dtype), y, cuts, dtype)
    with np.errstate(invalid='ignore'):
        total = np.sum(ll)
    if dtype is np.float64:
        return float(total), _tdot(D, w, dtype)
    return total, _tdot(D, w, dtype)


def hessian_matvec(D, y, offset, beta, v, cuts, dtype=np.float64):
    _, _, d = row_terms(_eta(D, beta, offset, dtype), y, cuts, dtype)
    u = _eta(D, v, np.zeros(len(y)), dtype)
    return _tdot(D, -(d * u), dtype)


def cutpoint_loglik(D, y, offset, beta, cuts, dtype=LD, gap_term=True):
    """L(c) = sum ll for one cutpoint vector (K - 1,) or several (n_c,
    K - 1)."""
    xo = _eta(D, beta, offset, dtype)
    cuts = np.asarray(cuts, dtype=np.float64)
    many = cuts.ndim == 2
    out = np.array([np.sum(row_terms(xo, y, c, dtype, gap_term)[0])
                    for c in np.atleast_2d(cuts)])
    out = out.astype(np.float64) if dtype is not np.float64 else out
    return out if many else float(out[0])


def precond_f(D, y, offset, scale, prior_prec, cuts):
    """f(q) of the preconditioned coordinates (reg_coef_sampler.py:259-279) on
    the oracle likelihood; no gradient where logp is not finite."""
    def f(q):
        ll, g = loglik_grad(D, y, offset, q * scale, cuts)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def newton_mle(D, y, offset, cuts, n_iter=100):
    """The maximum-likelihood coefficients at fixed cutpoints."""
    P = D[0].shape[1] + int(D[2])
    eye = np.eye(P)
    beta = np.zeros(P)
    ll, grad = loglik_grad(D, y, offset, beta, cuts)
    for _ in range(n_iter):
        info = -np.column_stack([
            hessian_matvec(D, y, offset, beta, e, cuts) for e in eye])
        step = np.linalg.solve(info, grad)
        # the likelihood is concave in beta: halve a step that overshoots
        for _ in range(40):
            new_ll, new_grad = loglik_grad(D, y, offset, beta + step, cuts)
            if new_ll >= ll or np.abs(step).max() < 1e-13:
                break
            step = step / 2
        beta, ll, grad = beta + step, new_ll, new_grad
        if np.abs(step).max() < 1e-13:
            break
    return beta


def initial_cutpoints(y, K):
    counts = np.bincount(np.asarray(y).astype(np.intp), minlength=K)
    cum = np.cumsum(counts)[:-1] / float(len(y))
    return np.log(cum) - np.log1p(-cum)


def simulate(rs, eta, cuts):
    """Categories with P(y <= k) = sigma(c_{k+1} - eta)."""
    return np.searchsorted(np.asarray(cuts), eta + rs.logistic(size=len(eta)),
                           side='left').astype(np.float64)


class OracleModel(po.OracleModel):
    """The ordinal model on the host.  `design` is only handed on (the Gibbs
    driver reads its shape and its intercept flag).  `perturb`: a relative
    perturbation of the likelihood, the gradient and L(c), for the choice of
    chain seeds whose path does not hang on the last bits."""
    name = 'ordinal'

    def __init__(self, D, y, offset=None, design=None, cutpoints=None,
                 cutpoint_prior=None, perturb=0.):
        y = np.asarray(y, dtype=np.float64)
        offset = np.zeros(len(y)) if offset is None else offset
        super().__init__(D, y, offset, design)
        self.offset = self.log_exposure
        self.n_category = int(y.max()) + 1
        self.cutpoints_fixed = cutpoints is not None
        self.cutpoints = initial_cutpoints(y, self.n_category) \
            if cutpoints is None else np.array(cutpoints, dtype=np.float64)
        self.cutpoint_prior = cutpoint_prior or {'sd': 10.}
        self.perturb = perturb
        self._beta = None

    def calc_intercept_mle(self):
        raise ValueError("no intercept")

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        ll, grad = loglik_grad(self.D, self.y, self.offset,
                               np.asarray(beta, dtype=np.float64),
                               self.cutpoints)
        if ll == -math.inf:
            return -math.inf, None
        ll, grad = ll * (1. + self.perturb), grad * (1. + self.perturb)
        return ll, (None if loglik_only else grad)

    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        beta, cuts = np.array(beta, dtype=np.float64), self.cutpoints.copy()
        return lambda v: hessian_matvec(self.D, self.y, self.offset, beta,
                                        np.ravel(v), cuts)

    def cutpoint_loglik(self, coef, cuts, gap_term=True):
        if coef is not None:
            self._beta = np.array(coef, dtype=np.float64)
        out = cutpoint_loglik(self.D, self.y, self.offset, self._beta, cuts,
                              gap_term=gap_term)
        return out * (1. + self.perturb)

    def _f(self, scale, prior_prec):
        base = precond_f(self.D, self.y, self.offset,
                         np.asarray(scale, dtype=np.float64),
                         np.asarray(prior_prec, dtype=np.float64),
                         self.cutpoints.copy())
        if not self.perturb:
            return base

        def f(q):
            logp, grad = base(q)
            return logp * (1. + self.perturb), \
                (None if grad is None else grad * (1. + self.perturb))
        return f


# ---- prediction -------------------------------------------------------------

def _predict_terms(Xt, coef, cuts, y, offset, dtype):
    """(p (n, S, K), ll (n, S) or None): Xt the centred design (n, P), coef
    (P, S), cuts (K - 1, S).  p as the device forms it, a difference of two
    sigmas (its absolute error is what a mean needs); ll in the stable
    form."""
    Xt = np.asarray(Xt, dtype=dtype)
    eta = Xt.dot(np.asarray(coef, dtype=dtype))
    if offset is not None:
        eta = eta + np.asarray(offset, dtype=dtype)[:, None]
    n, S = eta.shape
    K = cuts.shape[0] + 1
    p = np.empty((n, S, K), dtype=dtype)
    ll = None if y is None else np.empty((n, S), dtype=dtype)
    for s in range(S):
        c = np.asarray(cuts[:, s], dtype=dtype)
        cdf = np.column_stack(
            [np.zeros(n, dtype=dtype)]
            + [sigma(ck - eta[:, s]) for ck in c] + [np.ones(n, dtype=dtype)])
        p[:, s, :] = np.diff(cdf, axis=1)
        if y is not None:
            ll[:, s] = row_terms(eta[:, s], y, cuts[:, s], dtype)[0]
    return p, ll


def predict_explicit(Xt, coef, cuts, y=None, offset=None):
    """The summaries from their definitions, in long double."""
    p, ll = _predict_terms(Xt, coef, cuts, y, offset, LD)
    S = p.shape[1]
    mean = p.sum(axis=1) / S
    res = {'mean': mean,
           'sd': np.sqrt(((p - mean[:, None, :]) ** 2).sum(axis=1) / S)}
    if ll is not None:
        top = ll.max(axis=1)
        res.update({
            'lpd': top + np.log(np.exp(ll - top[:, None]).sum(axis=1))
            - np.log(LD(S)),
            'loglik_mean': ll.sum(axis=1) / S,
            'loglik_var': ll.var(axis=1, ddof=1)})
    return res


def predict_recurrence(Xt, coef, cuts, y=None, offset=None):
    """The device's float64 updates, one per draw in draw order."""
    p, ll = _predict_terms(Xt, coef, cuts, y, offset, np.float64)
    n, S, K = p.shape
    mean, m2 = np.zeros((n, K)), np.zeros((n, K))
    lmean, lm2 = np.zeros(n), np.zeros(n)
    lmax, lsum = np.full(n, -np.inf), np.zeros(n)
    for s in range(S):
        k = float(s + 1)
        delta = p[:, s, :] - mean
        mean = mean + delta / k
        m2 = m2 + delta * (p[:, s, :] - mean)
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
    res = {'mean': mean, 'sd': np.sqrt(m2 / S)}
    if ll is not None:
        res.update({'lpd': lmax + np.log(lsum) - math.log(S),
                    'loglik_mean': lmean, 'loglik_var': lm2 / (S - 1.)})
    return res
