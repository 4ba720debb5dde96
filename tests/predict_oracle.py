"""NumPy oracle of the posterior prediction of the linear, logit and Poisson
models (bayesbridge_amd model.predict, csrc/predict.hip), in two forms:

explicit    in np.longdouble: the (n, S) matrices of mu and of the pointwise
            log-likelihood from X~ @ coef (X~ centred and intercepted by
            hand), a two-pass mean and population sd, logsumexp for lpd and
            var(ddof=1) for loglik_var;
recurrence  in float64: the device's updates draw by draw, in draw order
            (Welford on mu and on ll, the online log-sum-exp).

Both take the design as (X raw (n, p) dense, column means or None,
intercept flag) and coef as (P, S)."""
import math

import numpy as np
from scipy.special import gammaln

LD = np.longdouble
FAMILIES = ('linear', 'logit', 'poisson')
KEYS = ('mean', 'sd', 'lpd', 'loglik_mean', 'loglik_var')


def design_matrix(X, center=None, intercept=True, dtype=np.float64):
    """X~: the columns minus `center` (the TRAINING means), a leading column
    of ones with `intercept`."""
    X = np.asarray(X.todense() if hasattr(X, 'todense') else X, dtype=dtype)
    if center is not None:
        X = X - np.asarray(center, dtype=dtype)
    if intercept:
        X = np.hstack((np.ones((X.shape[0], 1), dtype=dtype), X))
    return X


def ll_const(family, y, n_trial=None):
    """What makes ll a proper log density (float64, as model.py forms it)."""
    y = np.asarray(y, dtype=np.float64)
    if family == 'linear':
        return np.full(y.shape, -.5 * math.log(2. * math.pi))
    if family == 'logit':
        m = np.ones(y.shape) if n_trial is None else np.asarray(n_trial, float)
        return gammaln(m + 1.) - gammaln(y + 1.) - gammaln(m - y + 1.)
    return -gammaln(y + 1.)


def _terms(family, eta, y, obs_prec, n_trial, const, dtype):
    """(mu, ll or None), each (n, S), from eta (n, S) (offset included)."""
    with np.errstate(over='ignore', invalid='ignore'):
        if family == 'linear':
            mu = eta
        elif family == 'logit':
            e = np.exp(-np.abs(eta))
            mu = np.where(eta >= 0, 1 / (1 + e), e / (1 + e))
        else:
            mu = np.exp(eta)
        if y is None:
            return mu, None
        y = np.asarray(y, dtype=dtype)[:, None]
        if family == 'linear':
            tau = np.asarray(obs_prec, dtype=dtype)[None, :]
            r = y - eta
            ll = dtype(.5) * np.log(tau) - dtype(.5) * tau * r * r
        elif family == 'logit':
            m = 1 if n_trial is None \
                else np.asarray(n_trial, dtype=dtype)[:, None]
            sp = np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))
            ll = y * eta - m * sp
        else:
            ll = y * eta - mu
        if const is not None:
            ll = ll + np.asarray(const, dtype=dtype)[:, None]
    return mu, ll


def _eta(Xt, coef, offset, dtype):
    Xt, coef = np.asarray(Xt, dtype=dtype), np.asarray(coef, dtype=dtype)
    if dtype is LD:
        eta = Xt @ coef
    else:
        # column by column in index order: the same bits whatever BLAS and
        # however many threads this machine has
        eta = np.zeros((Xt.shape[0], coef.shape[1]))
        for j in range(Xt.shape[1]):
            eta += Xt[:, j:j + 1] * coef[j]
    if offset is not None:
        eta = eta + np.asarray(offset, dtype=dtype)[:, None]
    return eta


def explicit(family, Xt, coef, y=None, obs_prec=None, offset=None,
             n_trial=None, const=None):
    """The long-double form on X~ (n, P) and coef (P, S): a dict of KEYS (the
    first two without y) and 'll', the (n, S) matrix."""
    eta = _eta(Xt, coef, offset, LD)
    mu, ll = _terms(family, eta, y, obs_prec, n_trial, const, LD)
    S = eta.shape[1]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        mean = mu.sum(axis=1) / S
        sd = np.sqrt(((mu - mean[:, None]) ** 2).sum(axis=1) / S)
        res = {'mean': mean, 'sd': sd, 'mu': mu}
        if ll is not None:
            top = ll.max(axis=1)
            safe = np.where(np.isfinite(top), top, 0)
            lpd = safe + np.log(np.exp(ll - safe[:, None]).sum(axis=1)) \
                - np.log(LD(S))
            res.update({'lpd': lpd, 'loglik_mean': ll.sum(axis=1) / S,
                        'loglik_var': ll.var(axis=1, ddof=1) if S > 1
                        else np.full(len(lpd), np.nan, LD), 'll': ll})
    return res


def _welford_mean(mean, x, delta, k):
    """mean + delta / k; an infinite mean stays (the plain sum's value)
    unless the draw is a NaN or the opposite infinity."""
    stuck = np.where(np.isnan(x) | (x == -mean), np.nan, mean)
    return np.where(np.isinf(mean), stuck, mean + delta / k)


def recurrence(family, Xt, coef, y=None, obs_prec=None, offset=None,
               n_trial=None, const=None, eta=None):
    """The device's float64 updates, one per draw in draw order (eta (n, S):
    the linear predictors to use instead of X~ @ coef, offset not yet
    added)."""
    if eta is None:
        eta = _eta(Xt, coef, offset, np.float64)
    elif offset is not None:
        eta = eta + np.asarray(offset, dtype=np.float64)[:, None]
    mu, ll = _terms(family, eta, y, obs_prec, n_trial, const, np.float64)
    n, S = eta.shape
    mean, m2 = np.zeros(n), np.zeros(n)
    lmean, lm2 = np.zeros(n), np.zeros(n)
    lmax, lsum = np.full(n, -np.inf), np.zeros(n)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for s in range(S):
            k = float(s + 1)
            x = mu[:, s]
            delta = x - mean
            mean = _welford_mean(mean, x, delta, k)
            m2 = m2 + delta * (x - mean)
            if ll is None:
                continue
            x = ll[:, s]
            delta = x - lmean
            lmean = _welford_mean(lmean, x, delta, k)
            lm2 = lm2 + delta * (x - lmean)
            up = x > lmax
            add = ~up & (x != -np.inf)
            new_sum = np.where(up, lsum * np.exp(lmax - x) + 1., lsum)
            new_sum = np.where(add, lsum + np.exp(x - lmax), new_sum)
            lmax = np.where(up, x, lmax)
            lsum = new_sum
        res = {'mean': mean, 'sd': np.sqrt(m2 / S), 'mu': mu}
        if ll is not None:
            res.update({'lpd': lmax + np.log(lsum) - math.log(S),
                        'loglik_mean': lmean,
                        'loglik_var': lm2 / (S - 1.) if S > 1
                        else np.full(n, np.nan), 'll': ll})
    return res


def waic(res):
    """(lppd, p_waic, waic) of a result with an outcome."""
    lppd = res['lpd'].sum()
    p = res['loglik_var'].sum()
    return lppd, p, -2 * (lppd - p)


def rel_err(got, want):
    """max |got - want| relative to the largest magnitude of `want`."""
    want = np.asarray(want, dtype=LD)
    scale = np.abs(want).max()
    return float(np.abs(np.asarray(got, dtype=LD) - want).max()
                 / (scale if scale > 0 else 1))


def within(got, want, tol):
    want = np.asarray(want, dtype=LD)
    return bool(np.all(np.abs(np.asarray(got, dtype=LD) - want)
                       <= tol * np.abs(want).max()))
