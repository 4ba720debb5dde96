"""NumPy restatement of the probit chain (Albert & Chib 1993 under the bridge
prior): what tests/test_hip_probit.py compares the device chain's posterior
with, and the log-likelihood its iterations are checked against.

  z_i | beta          ~ N(psi_i, 1) on z > 0 (y_i = 1) or z <= 0 (y_i = 0), by
                        inversion of the tail probability (the device rejects)
  beta | z, tau, lam  ~ N(A^-1 X~^T z, A^-1), A = X~^T X~ + diag(1 / sd^2),
                        by a Cholesky factor (the device: 'cg', 'cholesky' or
                        'woodbury')
  tau | beta, lam | tau, beta   as bayesbridge.py:412-478, raw parametrisation,
                        the tilted stable variate from the host sampler of
                        libbbx_hostrng
X~ = [1, X - column means].  No GPU, no libbbx."""
from ctypes import c_void_p

import numpy as np
from numpy.random import PCG64, Generator
from scipy.special import log_ndtr, ndtr, ndtri


def loglik(psi, y):
    """sum_i log Phi(s_i psi_i), s = 2 y - 1."""
    return float(np.sum(log_ndtr((2. * np.asarray(y) - 1.) * psi)))


def truncated_normal(rng, psi, y):
    """Inversion: with a = -s psi the standardised draw x >= a has the upper
    tail u Phi(-a), u uniform, i.e. x = -Phi^-1(u Phi(-a)); z = psi + s x."""
    s = 2. * np.asarray(y) - 1.
    a = -s * psi
    x = -ndtri(rng.random(len(psi)) * ndtr(-a))
    return psi + s * np.maximum(x, a)


def shrunk_scale(tau, lam, slab):
    raw = tau * lam
    return raw / np.sqrt(1. + (raw / slab) ** 2)


class ProbitOracle():

    def __init__(self, y, X, bridge_exponent=.5, sd_for_intercept=2.,
                 slab=2., gscale_shape=0., gscale_rate=0.):
        from math import gamma
        self.y = np.asarray(y, dtype=np.float64)
        X = np.asarray(X, dtype=np.float64)
        self.Xt = np.hstack([np.ones((X.shape[0], 1)), X - X.mean(axis=0)])
        self.gram = self.Xt.T @ self.Xt
        self.alpha, self.sd0, self.slab = bridge_exponent, sd_for_intercept, \
            slab
        self.shape0, self.rate0 = gscale_shape, gscale_rate
        # bayesbridge.py:420-424
        self.lower_bd = .001 / (gamma(2. / bridge_exponent)
                                / gamma(1. / bridge_exponent))

    def _tilted_stable(self, bitgen, tilt):
        from bayesbridge_amd import hostrng
        out = np.zeros(tilt.size)
        a = np.full(tilt.size, self.alpha / 2.)
        st = hostrng.load().bbx_host_tilted_stable(
            hostrng._bitgen_address(bitgen), tilt.size,
            a.ctypes.data_as(c_void_p), tilt.ctypes.data_as(c_void_p),
            out.ctypes.data_as(c_void_p))
        assert st == 0
        return out

    def run(self, n_iter, n_burnin, seed, tau=.1):
        """Kept coefficient draws [n_iter - n_burnin, P]."""
        rng = Generator(PCG64(seed))
        ts_bitgen = PCG64(seed + 7919)
        n, P = self.Xt.shape
        alpha = self.alpha
        beta = np.zeros(P)
        lam = np.ones(P - 1)
        kept = np.empty((n_iter - n_burnin, P))
        for it in range(n_iter):
            z = truncated_normal(rng, self.Xt @ beta, self.y)
            sd = np.concatenate(([self.sd0],
                                 shrunk_scale(tau, lam, self.slab)))
            L = np.linalg.cholesky(self.gram + np.diag(sd ** -2.))
            mean = np.linalg.solve(L.T, np.linalg.solve(L, self.Xt.T @ z))
            beta = mean + np.linalg.solve(L.T, rng.standard_normal(P))
            b = beta[1:]
            phi = rng.gamma(self.shape0 + b.size / alpha) \
                / (self.rate0 + np.sum(np.abs(b) ** alpha))
            tau = max(phi ** (-1. / alpha), self.lower_bd)
            lam = np.sqrt(.5 / self._tilted_stable(ts_bitgen,
                                                   (b / tau) ** 2))
            lam[lam == 0.] = 10e-16
            lam[np.isinf(lam)] = 2. / tau
            if it >= n_burnin:
                kept[it - n_burnin] = beta
        return kept


# ---- posterior prediction (ProbitModel.predict, csrc/probit_predict.hip)

PRED_KEYS = ('mean', 'sd', 'lpd', 'loglik_mean', 'loglik_var')
LD = np.longdouble


def predict_cases():
    """(n rows, S draws) -> (X raw [n, 5], coef [5, S], y): the rows around a
    workgroup's edge, the draws around a pass of 16.  From 257 rows on the
    first and the last row have eta = +40 and -40 in every draw (column 0 is
    +-1 there and 0 elsewhere, its coefficient 40), once with each outcome."""
    out = {}
    for n in (1, 257, 4099):
        for S in (2, 16, 17, 33):
            rng = np.random.default_rng(100 * n + S)
            X = rng.standard_normal((n, 5))
            X[:, 0] = 0.
            coef = .7 * rng.standard_normal((5, S))
            coef[0] = 40.
            y = (rng.random(n) < .5).astype(np.float64)
            if n >= 257:
                X[[0, 1, n - 2, n - 1]] = 0.
                X[[0, 1], 0], X[[n - 2, n - 1], 0] = 1., -1.
                y[[0, 1, n - 2, n - 1]] = [1., 0., 1., 0.]
            out[n, S] = (X, coef, y)
    return out


def _pred_terms(eta, y):
    """float64 terms (mu, ll) [n, S] from the linear predictors."""
    eta = np.asarray(eta, dtype=np.float64)
    s = 2. * np.asarray(y, dtype=np.float64)[:, None] - 1.
    return ndtr(eta), log_ndtr(s * eta)


def predict_explicit(X, coef, y):
    """The yardstick: eta in long double, the float64 terms accumulated in
    long double -- two-pass mean and population sd, logsumexp, var(ddof=1)."""
    eta = np.asarray(X, dtype=LD) @ np.asarray(coef, dtype=LD)
    mu, ll = (t.astype(LD) for t in _pred_terms(eta, y))
    S = LD(mu.shape[1])
    mean = mu.sum(axis=1) / S
    sd = np.sqrt(((mu - mean[:, None]) ** 2).sum(axis=1) / S)
    top = ll.max(axis=1)
    lpd = top + np.log(np.exp(ll - top[:, None]).sum(axis=1)) - np.log(S)
    ll_mean = ll.sum(axis=1) / S
    ll_var = ((ll - ll_mean[:, None]) ** 2).sum(axis=1) / (S - 1)
    return dict(zip(PRED_KEYS, (mean, sd, lpd, ll_mean, ll_var)))


def predict_recurrence(X, coef, y):
    """The device's updates in float64, draw by draw (the accumulators'
    contract of csrc/predict_summary.hpp)."""
    X, coef = np.asarray(X, dtype=np.float64), np.asarray(coef, np.float64)
    eta = np.zeros((X.shape[0], coef.shape[1]))
    for j in range(X.shape[1]):
        eta += X[:, j:j + 1] * coef[j]
    mu, ll = _pred_terms(eta, y)
    n, S = mu.shape
    mean, m2 = np.zeros(n), np.zeros(n)
    lmean, lm2 = np.zeros(n), np.zeros(n)
    lmax, lsum = np.full(n, -np.inf), np.zeros(n)
    for k in range(S):
        x = mu[:, k]
        d = x - mean
        mean = mean + d / (k + 1.)
        m2 = m2 + d * (x - mean)
        x = ll[:, k]
        d = x - lmean
        lmean = lmean + d / (k + 1.)
        lm2 = lm2 + d * (x - lmean)
        up = x > lmax
        with np.errstate(invalid='ignore'):
            lsum = np.where(up, lsum * np.exp(lmax - x) + 1.,
                            lsum + np.exp(x - lmax))
        lmax = np.where(up, x, lmax)
    return dict(zip(PRED_KEYS, (mean, np.sqrt(m2 / S),
                                lmax + np.log(lsum) - np.log(float(S)),
                                lmean, lm2 / (S - 1.))))


def rel_err(got, want):
    """Largest error relative to the largest magnitude of `want`."""
    want = np.asarray(want, dtype=LD)
    scale = max(float(np.abs(want).max()), 1e-300)
    return float(np.abs(np.asarray(got, dtype=LD) - want).max()) / scale


# Largest rel_err of predict_recurrence against predict_explicit over
# predict_cases(), measured (tests/test_probit_host_logic.py repeats it); the
# tolerance the device is held to is 16 x that rounded up to a power of ten,
# the rule of tests/test_hip_predict.py.
PRED_MEASURED = {'mean': 3.7e-16, 'sd': 3.4e-16, 'lpd': 1.9e-16,
                 'loglik_mean': 1.9e-16, 'loglik_var': 5.7e-16}


def pred_tolerance(measured):
    return 10. ** np.ceil(np.log10(16. * measured))


def batch_means(x, n_batch=25):
    """(mean, its standard error by batch means) of the columns of x."""
    x = np.asarray(x, dtype=np.float64)
    m = x.shape[0] // n_batch
    b = x[:m * n_batch].reshape(n_batch, m, -1).mean(axis=1)
    return b.mean(axis=0), b.std(axis=0, ddof=1) / np.sqrt(n_batch)


def moments(draws, n_batch=25):
    """Ergodic mean and variance of every coefficient, each with its
    batch-means standard error: (values [2 P], errors [2 P])."""
    draws = np.asarray(draws, dtype=np.float64)
    mean, se_mean = batch_means(draws, n_batch)
    var, se_var = batch_means((draws - mean) ** 2, n_batch)
    return np.concatenate((mean, var)), np.concatenate((se_mean, se_var))


def z_scores(draws_a, draws_b, n_batch=25):
    """|difference| / its standard error for every mean and variance; the two
    sets of draws are lists of independent chains [n_sample, P]."""
    def pooled(chains):
        vals, errs = zip(*(moments(c, n_batch) for c in chains))
        k = len(chains)
        return np.mean(vals, axis=0), \
            np.sqrt(np.sum(np.square(errs), axis=0)) / k
    va, ea = pooled(draws_a)
    vb, eb = pooled(draws_b)
    return np.abs(va - vb) / np.sqrt(ea ** 2 + eb ** 2)
