"""NumPy restatement of the censored-outcome chain (log-normal AFT, Tobit:
truncated-normal latents on the censored rows, under the bridge prior): what
tests/test_hip_censored.py compares the device chain's posterior with, the
long-double log-likelihood its iterations are checked against, and the
long-double oracle of the predictive and survival summaries.  Row i has a value
b_i and a status: 0 observed (z_i = b_i), 1 right-censored (z_i > b_i), 2
left-censored (z_i <= b_i).  With psi = X~ beta one iteration is, in this
order,

  beta | z, tau, tau_g, lam ~ N(A^-1 tau X~^T z, A^-1), A = tau X~^T X~ +
                        diag(1 / sd^2), by a Cholesky factor (the device: 'cg',
                        'cholesky' or 'woodbury')
  tau | beta, z         ~ Gamma(n/2) / (S/2), S = sum (z_i - psi_i)^2 with the
                        OLD latents
  z_i | beta, tau       truncated normal on the censored rows with the NEW tau
  tau_g | beta, lam | tau_g, beta   as bayesbridge.py:412-478, raw
                        parametrisation, the tilted stable variate from the
                        host sampler of libbbx_hostrng
X~ = [1, X - column means].  All status 0 is the linear model.  No GPU, no
libbbx."""
from ctypes import c_void_p

import numpy as np
from numpy.random import PCG64, Generator
from scipy.special import log_ndtr, ndtr, ndtri

# the z-score helper, the relative error and the rule that turns a measured
# error into a tolerance: those of the probit oracle
from probit_oracle import (PRED_KEYS, batch_means, moments,  # noqa: F401
                           pred_tolerance, rel_err, shrunk_scale, z_scores)

LD = np.longdouble


def loglik(psi, bound, status, tau):
    """The chain's log-likelihood: sum over observed rows of 1/2 log tau - 1/2
    tau (b - psi)^2 in long double, over the censored rows of log Phi(-+a), a =
    (b - psi) sqrt(tau) formed in long double and handed to scipy's log_ndtr."""
    r = np.asarray(bound, dtype=LD) - np.asarray(psi, dtype=LD)
    tau = LD(tau)
    status = np.asarray(status)
    obs = status == 0
    total = (LD(.5) * np.log(tau) - LD(.5) * tau * r[obs] * r[obs]).sum()
    a = (r * np.sqrt(tau)).astype(np.float64)
    sign = np.where(status == 1, -1., 1.)
    return float(total + log_ndtr((sign * a)[~obs]).astype(LD).sum())


def truncated_latents(rng, psi, bound, status, tau):
    """Inversion: the standardised draw x >= a (right-censored) has the upper
    tail u Phi(-a), x <= a (left-censored) the lower tail u Phi(a)."""
    rt = np.sqrt(tau)
    a = (bound - psi) * rt
    u = rng.random(len(psi))
    right = np.maximum(-ndtri(u * ndtr(-a)), a)
    left = np.minimum(ndtri(u * ndtr(a)), a)
    x = np.where(status == 1, right, left)
    return np.where(status == 0, bound, psi + x / rt)


class CensoredOracle():

    def __init__(self, bound, status, X, bridge_exponent=.5,
                 sd_for_intercept=2., slab=2., gscale_shape=0.,
                 gscale_rate=0.):
        from math import gamma
        self.b = np.asarray(bound, dtype=np.float64)
        self.status = np.asarray(status)
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

    def run(self, n_iter, n_burnin, seed, tau_g=.1):
        """Kept draws [n_iter - n_burnin, P + 1]: the coefficients, then tau."""
        rng = Generator(PCG64(seed))
        ts_bitgen = PCG64(seed + 7919)
        Xt, b, status = self.Xt, self.b, self.status
        n, P = Xt.shape
        alpha = self.alpha
        beta = np.zeros(P)
        lam = np.ones(P - 1)
        z = b.copy()
        tau = 1. / np.mean((b - Xt @ beta) ** 2)
        z = truncated_latents(rng, Xt @ beta, b, status, tau)
        kept = np.empty((n_iter - n_burnin, P + 1))
        for it in range(n_iter):
            sd = np.concatenate(([self.sd0],
                                 shrunk_scale(tau_g, lam, self.slab)))
            L = np.linalg.cholesky(tau * self.gram + np.diag(sd ** -2.))
            mean = np.linalg.solve(L.T, np.linalg.solve(L, tau * (Xt.T @ z)))
            beta = mean + np.linalg.solve(L.T, rng.standard_normal(P))
            psi = Xt @ beta
            tau = rng.gamma(n / 2.) / (np.sum((z - psi) ** 2) / 2.)
            z = truncated_latents(rng, psi, b, status, tau)
            bs = beta[1:]
            phi = rng.gamma(self.shape0 + bs.size / alpha) \
                / (self.rate0 + np.sum(np.abs(bs) ** alpha))
            tau_g = max(phi ** (-1. / alpha), self.lower_bd)
            lam = np.sqrt(.5 / self._tilted_stable(ts_bitgen,
                                                   (bs / tau_g) ** 2))
            lam[lam == 0.] = 10e-16
            lam[np.isinf(lam)] = 2. / tau_g
            if it >= n_burnin:
                kept[it - n_burnin, :P] = beta
                kept[it - n_burnin, P] = tau
        return kept


def posterior_problem(seed):
    """The posterior test's data: 400 x 12, planted slopes and intercept 0.3,
    N(0, 1) noise, right-censored at independent N(0.9, 1.5^2) limits: about
    40 % of the rows.  (bound, status, X)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((400, 12))
    beta = np.array([1.2, -1., .8, -.6, .4] + [0.] * 7)
    z = .3 + X @ beta + rng.standard_normal(400)
    limit = .9 + 1.5 * rng.standard_normal(400)
    status = (z > limit).astype(np.uint8)
    return np.where(status == 1, limit, z), status, X


# ---- posterior prediction (CensoredNormalModel.predict, LogNormalAFTModel's,
# csrc/censored_predict.hip)

def predict_cases():
    """(n rows, S draws) -> (X raw [n, 5], coef [5, S], tau [S], y, status):
    the rows around a workgroup's edge, the draws around a pass of 16, a third
    of the rows per status.  From 257 rows on the first and the last three rows
    hold a = (y - eta) sqrt(tau) of about +-40 sqrt(tau) in every draw (column
    0 is +-1 there and 0 elsewhere, its coefficient 40), once per status."""
    out = {}
    for n in (1, 257, 4099):
        for S in (2, 16, 17, 33):
            rng = np.random.default_rng(300 * n + S)
            X = rng.standard_normal((n, 5))
            X[:, 0] = 0.
            coef = .7 * rng.standard_normal((5, S))
            coef[0] = 40.
            tau = np.exp(rng.normal(0., 1., S))
            y = X @ coef[:, 0] + rng.standard_normal(n)
            status = rng.integers(0, 3, n).astype(np.uint8)
            if n >= 257:
                edge = [0, 1, 2, n - 3, n - 2, n - 1]
                X[edge] = 0.
                X[edge[:3], 0], X[edge[3:], 0] = 1., -1.
                y[edge] = 0.
                status[edge] = [0, 1, 2, 0, 1, 2]
            out[n, S] = (X, coef, tau, y, status)
    return out


def survival_points(y):
    """Points of the latent scale before the first and past the last value,
    and those among them (one row: its value alone), increasing; -inf and +inf
    (t = 0 and never) as well."""
    lo, hi = float(np.min(y)), float(np.max(y))
    return np.unique([-np.inf, lo - 5., lo, .5 * (lo + hi), hi, hi + 5.,
                      np.inf])


def _summaries(mu, ll):
    S = LD(mu.shape[1])
    mean = mu.sum(axis=1) / S
    sd = np.sqrt(((mu - mean[:, None]) ** 2).sum(axis=1) / S)
    top = ll.max(axis=1)
    lpd = top + np.log(np.exp(ll - top[:, None]).sum(axis=1)) - np.log(S)
    ll_mean = ll.sum(axis=1) / S
    ll_var = ((ll - ll_mean[:, None]) ** 2).sum(axis=1) / (S - 1)
    return dict(zip(PRED_KEYS, (mean, sd, lpd, ll_mean, ll_var)))


def predict_explicit(X, coef, tau, y, status, exp_mean=False, ll_const=None,
                     points=None):
    """The yardstick: eta and the observed rows' density in long double, the
    tails by scipy's log_ndtr at a formed in long double -- two-pass mean and
    population sd, logsumexp, var(ddof=1).  With points, 'surv_mean' and
    'surv_sd' [n, T] as well: 1 - Phi((c - eta) sqrt(tau)) = ndtr(-x), x in
    long double."""
    eta = np.asarray(X, dtype=LD) @ np.asarray(coef, dtype=LD)
    tau_ = np.asarray(tau, dtype=LD)
    status = np.asarray(status)[:, None]
    a = (np.asarray(y, dtype=LD)[:, None] - eta) * np.sqrt(tau_)
    dens = LD(.5) * np.log(tau_ / (2 * LD(np.pi))) - LD(.5) * a * a
    sign = np.where(status == 1, -1., 1.)
    tail = log_ndtr((sign * a).astype(np.float64)).astype(LD)
    ll = np.where(status == 0, dens, tail)
    if ll_const is not None:
        ll = ll + np.asarray(ll_const, dtype=LD)[:, None]
    res = _summaries(np.exp(eta) if exp_mean else eta, ll)
    if points is not None:
        S = LD(eta.shape[1])
        x = (np.asarray(points, dtype=LD)[None, :, None] - eta[:, None, :]) \
            * np.sqrt(tau_)
        surv = ndtr(-x.astype(np.float64)).astype(LD)
        mean = surv.sum(axis=2) / S
        res['surv_mean'] = mean
        res['surv_sd'] = np.sqrt(((surv - mean[:, :, None]) ** 2).sum(axis=2)
                                 / S)
    return res


def _welford(x):
    """Mean and population sd over the last axis by the device's updates."""
    mean, m2 = np.zeros(x.shape[:-1]), np.zeros(x.shape[:-1])
    for k in range(x.shape[-1]):
        d = x[..., k] - mean
        mean = mean + d / (k + 1.)
        m2 = m2 + d * (x[..., k] - mean)
    return mean, np.sqrt(m2 / x.shape[-1])


def predict_recurrence(X, coef, tau, y, status, exp_mean=False, ll_const=None,
                       points=None):
    """The device's updates in float64, draw by draw (the accumulators'
    contract of csrc/predict_summary.hpp), the terms in the device's order of
    operations."""
    X, coef = np.asarray(X, dtype=np.float64), np.asarray(coef, np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    eta = np.zeros((X.shape[0], coef.shape[1]))
    for j in range(X.shape[1]):
        eta += X[:, j:j + 1] * coef[j]
    status = np.asarray(status)[:, None]
    a = (np.asarray(y, dtype=np.float64)[:, None] - eta) * np.sqrt(tau)
    hlt = .5 * np.log(tau / (2. * np.pi))
    sign = np.where(status == 1, -1., 1.)
    ll = np.where(status == 0, hlt - .5 * (a * a), log_ndtr(sign * a))
    if ll_const is not None:
        ll = ll + np.asarray(ll_const, dtype=np.float64)[:, None]
    mu = np.exp(eta) if exp_mean else eta
    n, S = mu.shape
    mean, sd = _welford(mu)
    lmean, lm2 = np.zeros(n), np.zeros(n)
    lmax, lsum = np.full(n, -np.inf), np.zeros(n)
    for k in range(S):
        x = ll[:, k]
        d = x - lmean
        lmean = lmean + d / (k + 1.)
        lm2 = lm2 + d * (x - lmean)
        up = x > lmax
        with np.errstate(invalid='ignore', over='ignore'):
            lsum = np.where(up, lsum * np.exp(lmax - x) + 1.,
                            lsum + np.exp(x - lmax))
        lmax = np.where(up, x, lmax)
    res = dict(zip(PRED_KEYS, (mean, sd,
                               lmax + np.log(lsum) - np.log(float(S)),
                               lmean, lm2 / (S - 1.))))
    if points is not None:
        from scipy.special import erfc
        x = (np.asarray(points, dtype=np.float64)[None, :, None]
             - eta[:, None, :]) * np.sqrt(tau)
        res['surv_mean'], res['surv_sd'] = _welford(
            .5 * erfc(0.70710678118654752440 * x))
    return res


SURV_KEYS = ('surv_mean', 'surv_sd')
# Largest rel_err of predict_recurrence against predict_explicit over
# predict_cases(), both models' forms and survival_points, measured
# (tests/test_censored_host_logic.py repeats it); the tolerance the device is
# held to is 16 x that rounded up to a power of ten, the rule of
# tests/test_hip_predict.py.
PRED_MEASURED = {'mean': 6.6e-16, 'sd': 6.5e-16, 'lpd': 2.3e-15,
                 'loglik_mean': 4.7e-16, 'loglik_var': 2.8e-15,
                 'surv_mean': 4.2e-16, 'surv_sd': 4.5e-16}
