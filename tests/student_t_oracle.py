"""NumPy restatement of the Student-t regression chain (the t-density as a scale
mixture of normals, under the bridge prior): what tests/test_hip_student_t.py
compares the device chain's posterior with, and the long-double log-likelihood
its iterations are checked against.  With r = y - psi, psi = X~ beta, one
iteration is, in this order,

  beta | omega, tau, tau_g, lam ~ N(A^-1 X~^T (Omega y), A^-1),
                        A = X~^T Omega X~ + diag(1 / sd^2), Omega = tau omega,
                        by a Cholesky factor (the device: 'cg', 'cholesky' or
                        'woodbury')
  tau | beta, omega     ~ Gamma(n/2) / (S/2), S = sum omega_i r_i^2 with the OLD
                        omega
  omega_i | beta, tau   ~ Gamma((nu+1)/2) / ((nu + tau r_i^2)/2) with the NEW tau
  tau_g | beta, lam | tau_g, beta   as bayesbridge.py:412-478, raw
                        parametrisation, the tilted stable variate from the
                        host sampler of libbbx_hostrng
X~ = [1, X - column means].  nu = None is the linear model: omega stays 1.
No GPU, no libbbx."""
from ctypes import c_void_p
from math import lgamma

import numpy as np
from numpy.random import PCG64, Generator

# the z-score helper, the relative error and the rule that turns a measured
# error into a tolerance: those of the probit oracle
from probit_oracle import (PRED_KEYS, batch_means, moments,  # noqa: F401
                           pred_tolerance, rel_err, shrunk_scale, z_scores)

LD = np.longdouble


def row_const(nu):
    return lgamma((nu + 1.) / 2.) - lgamma(nu / 2.) - .5 * np.log(nu / 2.)


def loglik(psi, y, tau, nu):
    """sum_i [1/2 log tau - (nu+1)/2 log1p(tau r_i^2 / nu)] + n [lgamma((nu+1)/2)
    - lgamma(nu/2) - 1/2 log(nu/2)] in long double (the constant in float64)."""
    r = np.asarray(y, dtype=LD) - np.asarray(psi, dtype=LD)
    tau, nu_ = LD(tau), LD(nu)
    terms = LD(.5) * np.log(tau) - (nu_ + 1) / 2 * np.log1p(tau * r * r / nu_)
    return float(terms.sum() + LD(len(r)) * LD(row_const(nu)))


def weights(gamma_draws, psi, y, tau, nu):
    """omega from its Gamma((nu+1)/2) variates: the division the device does."""
    r = np.asarray(y) - np.asarray(psi)
    return gamma_draws / ((nu + tau * (r * r)) / 2.)


class StudentTOracle():

    def __init__(self, y, X, nu=4., bridge_exponent=.5, sd_for_intercept=2.,
                 slab=2., gscale_shape=0., gscale_rate=0.):
        from math import gamma
        self.y = np.asarray(y, dtype=np.float64)
        X = np.asarray(X, dtype=np.float64)
        self.Xt = np.hstack([np.ones((X.shape[0], 1)), X - X.mean(axis=0)])
        self.nu = nu
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
        Xt, y, nu = self.Xt, self.y, self.nu
        n, P = Xt.shape
        alpha = self.alpha
        beta = np.zeros(P)
        beta[0] = np.median(y)
        lam = np.ones(P - 1)
        omega = np.ones(n)
        tau = 1. / np.mean((y - Xt @ beta) ** 2)
        kept = np.empty((n_iter - n_burnin, P + 1))
        for it in range(n_iter):
            prec = tau * omega
            sd = np.concatenate(([self.sd0],
                                 shrunk_scale(tau_g, lam, self.slab)))
            L = np.linalg.cholesky((Xt.T * prec) @ Xt + np.diag(sd ** -2.))
            mean = np.linalg.solve(L.T, np.linalg.solve(L, Xt.T @ (prec * y)))
            beta = mean + np.linalg.solve(L.T, rng.standard_normal(P))
            r2 = (y - Xt @ beta) ** 2
            tau = rng.gamma(n / 2.) / (np.sum(omega * r2) / 2.)
            if nu is not None:
                omega = rng.gamma((nu + 1.) / 2., size=n) \
                    / ((nu + tau * r2) / 2.)
            b = beta[1:]
            phi = rng.gamma(self.shape0 + b.size / alpha) \
                / (self.rate0 + np.sum(np.abs(b) ** alpha))
            tau_g = max(phi ** (-1. / alpha), self.lower_bd)
            lam = np.sqrt(.5 / self._tilted_stable(ts_bitgen,
                                                   (b / tau_g) ** 2))
            lam[lam == 0.] = 10e-16
            lam[np.isinf(lam)] = 2. / tau_g
            if it >= n_burnin:
                kept[it - n_burnin, :P] = beta
                kept[it - n_burnin, P] = tau
        return kept


def contaminated_problem(seed):
    """The posterior test's data: 400 x 12, planted slopes and intercept 0.3,
    N(0, 1) noise, and every tenth row (a random tenth) with N(m_i, 10^2) noise
    instead, m_i = 6 x_i1: a shift correlated with the first column, which
    biases a Gaussian fit's first slope and does not merely widen it."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((400, 12))
    beta = np.array([1.2, -1., .8, -.6, .4] + [0.] * 7)
    noise = rng.standard_normal(400)
    bad = rng.permutation(400)[:40]
    noise[bad] = 6. * X[bad, 0] + 10. * rng.standard_normal(40)
    return X, .3 + X @ beta + noise, beta


# ---- posterior prediction (StudentTModel.predict, csrc/student_t_predict.hip)

def predict_cases(nu=4.):
    """(n rows, S draws) -> (X raw [n, 5], coef [5, S], tau [S], y): the rows
    around a workgroup's edge, the draws around a pass of 16.  From 257 rows on
    the first and the last two rows hold residuals of +-1e3 and +-1e8 in every
    draw (column 0 is +-1 there and 0 elsewhere, its coefficient 1e3, the
    outcome of the outermost rows 1e8 away)."""
    out = {}
    for n in (1, 257, 4099):
        for S in (2, 16, 17, 33):
            rng = np.random.default_rng(200 * n + S)
            X = rng.standard_normal((n, 5))
            X[:, 0] = 0.
            coef = .7 * rng.standard_normal((5, S))
            coef[0] = 1e3
            tau = np.exp(rng.normal(0., 1., S))
            y = X @ coef[:, 0] + rng.standard_t(nu, n)
            if n >= 257:
                X[[0, 1, n - 2, n - 1]] = 0.
                X[[0, 1], 0], X[[n - 2, n - 1], 0] = 1., -1.
                y[[0, 1, n - 2, n - 1]] = [1e8, 0., 0., -1e8]
            out[n, S] = (X, coef, tau, y)
    return out


def _pred_terms(eta, tau, y, nu):
    """float64 terms (mu, ll) [n, S] from the linear predictors, the log density
    in the device's order of operations."""
    eta = np.asarray(eta, dtype=np.float64)
    r = np.asarray(y, dtype=np.float64)[:, None] - eta
    const = (lgamma((nu + 1.) / 2.) - lgamma(nu / 2.)) \
        + .5 * np.log(tau / (nu * np.pi))
    return eta, const - (nu + 1.) / 2. * np.log1p(tau * (r * r) / nu)


def predict_explicit(X, coef, tau, y, nu=4.):
    """The yardstick: eta and the terms in long double -- two-pass mean and
    population sd, logsumexp, var(ddof=1)."""
    eta = np.asarray(X, dtype=LD) @ np.asarray(coef, dtype=LD)
    tau_, nu_ = np.asarray(tau, dtype=LD), LD(nu)
    r = np.asarray(y, dtype=LD)[:, None] - eta
    const = LD(lgamma((nu + 1.) / 2.) - lgamma(nu / 2.)) \
        + LD(.5) * np.log(tau_ / (nu_ * LD(np.pi)))
    mu, ll = eta, const - (nu_ + 1) / 2 * np.log1p(tau_ * r * r / nu_)
    S = LD(mu.shape[1])
    mean = mu.sum(axis=1) / S
    sd = np.sqrt(((mu - mean[:, None]) ** 2).sum(axis=1) / S)
    top = ll.max(axis=1)
    lpd = top + np.log(np.exp(ll - top[:, None]).sum(axis=1)) - np.log(S)
    ll_mean = ll.sum(axis=1) / S
    ll_var = ((ll - ll_mean[:, None]) ** 2).sum(axis=1) / (S - 1)
    return dict(zip(PRED_KEYS, (mean, sd, lpd, ll_mean, ll_var)))


def predict_recurrence(X, coef, tau, y, nu=4.):
    """The device's updates in float64, draw by draw (the accumulators'
    contract of csrc/predict_summary.hpp)."""
    X, coef = np.asarray(X, dtype=np.float64), np.asarray(coef, np.float64)
    eta = np.zeros((X.shape[0], coef.shape[1]))
    for j in range(X.shape[1]):
        eta += X[:, j:j + 1] * coef[j]
    mu, ll = _pred_terms(eta, np.asarray(tau, dtype=np.float64), y, nu)
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


# Largest rel_err of predict_recurrence against predict_explicit over
# predict_cases(), measured (tests/test_student_t_host_logic.py repeats it); the
# tolerance the device is held to is 16 x that rounded up to a power of ten,
# the rule of tests/test_hip_predict.py.
PRED_MEASURED = {'mean': 8.8e-16, 'sd': 2.4e-16, 'lpd': 1.9e-16,
                 'loglik_mean': 2.0e-16, 'loglik_var': 2.5e-15}
