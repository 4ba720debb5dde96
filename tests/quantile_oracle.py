"""NumPy restatement of the quantile regression chain (the asymmetric-Laplace
likelihood as a scale mixture of normals, Kozumi & Kobayashi 2011, under the
bridge prior): what tests/test_hip_quantile.py compares the device chain's
posterior with, the long-double log-likelihood its iterations are checked
against, and a random-walk Metropolis chain on the MARGINAL posterior that the
augmentation itself is checked against (tests/test_quantile_replay_cpu.py).
With q the level, qq = q (1 - q), theta = (1 - 2q) / qq, kappa2 = 2 / qq, r = y
- psi, psi = X~ beta and w = 1 / v the stored latent, one iteration is, in this
order,

  beta | w, tau, tau_g, lam ~ N(A^-1 X~^T kappa, A^-1), A = X~^T Omega X~ +
                        diag(1 / sd^2), Omega_i = tau w_i / kappa2, kappa_i =
                        Omega_i y_i - tau theta / kappa2, by a Cholesky factor
                        (the device: 'cg', 'cholesky' or 'woodbury')
  tau | beta, w         ~ Gamma(3n/2) / S, S = sum_i [1 / w_i + w_i (r_i -
                        theta / w_i)^2 / (2 kappa2)] with the OLD w
  w_i | beta, tau       ~ InverseGaussian(mean 1 / (qq |r_i|), shape tau /
                        (2 qq)) with the NEW tau
  tau_g | beta, lam | tau_g, beta   as bayesbridge.py:412-478 (fixed_sd: the
                        prior scales are held at these values instead)
X~ = [1, X - column means].  No GPU, no libbbx."""
from ctypes import c_void_p

import numpy as np
from numpy.random import PCG64, Generator

from probit_oracle import (PRED_KEYS, batch_means, moments,  # noqa: F401
                           pred_tolerance, rel_err, shrunk_scale, z_scores)
from student_t_oracle import predict_cases  # noqa: F401  (the shapes)

LD = np.longdouble


def level(q):
    """(qq, theta, kappa2) of the level q."""
    qq = q * (1. - q)
    return qq, (1. - 2. * q) / qq, 2. / qq


def check_loss(r, q):
    """rho_q(r) = r (q - 1[r < 0])."""
    r = np.asarray(r)
    return r * np.where(r < 0., q - 1., q)


def loglik(psi, y, tau, q):
    """sum_i [log tau - tau rho_q(r_i)] + n log(q (1 - q)) in long double."""
    r = np.asarray(y, dtype=LD) - np.asarray(psi, dtype=LD)
    tau, q_ = LD(tau), LD(q)
    rho = r * np.where(r < 0, q_ - 1, q_)
    return float((np.log(tau) - tau * rho).sum()
                 + LD(len(r)) * np.log(q_ * (1 - q_)))


def tau_sum(w, r, q):
    """S of tau's conditional, every term positive."""
    _, theta, kappa2 = level(q)
    v = 1. / w
    return np.sum(v + w * (r - theta * v) ** 2 / (2. * kappa2))


class QuantileOracle():

    def __init__(self, y, X, q=.5, bridge_exponent=.5, sd_for_intercept=2.,
                 slab=2., gscale_shape=0., gscale_rate=0., fixed_sd=None,
                 theta_zero=False):
        from math import gamma
        self.y = np.asarray(y, dtype=np.float64)
        X = np.asarray(X, dtype=np.float64)
        self.Xt = np.hstack([np.ones((X.shape[0], 1)), X - X.mean(axis=0)])
        self.q = q
        self.alpha, self.sd0, self.slab = bridge_exponent, sd_for_intercept, \
            slab
        self.shape0, self.rate0 = gscale_shape, gscale_rate
        self.fixed_sd = fixed_sd
        # the negative control of the augmentation's check: the shift dropped
        self.theta_zero = theta_zero
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
        Xt, y, q = self.Xt, self.y, self.q
        qq, theta, kappa2 = level(q)
        if self.theta_zero:
            theta = 0.
        n, P = Xt.shape
        alpha = self.alpha
        beta = np.zeros(P)
        beta[0] = np.quantile(y, q)
        lam = np.ones(P - 1)
        w = np.ones(n)
        tau = 1. / np.mean(check_loss(y - Xt @ beta, q))
        kept = np.empty((n_iter - n_burnin, P + 1))
        for it in range(n_iter):
            prec = tau * w / kappa2
            kap = prec * y - tau * theta / kappa2
            sd = self.fixed_sd if self.fixed_sd is not None else \
                np.concatenate(([self.sd0],
                                shrunk_scale(tau_g, lam, self.slab)))
            L = np.linalg.cholesky((Xt.T * prec) @ Xt + np.diag(sd ** -2.))
            mean = np.linalg.solve(L.T, np.linalg.solve(L, Xt.T @ kap))
            beta = mean + np.linalg.solve(L.T, rng.standard_normal(P))
            r = y - Xt @ beta
            v = 1. / w
            S = np.sum(v + w * (r - theta * v) ** 2 / (2. * kappa2))
            tau = rng.gamma(1.5 * n) / S
            w = rng.wald(1. / (qq * np.abs(r)), tau / (2. * qq))
            if self.fixed_sd is None:
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


def metropolis(y, X, q, sd, n_iter, n_burnin, seed, thin=10, step=None):
    """Random-walk Metropolis on (beta, log tau) of the MARGINAL posterior --
    the asymmetric-Laplace likelihood itself, beta_j ~ N(0, sd_j^2), p(tau) =
    1 / tau (flat in log tau) -- with no augmentation anywhere.  Kept draws
    [(n_iter - n_burnin) / thin, P + 1]: the coefficients, then tau."""
    rng = Generator(PCG64(seed))
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    Xt = np.hstack([np.ones((X.shape[0], 1)), X - X.mean(axis=0)])
    n, P = Xt.shape

    def logp(beta, lt):
        r = y - Xt @ beta
        return n * lt - np.exp(lt) * np.sum(r * np.where(r < 0., q - 1., q)) \
            - .5 * np.sum((beta / sd) ** 2)

    beta = np.zeros(P)
    beta[0] = np.quantile(y, q)
    lt = -np.log(np.mean(check_loss(y - Xt @ beta, q)))
    if step is None:
        # a posterior sd is of order 1 / (tau sqrt(n)) per unit column
        step = np.concatenate((np.full(P, .8 * np.exp(-lt) / np.sqrt(n)),
                               [.8 / np.sqrt(n)]))
    cur = logp(beta, lt)
    kept = np.empty(((n_iter - n_burnin) // thin, P + 1))
    accepted = 0
    for it in range(n_iter):
        move = step * rng.standard_normal(P + 1)
        b2, lt2 = beta + move[:P], lt + move[P]
        new = logp(b2, lt2)
        if np.log(rng.random()) < new - cur:
            beta, lt, cur = b2, lt2, new
            accepted += 1
        k = it - n_burnin
        if k >= 0 and k % thin == 0 and k // thin < len(kept):
            kept[k // thin, :P] = beta
            kept[k // thin, P] = np.exp(lt)
    return kept, accepted / n_iter


def augmentation_problem(seed=4):
    """The 40 x 3 problem of the augmentation's check: skewed noise, q = .25,
    fixed prior scales (intercept 2, slopes 1)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((40, 3))
    y = .5 + X @ np.array([1., -.5, 0.]) + rng.standard_exponential(40) - .3
    return X, y, .25, np.array([2., 1., 1., 1.])


def skewed_scale_problem(seed):
    """The posterior test's data: 400 x 12, planted slopes and intercept 0.3,
    N(0, 1) noise of scale exp(.5 x_1): the conditional q-quantile at q = .8 is
    not linear in x_1 and its best linear fit has another first slope and
    another intercept than the mean's, which a Gaussian fit estimates."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((400, 12))
    beta = np.array([1.2, -1., .8, -.6, .4] + [0.] * 7)
    noise = np.exp(.5 * X[:, 0]) * rng.standard_normal(400)
    return X, .3 + X @ beta + noise, beta


# ---- posterior prediction (QuantileModel.predict, csrc/quantile_predict.hip)

def _pred_terms(eta, tau, y, q):
    """float64 terms (mu, ll) [n, S] from the linear predictors, the log density
    in the device's order of operations."""
    eta = np.asarray(eta, dtype=np.float64)
    r = np.asarray(y, dtype=np.float64)[:, None] - eta
    hlt = np.log(tau) + np.log(q * (1. - q))
    return eta, hlt - tau * (r * np.where(r < 0., q - 1., q))


def predict_explicit(X, coef, tau, y, q):
    """The yardstick: eta and the terms in long double -- two-pass mean and
    population sd, logsumexp, var(ddof=1)."""
    eta = np.asarray(X, dtype=LD) @ np.asarray(coef, dtype=LD)
    tau_, q_ = np.asarray(tau, dtype=LD), LD(q)
    r = np.asarray(y, dtype=LD)[:, None] - eta
    mu = eta
    ll = np.log(tau_) + np.log(q_ * (1 - q_)) \
        - tau_ * (r * np.where(r < 0, q_ - 1, q_))
    S = LD(mu.shape[1])
    mean = mu.sum(axis=1) / S
    sd = np.sqrt(((mu - mean[:, None]) ** 2).sum(axis=1) / S)
    top = ll.max(axis=1)
    lpd = top + np.log(np.exp(ll - top[:, None]).sum(axis=1)) - np.log(S)
    ll_mean = ll.sum(axis=1) / S
    ll_var = ((ll - ll_mean[:, None]) ** 2).sum(axis=1) / (S - 1)
    return dict(zip(PRED_KEYS, (mean, sd, lpd, ll_mean, ll_var)))


def predict_recurrence(X, coef, tau, y, q):
    """The device's updates in float64, draw by draw (the accumulators'
    contract of csrc/predict_summary.hpp)."""
    X, coef = np.asarray(X, dtype=np.float64), np.asarray(coef, np.float64)
    eta = np.zeros((X.shape[0], coef.shape[1]))
    for j in range(X.shape[1]):
        eta += X[:, j:j + 1] * coef[j]
    mu, ll = _pred_terms(eta, np.asarray(tau, dtype=np.float64), y, q)
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
        # (the branch np.where does not take: exp(x + inf) at the first draw)
        with np.errstate(invalid='ignore', over='ignore'):
            lsum = np.where(up, lsum * np.exp(lmax - x) + 1.,
                            lsum + np.exp(x - lmax))
        lmax = np.where(up, x, lmax)
    return dict(zip(PRED_KEYS, (mean, np.sqrt(m2 / S),
                                lmax + np.log(lsum) - np.log(float(S)),
                                lmean, lm2 / (S - 1.))))


PRED_Q = .25
# Largest rel_err of predict_recurrence against predict_explicit over
# predict_cases() at q = PRED_Q, measured (tests/test_quantile_host_logic.py
# repeats it); the tolerance the device is held to is 16 x that rounded up to a
# power of ten, the rule of tests/test_hip_predict.py.
PRED_MEASURED = {'mean': 8.8e-16, 'sd': 2.4e-16, 'lpd': 1.5e-16,
                 'loglik_mean': 1.7e-16, 'loglik_var': 4.3e-16}
