"""CPU statement of the n-space ('woodbury') coefficient draw (DESIGN.md 11:
Bhattacharya, Chakraborty and Mallick 2016, extended to coefficients with a
flat prior), of the Gaussian it must equal, and of a Gibbs loop that uses it,
for the tests of the woodbury sampler (oracle/ stays as it is).  NumPy/SciPy
only."""
import numpy as np
import scipy.linalg

from oracle.gibbs import OracleGibbs


def transposed_fisher_info(Xt, weight):
    """X~ diag(w) X~^T, w over the columns."""
    return (Xt * np.asarray(weight, dtype=np.float64)[None, :]) @ Xt.T


def woodbury_draw(Xt, obs_prec, prior_prec_sqrt, y, delta, xi):
    """The draw with its n + P normals given (xi[j] belongs to coefficient j;
    zeros of prior_prec_sqrt mark the coefficients with a flat prior)."""
    n, P = Xt.shape
    pps = np.asarray(prior_prec_sqrt, dtype=np.float64)
    s = np.sqrt(np.asarray(obs_prec, dtype=np.float64) * np.ones(n))
    F = np.flatnonzero(pps == 0)
    live = (pps > 0) & np.isfinite(pps)
    d, u = np.zeros(P), np.zeros(P)
    d[live] = 1 / pps[live] ** 2
    u[live] = xi[live] / pps[live]
    Phi = s[:, None] * Xt
    alpha = s * y
    M = s[:, None] * transposed_fisher_info(Xt, d) * s[None, :] + np.eye(n)
    L = scipy.linalg.cholesky(M, lower=True)
    r = alpha - Phi @ u - delta
    q = len(F)
    if q:
        PF = Phi[:, F]
        LC = scipy.linalg.cholesky(PF.T @ PF, lower=True)
        r = r - PF @ scipy.linalg.cho_solve((LC, True), PF.T @ r)
        Z = scipy.linalg.cho_solve((L, True), np.column_stack((r, PF)))
        lam = -np.linalg.solve(PF.T @ Z[:, 1:], PF.T @ Z[:, 0])
        w = Z[:, 0] + Z[:, 1:] @ lam
    else:
        w = scipy.linalg.cho_solve((L, True), r)
    beta = u + d * (Phi.T @ w)
    if q:
        g = PF.T @ (alpha - Phi @ beta)
        beta[F] = scipy.linalg.cho_solve((LC, True), g) \
            + scipy.linalg.solve_triangular(LC.T, xi[F], lower=False)
    return beta


def affine_map(draw, n, P):
    """(m, T) of a draw that is affine in its normals, beta = m + T [delta; xi],
    from n + P + 1 calls of draw(delta, xi)."""
    m = draw(np.zeros(n), np.zeros(P))
    T = np.empty((P, n + P))
    for k in range(n + P):
        e = np.zeros(n + P)
        e[k] = 1.
        T[:, k] = draw(e[:n], e[n:]) - m
    return m, T


def explicit_posterior(Xt, obs_prec, prior_prec_sqrt, y):
    """(A^-1 X~^T Omega y, A^-1), A = X~^T Omega X~ + diag(prior_prec_sqrt^2)."""
    w = np.asarray(obs_prec, dtype=np.float64) * np.ones(Xt.shape[0])
    pps = np.where(np.isfinite(prior_prec_sqrt), prior_prec_sqrt, 1e150)
    A = Xt.T @ (w[:, None] * Xt) + np.diag(pps ** 2)
    cov = np.linalg.inv(A)
    cov = .5 * (cov + cov.T)
    return cov @ (Xt.T @ (w * y)), cov


def case(name, seed=0):
    """The small problems of the tests: (Xt, obs_prec, prior_prec_sqrt, y).
    n < P and n > P; q = 0, 1, 3 flat coefficients; logit-like weights or one
    number (linear); one unshrunk coefficient with a finite sd; prior scales
    over several decades as under the bridge prior.  `name`: one of CASES, or
    the shape itself, (n, P, q, linear)."""
    shapes = {
        'wide_q1_logit': (40, 130, 1, False), 'wide_q0_logit': (40, 130, 0, False),
        'wide_q3_linear': (70, 200, 3, True), 'tall_q1_logit': (150, 60, 1, False),
        'tall_q3_linear': (150, 60, 3, True), 'wide_q0_linear': (33, 97, 0, True),
    }
    if isinstance(name, str):
        n, P, q, linear = shapes[name]
        rng = np.random.default_rng(1000 + seed + len(name))
    else:
        n, P, q, linear = name
        rng = np.random.default_rng([2000 + seed, n, P, q, int(linear)])
    X = rng.normal(size=(n, P - 1))
    X[:, ::3] = (rng.random((n, len(range(0, P - 1, 3)))) < .3)
    X = X - X.mean(axis=0)
    Xt = np.hstack((np.ones((n, 1)), X))
    sd = .5 * np.exp(rng.normal(0., 1.5, P))
    pps = 1 / sd
    pps[:q] = 0.
    pps[q] = 1 / 2.                 # an unshrunk coefficient with sd 2
    if linear:
        obs_prec = 1.7
        y = Xt[:, 1:6] @ rng.normal(size=5) + rng.normal(size=n) / np.sqrt(1.7)
    else:
        obs_prec = rng.gamma(2., .15, n) + 1e-3
        y = (rng.integers(0, 2, n) - .5) / obs_prec
    return Xt, obs_prec, pps, y


CASES = ('wide_q1_logit', 'wide_q0_logit', 'wide_q3_linear', 'tall_q1_logit',
         'tall_q3_linear', 'wide_q0_linear')


class OracleWoodburyGibbs(OracleGibbs):
    """OracleGibbs with the coefficient step drawn by woodbury_draw: delta =
    randn(n), then xi = randn(P), from the global NumPy stream; no summariser
    update."""

    def draw_coef(self, obs_prec, gscale, lscale, summ, record=None):
        from oracle.gibbs import regularized_prior_scale
        from cholesky_oracle import explicit
        if self.family == 'linear':
            y_gauss = self.outcome
            omega = obs_prec * np.ones(self.n)
        else:
            omega = obs_prec
            y_gauss = (self.outcome[0] - self.outcome[1] / 2) / obs_prec
        prior_sd = np.concatenate((
            self.sd_unshrunk,
            regularized_prior_scale(gscale, lscale, self.slab)))
        with np.errstate(divide='ignore'):
            pps = 1 / prior_sd
        if not hasattr(self, '_Xt'):
            self._Xt = explicit(self.design)
        delta = np.random.randn(self.n)
        xi = np.random.randn(self.P)
        coef = woodbury_draw(self._Xt, omega, pps, y_gauss, delta, xi)
        return coef, {'n_iter': 0}
