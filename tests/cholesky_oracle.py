"""CPU restatement of the reference's direct ('cholesky') coefficient draw
(direct_gaussian_sampler.py:4-44) and of its Gibbs loop, for the tests of the
cholesky sampler (oracle/ stays as it is).  NumPy/SciPy only."""
import numpy as np
import scipy.linalg

from oracle.gibbs import OracleGibbs


def explicit(design):
    """X~ as an n x P array, column by column from the design's dot."""
    n, P = design.shape
    out, e = np.empty((n, P)), np.zeros(P)
    for j in range(P):
        e[j] = 1.
        out[:, j] = design.dot(e)
        e[j] = 0.
    return out


def fisher_info(Xt, weight, diag_only=False):
    """X~^T diag(w) X~ (dense_matrix.py:54-58)."""
    if diag_only:
        return np.sum(weight[:, None] * Xt ** 2, axis=0)
    return Xt.T @ (weight[:, None] * Xt)


def chol_draw(Xt, obs_prec, prior_prec_sqrt, z, normals):
    """generate_gaussian_with_weight with the P normals given."""
    w = np.asarray(obs_prec, dtype=np.float64) * np.ones(Xt.shape[0])
    d = prior_prec_sqrt ** 2 + fisher_info(Xt, w, diag_only=True)
    s = 1 / np.sqrt(d)
    A = s[:, None] * fisher_info(Xt, w) * s[None, :]
    A += np.diag((s * prior_prec_sqrt) ** 2)
    U = scipy.linalg.cholesky(A, lower=False)                # A = U^T U
    mean = scipy.linalg.cho_solve((U, False), s * z)
    return s * (mean + scipy.linalg.solve_triangular(U, normals, lower=False))


class OracleCholeskyGibbs(OracleGibbs):
    """OracleGibbs with the coefficient step of the 'cholesky' branch
    (reg_coef_sampler.py:81-84): normals from the global NumPy stream, no
    summariser update."""

    def draw_coef(self, obs_prec, gscale, lscale, summ, record=None):
        from oracle.gibbs import regularized_prior_scale
        if self.family == 'linear':
            y_gauss = self.outcome
            omega = obs_prec * np.ones(self.n)
        else:
            omega = obs_prec
            y_gauss = (self.outcome[0] - self.outcome[1] / 2) / obs_prec
        z = self.design.Tdot(omega * y_gauss)
        prior_sd = np.concatenate((
            self.sd_unshrunk,
            regularized_prior_scale(gscale, lscale, self.slab)))
        with np.errstate(divide='ignore'):
            pps = 1 / prior_sd
        if not hasattr(self, '_Xt'):
            self._Xt = explicit(self.design)
        g = np.random.randn(self.P)
        coef = chol_draw(self._Xt, omega, pps, z, g)
        return coef, {'n_iter': 0}
