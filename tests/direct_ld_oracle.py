"""Long-double (80-bit, eps 1.08e-19) statements of what the two direct
samplers compute -- the weighted Gram, the preconditioned matrix, its Cholesky
factor, the 'cholesky' draw (cholesky_oracle.chol_draw) and the 'woodbury' draw
(woodbury_oracle.woodbury_draw) -- and the small problems that the CPU tests
(test_direct_ld_oracle.py) and the GPU tests (test_hip_direct_edges.py) share.

Plain NumPy.  The factorisation and the substitutions are unblocked loops over
columns, vectorised over rows (NumPy's products of long-double arrays are its
generic loops, no BLAS), so nothing here shares a summation order or a code
path with the device's blocked kernels or with LAPACK.  P <= 200 takes about
0.1 s.  Every input is float64; every product is formed in long double."""
import functools
from types import SimpleNamespace

import numpy as np

LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=LD)


# ---- linear algebra ---------------------------------------------------------
def gram_ld(Xt, w):
    """X~^T diag(w) X~ (w: n numbers or one)."""
    X = _ld(Xt)
    w = _ld(w) * np.ones(X.shape[0], dtype=LD)
    return X.T @ (w[:, None] * X)


def precond_ld(Xt, w, pps):
    """(A, s): d = pps^2 + diag F, s = 1 / sqrt(d),
    A = s F s + diag((s pps)^2), F = X~^T diag(w) X~."""
    F = gram_ld(Xt, w)
    p = _ld(pps)
    d = p * p + np.diag(F)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = 1 / np.sqrt(d)
        A = s[:, None] * F * s[None, :]
        t = s * p
        A[np.diag_indices_from(A)] += t * t
    return A, s


def chol_ld(A):
    """(L, first_bad, pivots) of A = L L^T, unblocked, left-looking.
    first_bad: the first column whose pivot is not > 0 or not finite (the
    factorisation stops there), else None; pivots: the pivot values up to and
    including that column."""
    A = _ld(A)
    P = A.shape[0]
    L = np.zeros((P, P), dtype=LD)
    pivots = []
    for j in range(P):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        p = v[0]
        pivots.append(p)
        if not (p > 0) or not np.isfinite(p):
            return L, j, pivots
        L[j:, j] = v / np.sqrt(p)
    return L, None, pivots


def fwd_ld(L, b):
    """L^-1 b, column-oriented."""
    x = _ld(b).copy()
    for j in range(L.shape[0]):
        x[j] = x[j] / L[j, j]
        x[j + 1:] -= L[j + 1:, j] * x[j]
    return x


def bwd_ld(L, b):
    """L^-T b."""
    x = _ld(b).copy()
    for j in range(L.shape[0] - 1, -1, -1):
        x[j] = x[j] / L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


def cho_solve_ld(L, B):
    B = _ld(B)
    if B.ndim == 1:
        return bwd_ld(L, fwd_ld(L, B))
    return np.column_stack([bwd_ld(L, fwd_ld(L, B[:, k]))
                            for k in range(B.shape[1])])


def solve_ld(M, b):
    """M^-1 b for a small square M: elimination with partial pivoting."""
    M, b = _ld(M).copy(), _ld(b).copy()
    q = M.shape[0]
    for j in range(q):
        k = j + int(np.argmax(np.abs(M[j:, j])))
        if k != j:
            M[[j, k]] = M[[k, j]]
            b[[j, k]] = b[[k, j]]
        f = M[j + 1:, j] / M[j, j]
        M[j + 1:] -= f[:, None] * M[j]
        b[j + 1:] -= f * b[j]
    for j in range(q - 1, -1, -1):
        b[j] = (b[j] - M[j, j + 1:] @ b[j + 1:]) / M[j, j]
    return b


def _spd_factor(A):
    L, bad, _ = chol_ld(A)
    if bad is not None:
        raise np.linalg.LinAlgError("pivot %d is not > 0" % bad)
    return L


def chol_draw_ld(Xt, w, pps, z, g):
    """cholesky_oracle.chol_draw in long double:
    s (A^-1 (s z) + L^-T g), A = L L^T."""
    A, s = precond_ld(Xt, w, pps)
    L = _spd_factor(A)
    return s * bwd_ld(L, fwd_ld(L, s * _ld(z)) + _ld(g))


def woodbury_draw_ld(Xt, obs_prec, pps, y, delta, xi):
    """woodbury_oracle.woodbury_draw with every array and every solve (the
    q x q systems too) in long double."""
    X = _ld(Xt)
    n, P = X.shape
    pps64 = np.asarray(pps, dtype=np.float64)
    p, y, delta, xi = _ld(pps64), _ld(y), _ld(delta), _ld(xi)
    s = np.sqrt(_ld(obs_prec) * np.ones(n, dtype=LD))
    F = np.flatnonzero(pps64 == 0)
    live = (pps64 > 0) & np.isfinite(pps64)
    d, u = np.zeros(P, dtype=LD), np.zeros(P, dtype=LD)
    d[live] = 1 / (p[live] * p[live])
    u[live] = xi[live] / p[live]
    Phi = s[:, None] * X
    alpha = s * y
    M = s[:, None] * ((X * d[None, :]) @ X.T) * s[None, :]
    M[np.diag_indices_from(M)] += 1
    L = _spd_factor(M)
    r = alpha - Phi @ u - delta
    q = len(F)
    if q:
        PF = Phi[:, F]
        LC = _spd_factor(PF.T @ PF)
        r = r - PF @ cho_solve_ld(LC, PF.T @ r)
        Z = cho_solve_ld(L, np.column_stack((r, PF)))
        lam = -solve_ld(PF.T @ Z[:, 1:], PF.T @ Z[:, 0])
        w = Z[:, 0] + Z[:, 1:] @ lam
    else:
        w = cho_solve_ld(L, r)
    beta = u + d * (Phi.T @ w)
    if q:
        g = PF.T @ (alpha - Phi @ beta)
        beta[F] = cho_solve_ld(LC, g) + bwd_ld(LC, xi[F])
    return beta


def backward_error(A, x, b):
    """max|A x - b| / (||A||_inf max|x| + max|b|), in long double."""
    A, x, b = _ld(A), _ld(x), _ld(b)
    r = np.abs(A @ x - b).max()
    return r / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())


def cond_2(A):
    """2-norm condition of a symmetric positive definite A (float64 suffices
    for a figure that is only reported)."""
    ev = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
    return float(ev[-1] / ev[0])


# ---- the cases --------------------------------------------------------------
# A case: Xt (X~, n x P float64, as the design stores it), intercept (column 0
# of Xt is the ones the design adds), w[n], pps[P], z[P], g[P].
def _finish(rng, Xt, intercept, w, pps, **more):
    P = Xt.shape[1]
    return SimpleNamespace(Xt=np.ascontiguousarray(Xt), intercept=intercept,
                           w=w, pps=pps, z=rng.normal(size=P),
                           g=rng.normal(size=P), **more)


def _centred(rng, n, p, scale=None):
    X = rng.normal(size=(n, p)) + .3 * rng.normal(size=(n, 1))
    if scale is not None:
        X = X * scale
    X = X - X.mean(axis=0)
    return np.hstack((np.ones((n, 1)), X))


@functools.lru_cache(maxsize=None)
def well(P, n=200, seed=0):
    """A generic case: intercept, centred columns, w ~ Gamma(2, .2),
    pps = exp(N(0, 1)), pps[0] = 0."""
    rng = np.random.default_rng(7000 + 13 * P + n + seed)
    Xt = _centred(rng, n, P - 1)
    w = rng.gamma(2., .2, n)
    pps = np.exp(rng.normal(0., 1., P))
    pps[0] = 0.
    return _finish(rng, Xt, True, w, pps)


@functools.lru_cache(maxsize=None)
def collinear(P=129, n=400):
    """Columns 64 and 65 are combinations of columns 62, 63 and 1 up to 1e-6
    noise, and the five columns of the group have pps = 1e-4 (a prior of
    ordinary strength on 62, 63 and 1 alone would hold the group's null
    directions: cond(A) stays near 3e3): a collinear group across the first
    block boundary, cond(A) 3.8e11."""
    rng = np.random.default_rng(7101)
    Xt = _centred(rng, n, P - 1)
    for j in (64, 65):
        c = rng.normal(size=3)
        Xt[:, j] = Xt[:, [62, 63, 1]] @ c + 1e-6 * rng.normal(size=n)
        Xt[:, j] -= Xt[:, j].mean()
    w = rng.gamma(2., .2, n)
    pps = np.exp(rng.normal(0., 1., P))
    pps[0] = 0.
    pps[[1, 62, 63, 64, 65]] = 1e-4
    return _finish(rng, Xt, True, w, pps)


@functools.lru_cache(maxsize=None)
def rankdef(P=193, n=100):
    """n < P: F has rank n and a weak prior (pps[1:] = 1e-3 exp(N(0, 1)))
    carries the rest."""
    rng = np.random.default_rng(7102)
    Xt = _centred(rng, n, P - 1)
    w = rng.gamma(2., .2, n)
    pps = 1e-3 * np.exp(rng.normal(0., 1., P))
    pps[0] = 0.
    return _finish(rng, Xt, True, w, pps)


@functools.lru_cache(maxsize=None)
def scales(P=129, n=400):
    """Column scales exp(N(0, 4^2)) and pps[1:] = exp(N(0, 6^2)): the diagonal
    preconditioning has to absorb them; the coefficients span decades."""
    rng = np.random.default_rng(7103)
    scale = np.exp(rng.normal(0., 4., P - 1))
    Xt = _centred(rng, n, P - 1, scale)
    w = rng.gamma(2., .2, n)
    pps = np.exp(rng.normal(0., 6., P))
    pps[0] = 0.
    return _finish(rng, Xt, True, w, pps)


@functools.lru_cache(maxsize=None)
def indefinite(P=129, j0=64, n=200):
    """A generic positive definite case without intercept or centring, plus
    one appended row e_j per j in j0 (an int or a tuple) with the negative
    weight -(1 - 1e-3) (pps_j^2 + F_jj): d_j stays positive but small, the
    scaled off-diagonals of column j exceed 1 and pivot j is the first that
    is not > 0.  j0 == 0: the weight is -(1 + 1e-3) (...), d_0 < 0, s_0 and
    pivot 0 are NaN.  `w_valid` is w with zeros for the appended rows: the
    positive definite problem on the same design."""
    cols = (j0,) if isinstance(j0, int) else tuple(j0)
    rng = np.random.default_rng(7200 + 7 * sum(cols) + len(cols))
    X = rng.normal(size=(n, P)) + .4 * rng.normal(size=(n, 1))
    w = rng.gamma(2., .2, n)
    pps = np.exp(rng.normal(0., 1., P))
    Fd = (w[:, None] * X ** 2).sum(axis=0)
    extra = np.zeros((len(cols), P))
    w_extra = np.empty(len(cols))
    for k, j in enumerate(cols):
        extra[k, j] = 1.
        f = 1 + 1e-3 if j == 0 else 1 - 1e-3
        w_extra[k] = -f * (pps[j] ** 2 + Fd[j])
    Xt = np.vstack((X, extra))
    return _finish(rng, Xt, False, np.concatenate((w, w_extra)), pps,
                   w_valid=np.concatenate((w, np.zeros(len(cols)))),
                   cols=cols)


INDEFINITE_J0 = (63, 64, 127, 128, 0)


@functools.lru_cache(maxsize=None)
def chol_ref(kind, *args, alpha=None, valid=False):
    """chol_draw_ld of a case, computed once per process (read-only).
    alpha: the scalar path's obs_prec in place of the case's w; valid: an
    indefinite case's w_valid."""
    c = globals()[kind](*args)
    w = c.w_valid if valid else (c.w if alpha is None else alpha)
    out = chol_draw_ld(c.Xt, w, c.pps, c.z, c.g)
    out.setflags(write=False)
    return out


def mean_backward_error(c, mean_coef):
    """backward_error of a draw's mean part (normals = 0) given as
    coefficients: x = mean_coef / s against A x = s z on the long-double A."""
    A, s = precond_ld(c.Xt, c.w, c.pps)
    return backward_error(A, _ld(mean_coef) / s, s * _ld(c.z))


@functools.lru_cache(maxsize=None)
def float64_figures(kind, *args):
    """What the float64 restatement (cholesky_oracle.chol_draw: NumPy, LAPACK)
    is off by on a case, measured against long double; nothing here looks at
    the device.  (E64, eta64, rel64):
      E64   = max|chol_draw - chol_draw_ld| / max(1, max|ref_ld|)
      eta64 = backward_error of its mean part (g = 0) on the long-double A
      rel64 = max_j |chol_draw_j - ref_j| / max(1e-300, |ref_j|)"""
    from cholesky_oracle import chol_draw
    c = globals()[kind](*args)
    ref = chol_ref(kind, *args)
    f = chol_draw(c.Xt, c.w, c.pps, c.z, c.g)
    err = np.abs(f - ref)
    E64 = float(err.max() / max(1., np.abs(ref).max()))
    rel64 = float((err / np.maximum(1e-300, np.abs(ref))).max())
    m = chol_draw(c.Xt, c.w, c.pps, c.z, np.zeros_like(c.g))
    return E64, float(mean_backward_error(c, m)), rel64


# The factor a device figure may exceed the float64 restatement's by: both
# factorisations are backward stable with bounds of the form c P u and differ
# in summation order only (LABNOTES, "Direct samplers at 64-block edges").
FACTOR = 32.


def kappa(rel64):
    """By how much the 1e-10 figure has to grow to be held per coefficient:
    not at all unless the float64 restatement's own worst per-coefficient
    error, with FACTOR, is above it."""
    return max(1., FACTOR * rel64 / 1e-10)
