"""CPU: the long-double oracle of the direct samplers (tests/direct_ld_oracle.py)
against the float64 restatements the suite has used so far, and the conditions
that its cases are built to meet.  The figures that tests/test_hip_direct_edges.py
derives its bounds from are measured (and printed) here; LABNOTES, "Direct
samplers at 64-block edges", records them."""
import numpy as np
import pytest
import scipy.linalg

import direct_ld_oracle as ldo
from cholesky_oracle import chol_draw
from woodbury_oracle import CASES, case, woodbury_draw

EDGE_P = (1, 2, 63, 64, 65, 127, 128, 129, 193)
WB_EDGE = [(n, n + 70, q, False) for n in (63, 64, 65, 128, 129)
           for q in (0, 1, 3)] + [(64, 134, 1, True), (129, 199, 3, True)]


def _rel(a, ref):
    return float(np.abs(a - ref).max() / max(1., np.abs(ref).max()))


def test_long_double_is_the_80_bit_type():
    assert np.finfo(np.longdouble).eps < 1.1e-19


def test_gram_and_factor_restate_numpy():
    c = ldo.well(65)
    F = ldo.gram_ld(c.Xt, c.w)
    ref = c.Xt.T @ (c.w[:, None] * c.Xt)
    assert np.abs(F - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.abs(F - F.T).max() <= 1e-18 * np.abs(ref).max()
    A, s = ldo.precond_ld(c.Xt, c.w, c.pps)
    assert np.abs(np.diag(A) - 1).max() <= 1e-18
    L, bad, piv = ldo.chol_ld(A)
    assert bad is None and len(piv) == 65 and min(piv) > 0
    assert np.abs(L @ L.T - A).max() <= 1e-17
    U = scipy.linalg.cholesky(np.asarray(A, dtype=np.float64))
    assert np.abs(L.T - U).max() <= 1e-13
    x = ldo.cho_solve_ld(L, s * c.z)
    assert ldo.backward_error(A, x, s * c.z) <= 1e-18
    assert ldo.backward_error(A, 1.001 * x, s * c.z) > 1e-5


@pytest.mark.parametrize("P", EDGE_P)
def test_float64_draw_agrees_on_well_cases(P):
    """Measured: 9e-18 (P = 1) to 6e-15 (P = 193)."""
    c = ldo.well(P)
    for w in (c.w, 1.7):
        ref = ldo.chol_draw_ld(c.Xt, w, c.pps, c.z, c.g)
        e = _rel(chol_draw(c.Xt, w, c.pps, c.z, c.g), ref)
        print("well P=%d: float64 vs long double %.2e" % (P, e))
        assert e <= 1e-13


def _woodbury_float64_error(name):
    Xt, obs_prec, pps, y = case(name)
    n, P = Xt.shape
    rng = np.random.default_rng(5)
    delta, xi = rng.standard_normal(n), rng.standard_normal(P)
    ref = ldo.woodbury_draw_ld(Xt, obs_prec, pps, y, delta, xi)
    e = _rel(woodbury_draw(Xt, obs_prec, pps, y, delta, xi), ref)
    print("%s: float64 vs long double %.2e" % (name, e))
    return e


@pytest.mark.parametrize("name", CASES)
def test_float64_woodbury_draw_agrees(name):
    """The bound is 1e-12, not the 'cholesky' draw's 1e-13:
    tests/test_woodbury_oracle.py measures this restatement at up to 9e-13
    from the explicit inverse, and against long double it is off by 4.2e-14
    to 3.1e-13 on the six cases."""
    assert _woodbury_float64_error(name) <= 1e-12


@pytest.mark.parametrize("name", WB_EDGE)
def test_float64_woodbury_draw_agrees_at_block_edges(name):
    """The shapes of tests/test_hip_direct_edges.py.  Measured: 1.5e-14 to
    2.3e-12 (n = 129 and the q = 1 cases are the worst: M's condition grows
    with n and with the prior scales' spread).  The device is held to 1e-10
    against long double there; this only keeps the float64 restatement a
    factor of ten inside that, as tests/test_hip_woodbury.py argues for its
    own use of it."""
    assert _woodbury_float64_error(name) <= 1e-11


@pytest.mark.parametrize("kind", ['collinear', 'rankdef'])
def test_float64_figures_of_the_ill_conditioned_cases(kind):
    """E64 (forward) and eta64 (backward error of the mean part) of the
    float64 restatement against long double.  Measured:
      collinear  cond(A) 3.8e11  E64 1.7e-05  eta64 5.4e-17
      rankdef    cond(A) 3.3e09  E64 5.7e-08  eta64 2.9e-17
    The forward error is cond * u, as it must be, and four to five decades
    above the 1e-10 the suite holds well-conditioned draws to; the backward
    error is a fraction of u.  The assertions only keep the cases what they
    are meant to be (ill-conditioned, and solved backward stably by LAPACK)."""
    c = getattr(ldo, kind)()
    A, _ = ldo.precond_ld(c.Xt, c.w, c.pps)
    cond = ldo.cond_2(A)
    E64, eta64, _ = ldo.float64_figures(kind)
    print("%s: cond(A) %.2e  E64 %.2e  eta64 %.2e" % (kind, cond, E64, eta64))
    assert cond >= 1e9
    assert 1e-10 < E64 < 1e-3
    assert eta64 <= c.Xt.shape[1] * 2. ** -53


def test_float64_figures_of_the_scales_case():
    """kappa of the per-coefficient check.  Measured: cond(A) 28, |coef| from
    1.5e-06 to 1.2e+05, max-norm error 1.7e-16, worst per-coefficient relative
    error rel64 = 3.1e-13.  FACTOR * rel64 = 1.0e-11 is below 1e-10, so
    kappa = 1: the 1e-10 figure holds coefficient by coefficient."""
    c = ldo.scales()
    A, _ = ldo.precond_ld(c.Xt, c.w, c.pps)
    ref = np.abs(ldo.chol_ref('scales'))
    E64, eta64, rel64 = ldo.float64_figures('scales')
    print("scales: cond(A) %.1f  |coef| %.1e .. %.1e  E64 %.2e  rel64 %.2e  "
          "kappa %.3g" % (ldo.cond_2(A), ref.min(), ref.max(), E64, rel64,
                          ldo.kappa(rel64)))
    assert ldo.cond_2(A) <= 100
    assert ref.max() / ref.min() >= 1e8
    assert rel64 >= 100 * E64        # what the max-norm check does not see
    assert ldo.kappa(rel64) <= 10


@pytest.mark.parametrize("j0", ldo.INDEFINITE_J0 + ((64, 127),))
def test_indefinite_cases_fail_where_they_are_built_to(j0):
    """first_bad == j0, by margins that no rounding crosses: every earlier
    pivot >= 0.1 (measured: >= 0.22), the bad one <= -1 (measured: -417 to
    -753), NaN for j0 = 0.  LAPACK names the same leading minor; for the NaN
    pivot its test `ajj <= 0` is false with this BLAS and the factorisation
    returns NaNs unreported, so there SciPy's finiteness check is what
    refuses the matrix."""
    first = j0 if isinstance(j0, int) else min(j0)
    c = ldo.indefinite(129, j0)
    A, s = ldo.precond_ld(c.Xt, c.w, c.pps)
    L, bad, piv = ldo.chol_ld(A)
    print("indefinite %s: first_bad %s pivot %.4g, earlier pivots >= %.3g"
          % (j0, bad, piv[-1], min(piv[:-1], default=np.nan)))
    assert bad == first and len(piv) == first + 1
    A64 = np.asarray(A, dtype=np.float64)
    if first == 0:
        assert np.isnan(piv[0]) and np.isnan(s[0])
        with pytest.raises((ValueError, np.linalg.LinAlgError)):
            scipy.linalg.cholesky(A64)
    else:
        assert min(piv[:-1]) >= .1 and piv[-1] <= -1
        assert np.all(s > 0) and np.all(np.isfinite(s))
        with pytest.raises(np.linalg.LinAlgError,
                           match=r"^%d-th leading minor" % (first + 1)):
            scipy.linalg.cholesky(A64, check_finite=False)
    # the same design with weight 0 on the appended rows is positive definite
    Av, _ = ldo.precond_ld(c.Xt, c.w_valid, c.pps)
    assert ldo.chol_ld(Av)[1] is None and ldo.cond_2(Av) < 1e4


def _parent_case(name, seed=0):
    """woodbury_oracle.case as it was before it took explicit shapes."""
    shapes = {
        'wide_q1_logit': (40, 130, 1, False), 'wide_q0_logit': (40, 130, 0, False),
        'wide_q3_linear': (70, 200, 3, True), 'tall_q1_logit': (150, 60, 1, False),
        'tall_q3_linear': (150, 60, 3, True), 'wide_q0_linear': (33, 97, 0, True),
    }
    n, P, q, linear = shapes[name]
    rng = np.random.default_rng(1000 + seed + len(name))
    X = rng.normal(size=(n, P - 1))
    X[:, ::3] = (rng.random((n, len(range(0, P - 1, 3)))) < .3)
    X = X - X.mean(axis=0)
    Xt = np.hstack((np.ones((n, 1)), X))
    sd = .5 * np.exp(rng.normal(0., 1.5, P))
    pps = 1 / sd
    pps[:q] = 0.
    pps[q] = 1 / 2.
    if linear:
        obs_prec = 1.7
        y = Xt[:, 1:6] @ rng.normal(size=5) + rng.normal(size=n) / np.sqrt(1.7)
    else:
        obs_prec = rng.gamma(2., .15, n) + 1e-3
        y = (rng.integers(0, 2, n) - .5) / obs_prec
    return Xt, obs_prec, pps, y


@pytest.mark.parametrize("name", CASES)
def test_named_woodbury_cases_keep_their_arrays(name):
    for seed in (0, 3):
        for a, b in zip(case(name, seed), _parent_case(name, seed)):
            assert np.array_equal(a, b)


def test_explicit_woodbury_shapes():
    Xt, obs_prec, pps, y = case((65, 135, 3, False))
    assert Xt.shape == (65, 135) and obs_prec.shape == (65,)
    assert np.all(pps[:3] == 0) and pps[3] == .5 and np.all(pps[3:] > 0)
    assert np.all(Xt[:, 0] == 1)
    assert np.abs(Xt[:, 1:].mean(axis=0)).max() < 1e-15
    assert np.var(Xt[:, 1:], axis=0).min() > 65 * 2. ** -52
    assert isinstance(case((64, 134, 1, True))[1], float)
    assert not np.array_equal(case((64, 134, 0, False))[0],
                              case((64, 134, 1, False))[0])
