"""GPU: the two direct samplers (csrc/cholesky.hip, csrc/woodbury.hip) where
their shared blocked kernels can go wrong unnoticed: matrices of exactly one or
two 64-blocks (no padding at all), of one column more (one real column next to
63 of identity padding), designs of fewer rows than a wave's group of four,
the cached-Gram scalar path, ill-conditioned and badly scaled problems, and
the index of a failed pivot.  Everything is compared with the long-double
oracle of tests/direct_ld_oracle.py, whose cases and float64 figures
tests/test_direct_ld_oracle.py checks on the CPU.

Tolerances: the Gram at the suite's 1e-12 max|ref|, a well-conditioned draw at
the suite's 1e-10 max(1, |ref|).  Where the problem is ill-conditioned the
bound is FACTOR = 32 times what the float64 restatement (NumPy, LAPACK) is
itself off by against long double on the same case, forward (E64) and backward
(eta64), recomputed here; LABNOTES, "Direct samplers at 64-block edges", gives
the figures and the reasoning."""
import re

import numpy as np
import pytest

import direct_ld_oracle as ldo
from cholesky_oracle import explicit
from woodbury_oracle import case as wb_case

pytestmark = pytest.mark.gpu

TOL = 1e-10
EDGE_P = (1, 2, 63, 64, 65, 127, 128, 129, 193)


def _design(X, centred=False, intercept=True, storage='float64'):
    """The HIP design of the predictors X.  Constant columns (every column
    when n = 1; the ones of a P = 1 problem) would be dropped by the
    constructor, so such an X is adopted from device memory instead."""
    from bayesbridge_amd import HipDenseDesignMatrix
    X = np.ascontiguousarray(X, dtype=np.float64)
    if not np.any(np.var(X, axis=0) < X.shape[0] * 2. ** -52):
        return HipDenseDesignMatrix(X, center_predictor=centred,
                                    add_intercept=intercept,
                                    storage_dtype=storage)
    import torch
    t = torch.from_numpy(X).cuda()
    off = torch.from_numpy(np.mean(X, axis=0)).cuda() if centred else None
    d = HipDenseDesignMatrix.from_device_array(
        X.shape[0], X.shape[1], t.data_ptr(),
        off.data_ptr() if centred else None, add_intercept=intercept,
        in_dtype='float64', storage_dtype=storage)
    torch.cuda.synchronize()
    return d


def _stored(X, centred, intercept, storage):
    """X~ as the design stores it."""
    X = np.asarray(X, dtype=np.float64)
    if centred:
        X = X - X.mean(axis=0)
    if intercept:
        X = np.hstack((np.ones((X.shape[0], 1)), X))
    if storage == 'float32':
        X = X.astype(np.float32).astype(np.float64)
    return X


def _case_design(c):
    """The float64 design whose X~ is c.Xt bit for bit."""
    if c.intercept and c.Xt.shape[1] > 1:
        return _design(c.Xt[:, 1:], False, True)
    return _design(c.Xt, False, False)


def _close(out, ref, what, tol=TOL):
    err = float(np.abs(out - ref).max())
    print("%s: max|dev - ld| = %.2e (|ref| %.2e)"
          % (what, err, float(np.abs(ref).max())))
    return err <= tol * max(1., float(np.abs(ref).max()))


def _sample(d, c, w=None, g=None):
    from bayesbridge_amd.reg_coef_sampler import chol_sample
    return chol_sample(d, c.w if w is None else w, c.pps, c.z,
                       normals=c.g if g is None else g)


# ---- a. the Gram -------------------------------------------------------------
GRAM_N = (1, 2, 3, 5, 67, 1027)     # 1027: two chunks of 514 rows


def _gram_problem(P, n, centred):
    rng = np.random.default_rng([P, n, int(centred)])
    p = P - centred                  # centred comes with the intercept
    X = rng.normal(size=(n, p)) + rng.normal(size=p)
    return X, rng.gamma(2., .3, n)


@pytest.mark.parametrize("storage", ['float64', 'float32'])
def test_stored_matrix_is_what_the_gram_tests_assume(storage):
    for n in (1, 5):
        for centred in (True, False):
            X, _ = _gram_problem(65, n, centred)
            d = _design(X, centred, centred, storage)
            assert d.shape == (n, 65)
            assert np.array_equal(explicit(d),
                                  _stored(X, centred, centred, storage))


@pytest.mark.parametrize("storage", ['float64', 'float32'])
@pytest.mark.parametrize("P", [63, 64, 65, 128, 129])
def test_gram_at_tile_edges(P, storage, monkeypatch):
    for n in GRAM_N:
        for centred in (True, False):
            X, w = _gram_problem(P, n, centred)
            d = _design(X, centred, centred, storage)
            ref = ldo.gram_ld(_stored(X, centred, centred, storage), w)
            bound = 1e-12 * float(np.abs(ref).max())
            F = d.compute_fisher_info(w)
            assert F.shape == (P, P)
            err = float(np.abs(F - ref).max())
            assert err <= bound, (n, centred, err, bound)
            assert np.array_equal(F, F.T)
            assert np.array_equal(F, d.compute_fisher_info(w))
            diag = d.compute_fisher_info(w, diag_only=True)
            assert float(np.abs(diag - np.diag(ref)).max()) <= bound
            assert np.array_equal(
                diag, d.compute_fisher_info(w, diag_only=True))
            if P in (65, 129) and n >= 67:
                # tiles in batches: a slab bound of two tiles' partials
                monkeypatch.setenv("BBX_GRAM_SLAB_BYTES", str(2 * 64 * 64 * 8))
                d.release_sampler_memory()
                assert np.array_equal(F, d.compute_fisher_info(w))
                monkeypatch.delenv("BBX_GRAM_SLAB_BYTES")


# ---- b. the 'cholesky' draw at block edges -----------------------------------
@pytest.mark.parametrize("P", EDGE_P)
def test_chol_sample_weighted_at_block_edges(P):
    c = ldo.well(P)
    d = _case_design(c)
    out = _sample(d, c)
    assert _close(out, ldo.chol_ref('well', P), "well P=%d weighted" % P)
    assert np.array_equal(out, _sample(d, c))


@pytest.mark.parametrize("P", EDGE_P)
def test_chol_sample_scalar_at_block_edges(P):
    """obs_prec one number: F = alpha (X~^T X~) from the Gram cached on the
    design; the second alpha reuses the cache."""
    c = ldo.well(P)
    d = _case_design(c)
    for alpha in (1.7, .3):
        out = _sample(d, c, alpha)
        assert _close(out, ldo.chol_ref('well', P, alpha=alpha),
                      "well P=%d alpha=%g" % (P, alpha))
        assert np.array_equal(out, _sample(d, c, alpha))


def test_chol_sample_paths_share_a_handle():
    """The scalar path's cached Gram (chol_gram) and the weighted path's F and
    factor (chol_A) on one design, in both orders."""
    P = 65
    c = ldo.well(P)
    ref_w = ldo.chol_ref('well', P)
    ref_a = {a: ldo.chol_ref('well', P, alpha=a) for a in (1.7, .3)}
    d = _case_design(c)
    first = _sample(d, c, 1.7)
    assert _close(first, ref_a[1.7], "scalar, cold")
    assert _close(_sample(d, c, .3), ref_a[.3], "scalar, cached")
    weighted = _sample(d, c)
    assert _close(weighted, ref_w, "weighted after scalar")
    assert np.array_equal(first, _sample(d, c, 1.7))       # after weighted
    assert np.array_equal(weighted, _sample(d, c))
    # the other order on a fresh design
    d2 = _case_design(c)
    assert np.array_equal(weighted, _sample(d2, c))
    assert np.array_equal(first, _sample(d2, c, 1.7))
    assert _close(_sample(d2, c, .3), ref_a[.3], "scalar after weighted")


# ---- c. scales ---------------------------------------------------------------
def test_chol_sample_badly_scaled_per_coefficient():
    """Column scales and prior scales over many decades: every coefficient,
    not only the largest, is held to 1e-10 kappa of its own size (kappa from
    the float64 restatement's own per-coefficient error: direct_ld_oracle.kappa;
    1 on this case)."""
    c = ldo.scales()
    ref = ldo.chol_ref('scales')
    _, _, rel64 = ldo.float64_figures('scales')
    kappa = ldo.kappa(rel64)
    out = _sample(_case_design(c), c)
    rel = np.abs(out - ref) / np.maximum(1e-300, np.abs(ref))
    print("scales: worst per-coefficient error %.2e (float64 restatement "
          "%.2e, kappa %.3g)" % (float(rel.max()), rel64, kappa))
    assert float(rel.max()) <= TOL * kappa


# ---- d. ill-conditioned ------------------------------------------------------
@pytest.mark.parametrize("kind", ['collinear', 'rankdef'])
def test_chol_sample_ill_conditioned_forward(kind):
    c = getattr(ldo, kind)()
    ref = ldo.chol_ref(kind)
    E64, _, _ = ldo.float64_figures(kind)
    out = _sample(_case_design(c), c)
    err = float(np.abs(out - ref).max() / max(1., np.abs(ref).max()))
    print("%s: forward error %.2e = %.2f E64 (E64 %.2e)"
          % (kind, err, err / E64, E64))
    assert err <= ldo.FACTOR * E64


@pytest.mark.parametrize("kind", ['collinear', 'rankdef'])
def test_chol_sample_ill_conditioned_backward(kind):
    c = getattr(ldo, kind)()
    _, eta64, _ = ldo.float64_figures(kind)
    mean = _sample(_case_design(c), c, g=np.zeros_like(c.g))
    eta = float(ldo.mean_backward_error(c, mean))
    print("%s: backward error %.2e = %.2f eta64 (eta64 %.2e)"
          % (kind, eta, eta / eta64, eta64))
    assert eta <= ldo.FACTOR * eta64


# ---- e. the failed pivot's index ---------------------------------------------
def _reported_pivot(d, c):
    with pytest.raises(np.linalg.LinAlgError, match="pivot") as info:
        _sample(d, c)
    m = re.search(r"pivot (\d+) is not > 0", str(info.value))
    assert m, str(info.value)
    return int(m.group(1))


@pytest.mark.parametrize("j0", ldo.INDEFINITE_J0 + ((64, 127),))
def test_failed_pivot_is_named_exactly(j0):
    P = 129
    c = ldo.indefinite(P, j0)
    A, _ = ldo.precond_ld(c.Xt, c.w, c.pps)
    first_bad = ldo.chol_ld(A)[1]
    assert first_bad == (j0 if isinstance(j0, int) else min(j0))
    d = _case_design(c)
    assert _reported_pivot(d, c) == first_bad
    # the flag is reset per call and nothing is left poisoned: the same design
    # with weight 0 on the appended rows, then a fresh design of the same P
    valid = _sample(d, c, c.w_valid)
    assert _close(valid, ldo.chol_ref('indefinite', P, j0, valid=True),
                  "same design, valid weights")
    assert _reported_pivot(d, c) == first_bad
    cw = ldo.well(P)
    assert _close(_sample(_case_design(cw), cw), ldo.chol_ref('well', P),
                  "fresh design")
    assert np.array_equal(valid, _sample(d, c, c.w_valid))


# ---- f. the 'woodbury' draw at block edges of its n x n system ---------------
WB_SHAPES = [(n, n + 70, q, False) for n in (63, 64, 65, 128, 129)
             for q in (0, 1, 3)] + [(64, 134, 1, True), (129, 199, 3, True)]


@pytest.mark.parametrize("shape", WB_SHAPES,
                         ids=lambda s: "n%d_P%d_q%d_%s" % (
                             s[0], s[1], s[2], 'linear' if s[3] else 'logit'))
def test_woodbury_sample_at_block_edges(shape):
    from bayesbridge_amd.reg_coef_sampler import woodbury_sample
    Xt, obs_prec, pps, y = wb_case(shape)
    n, P = Xt.shape
    d = _design(Xt[:, 1:], False, True)
    rng = np.random.default_rng(5)
    delta, xi = rng.standard_normal(n), rng.standard_normal(P)
    ref = ldo.woodbury_draw_ld(Xt, obs_prec, pps, y, delta, xi)
    out = woodbury_sample(d, obs_prec, pps, y, delta, xi)
    assert _close(out, ref, "woodbury n=%d P=%d q=%d" % shape[:3])
    assert np.array_equal(out, woodbury_sample(d, obs_prec, pps, y, delta, xi))
