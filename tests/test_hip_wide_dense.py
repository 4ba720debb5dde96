"""GPU: dense designs wider than the 19 200 columns the single-pass X~ v kernel
stages in LDS (csrc/dense.hip, dense_dot_wide_kernel): dot, Tdot, gram_matvec
and one CG draw on a 300 x 25 000 design against the oracle's dense operator,
and a design of exactly the old bound's width against the bits the parent
commit's build produced (tests/golden/dense_19200_parent_bits.npz, written by
tests/golden/make_dense_19200_bits.py)."""
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=['float64', 'float32'])
def wide(request):
    from bayesbridge_amd import HipDenseDesignMatrix
    rng = np.random.default_rng(25000)
    n, p = 300, 25000
    X = rng.normal(size=(n, p)) + rng.normal(size=p)
    if request.param == 'float32':
        X = X.astype(np.float32).astype(np.float64)
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                               storage_dtype=request.param)
    ora = oracle.OracleDenseDesign(X, center_predictor=True,
                                   add_intercept=True)
    if request.param == 'float32':      # the operator of the stored values
        ora.X = ora.X.astype(np.float32).astype(np.float64)
    return hip, ora, rng


def test_wide_products_match_oracle(wide):
    hip, ora, rng = wide
    n, P = hip.shape
    assert P == 25001
    for _ in range(2):
        v, w = rng.normal(size=P), rng.normal(size=n)
        omega = rng.gamma(2., .15, n)
        t, t_ref = hip.dot(v), ora.dot(v)
        assert np.abs(t - t_ref).max() <= 1e-12 * np.abs(t_ref).max()
        assert np.array_equal(t, hip.dot(v))                 # same bits
        g, g_ref = hip.Tdot(w), ora.Tdot(w)
        assert np.abs(g - g_ref).max() <= 1e-12 * np.abs(g_ref).max()
        assert np.array_equal(g, hip.Tdot(w))
        a, a_ref = hip.gram_matvec(omega, v), ora.Tdot(omega * ora.dot(v))
        assert np.abs(a - a_ref).max() <= 1e-12 * np.abs(a_ref).max()
        assert np.array_equal(a, hip.gram_matvec(omega, v))


def test_wide_cg_draw_matches_oracle(wide):
    from bayesbridge_amd import HipCGSampler
    from helpers import cg_inputs
    hip, ora, _ = wide
    n, P = hip.shape
    inp = cg_inputs(n, P, seed=4)
    atol = 10e-6 * np.sqrt(P)
    np.random.seed(7)
    state = np.random.get_state()
    eta1, eta2 = np.random.randn(n), np.random.randn(P)
    np.random.set_state(state)
    coef, info = HipCGSampler(1).sample(
        hip, inp['obs_prec'], inp['prior_prec_sqrt'], inp['z'],
        coef_cg_init=inp['coef_cg_init'],
        coef_scaled_sd=inp['coef_scaled_sd'], maxiter=2000, atol=atol)
    ref, info_o = oracle.cg_sample(
        ora, inp['obs_prec'], inp['prior_prec_sqrt'], inp['z'],
        inp['coef_cg_init'], inp['coef_scaled_sd'], 1, eta1, eta2, 2000, atol)
    assert info['converged'] and abs(info['n_iter'] - info_o['n_iter']) <= 1
    assert np.abs(coef - ref).max() <= 1e-5 * max(1., np.abs(ref).max())


@pytest.mark.parametrize("storage", ['float32', 'float64'])
def test_bound_width_gives_the_parent_builds_bits(golden_dir, storage):
    """P = 19 200 exactly: the single-pass kernels still run, bit for bit."""
    from make_dense_19200_bits import compute
    g = np.load(os.path.join(golden_dir, 'dense_19200_parent_bits.npz'))
    out = compute(storage)
    for key, val in out.items():
        assert np.array_equal(val, g['%s_%s' % (storage, key)]), key
