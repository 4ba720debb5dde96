"""CPU: the tests' restatement of the 'cholesky' draw (tests/cholesky_oracle.py)
against the committed fixtures and, where the reference is importable, against
generate_gaussian_with_weight itself."""
import os

import numpy as np
import pytest

from cholesky_oracle import OracleCholeskyGibbs, chol_draw, fisher_info


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _design_matrix(X, centred=True):
    # intercept column, centred predictors (RegressionModel's default)
    if centred:
        X = X - X.mean(axis=0)
    return np.hstack((np.ones((X.shape[0], 1)), X))


@pytest.mark.parametrize("model", ['linear', 'logit'])
def test_restated_draw_matches_recorded_reference(golden_dir, model):
    g = _load(golden_dir, 'chain_%s_dense_cholesky.npz' % model)
    Xt = _design_matrix(g['X'])
    for k in range(g['draw_coef'].shape[0]):
        coef = chol_draw(Xt, g['draw_obs_prec'][k],
                         g['draw_prior_prec_sqrt'][k], g['draw_z'][k],
                         g['draw_normals'][k])
        ref = g['draw_coef'][k]
        assert np.abs(coef - ref).max() <= 1e-10 * max(1., np.abs(ref).max())


def test_restated_fisher_info_matches_reference_fixture(golden_dir):
    g = _load(golden_dir, 'fisher_info_dense_100x50.npz')
    for tag in ('uncentred', 'centred'):
        Xt = _design_matrix(g['X'], centred=tag == 'centred')
        assert np.allclose(fisher_info(Xt, g['weight']), g['full_' + tag],
                           rtol=1e-12, atol=1e-10)
        assert np.allclose(fisher_info(Xt, g['weight'], diag_only=True),
                           g['diag_' + tag], rtol=1e-12, atol=1e-10)


def test_restated_chain_reproduces_reference_fixture(golden_dir):
    g = _load(golden_dir, 'chain_logit_dense_cholesky.npz')
    last = np.load(os.path.join(golden_dir,
                                'reference_logit_cholesky_last_sample.npy'))
    ora = OracleCholeskyGibbs((g['n_success'], g['n_trial']), g['X'], 'logit',
                              bridge_exponent=.25, sd_for_intercept=2.,
                              regularizing_slab_size=1.)
    out = ora.gibbs(10, seed=0, init={'global_scale': .1,
                                      'local_scale': np.ones(50)})
    assert np.allclose(out['coef'][:, -1], last, rtol=1e-3, atol=1e-5)
    assert np.allclose(out['coef'], g['coef_samples'], rtol=1e-6, atol=1e-8)


@pytest.mark.needs_reference
def test_restated_draw_equals_live_reference(golden_dir):
    import sys
    sys.path.insert(0, golden_dir)
    import ref_import
    ref_import.import_reference()
    from bayesbridge.design_matrix import DenseDesignMatrix
    from bayesbridge.reg_coef_sampler.direct_gaussian_sampler import \
        generate_gaussian_with_weight
    g = _load(golden_dir, 'chain_logit_dense_cholesky.npz')
    design = DenseDesignMatrix(g['X'].copy(), copy_array=True,
                               center_predictor=True, add_intercept=True)
    Xt = _design_matrix(g['X'])
    state = np.random.get_state()
    try:
        for k in range(g['draw_coef'].shape[0]):
            args = (g['draw_obs_prec'][k], g['draw_prior_prec_sqrt'][k],
                    g['draw_z'][k])
            np.random.seed(100 + k)
            normals = np.random.randn(Xt.shape[1])
            np.random.seed(100 + k)
            ref = generate_gaussian_with_weight(design, *args)
            mine = chol_draw(Xt, *args, normals)
            assert np.abs(mine - ref).max() <= 1e-12 * max(1., np.abs(ref).max())
    finally:
        np.random.set_state(state)
