"""GPU: the 'cholesky' coefficient sampler on dense designs (csrc/cholesky.hip):
the matrix-core Gram against NumPy, the draw against the reference's recorded
inputs and outputs, and exact-seed chains against the reference's fixtures."""
import os
import re
import warnings

import numpy as np
import pytest

from cholesky_oracle import chol_draw

pytestmark = pytest.mark.gpu


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _explicit(X, centred, intercept):
    X = np.asarray(X, dtype=np.float64)
    if centred:
        X = X - X.mean(axis=0)
    return np.hstack((np.ones((X.shape[0], 1)), X)) if intercept else X


@pytest.mark.parametrize("P", [1, 15, 17, 50, 257])
@pytest.mark.parametrize("storage", ['float64', 'float32'])
def test_fisher_info_matches_numpy(P, storage):
    from bayesbridge_amd import HipDenseDesignMatrix
    rng = np.random.default_rng(P)
    n = 6000                            # several row chunks of the Gram
    for centred, intercept in ((True, True), (False, True), (False, False)):
        p = P - intercept
        if p < 1:
            continue
        X = rng.normal(size=(n, p)) + rng.normal(size=p)
        w = rng.gamma(2., .3, n)
        d = HipDenseDesignMatrix(X, center_predictor=centred,
                                 add_intercept=intercept,
                                 storage_dtype=storage)
        Xt = _explicit(X, centred, intercept)
        if storage == 'float32':        # the Gram of the stored, rounded X~
            Xt = Xt.astype(np.float32).astype(np.float64)
        ref = Xt.T @ (w[:, None] * Xt)
        F = d.compute_fisher_info(w)
        assert F.shape == (P, P)
        assert np.abs(F - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(F, F.T)
        assert np.array_equal(F, d.compute_fisher_info(w))      # bit-equal
        diag = d.compute_fisher_info(w, diag_only=True)
        assert np.abs(diag - np.diag(ref)).max() <= 1e-12 * np.abs(ref).max()
        assert np.array_equal(diag, d.compute_fisher_info(w, diag_only=True))
        ones = d.compute_fisher_info(None)
        r1 = Xt.T @ Xt
        assert np.abs(ones - r1).max() <= 1e-12 * np.abs(r1).max()


def test_fisher_info_reference_fixture(golden_dir):
    from bayesbridge_amd import HipDenseDesignMatrix
    g = _load(golden_dir, 'fisher_info_dense_100x50.npz')
    for tag in ('uncentred', 'centred'):
        d = HipDenseDesignMatrix(g['X'], center_predictor=tag == 'centred',
                                 add_intercept=True)
        ref = g['full_' + tag]
        assert np.abs(d.compute_fisher_info(g['weight']) - ref).max() \
            <= 1e-12 * np.abs(ref).max()
        rd = g['diag_' + tag]
        assert np.abs(d.compute_fisher_info(g['weight'], diag_only=True)
                      - rd).max() <= 1e-12 * np.abs(rd).max()


@pytest.mark.parametrize("model", ['linear', 'logit'])
def test_chol_sample_reproduces_reference_draws(golden_dir, model):
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.reg_coef_sampler import chol_sample
    g = _load(golden_dir, 'chain_%s_dense_cholesky.npz' % model)
    d = HipDenseDesignMatrix(g['X'], center_predictor=True, add_intercept=True)
    for k in range(g['draw_coef'].shape[0]):
        # linear draws have equal weights: the cached-Gram scalar path
        coef = chol_sample(d, g['draw_obs_prec'][k],
                           g['draw_prior_prec_sqrt'][k], g['draw_z'][k],
                           normals=g['draw_normals'][k])
        ref = g['draw_coef'][k]
        assert np.abs(coef - ref).max() <= 1e-10 * max(1., np.abs(ref).max())


def test_chol_sample_larger_problem_matches_oracle():
    """P = 300 (five 64-blocks: panel, trailing update and the multi-block
    solves all run), n = 3000."""
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.reg_coef_sampler import chol_sample
    rng = np.random.default_rng(5)
    n, p = 3000, 299
    X = rng.normal(size=(n, p)) + .3 * rng.normal(size=(n, 1))
    d = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    Xt = _explicit(X, True, True)
    w = rng.gamma(2., .2, n)
    pps = np.exp(rng.normal(0., 1., p + 1))
    pps[0] = 0.
    z = rng.normal(size=p + 1)
    g = rng.normal(size=p + 1)
    ref = chol_draw(Xt, w, pps, z, g)
    coef = chol_sample(d, w, pps, z, normals=g)
    assert np.abs(coef - ref).max() <= 1e-10 * max(1., np.abs(ref).max())
    assert np.array_equal(coef, chol_sample(d, w, pps, z, normals=g))


def test_chol_sample_indefinite_raises_and_design_stays_usable(golden_dir):
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.reg_coef_sampler import chol_sample
    g = _load(golden_dir, 'chain_logit_dense_cholesky.npz')
    d = HipDenseDesignMatrix(g['X'], center_predictor=True, add_intercept=True)
    args = (g['draw_prior_prec_sqrt'][0], g['draw_z'][0])
    w = g['draw_obs_prec'][0].copy()
    w[::2] *= -50.
    with pytest.raises(np.linalg.LinAlgError, match="pivot") as info:
        chol_sample(d, w, *args, normals=g['draw_normals'][0])
    m = re.search(r"pivot (\d+)", str(info.value))
    assert m, str(info.value)
    assert 0 <= int(m.group(1)) < d.shape[1]
    coef = chol_sample(d, g['draw_obs_prec'][0], *args,
                       normals=g['draw_normals'][0])
    ref = g['draw_coef'][0]
    assert np.abs(coef - ref).max() <= 1e-10 * max(1., np.abs(ref).max())


def test_cholesky_refused_on_sparse_design(golden_dir):
    import scipy.sparse as sparse
    from bayesbridge_amd import HipSparseDesignMatrix, _lib
    from bayesbridge_amd.reg_coef_sampler import chol_sample
    g = _load(golden_dir, 'chain_logit_dense_cholesky.npz')
    d = HipSparseDesignMatrix(sparse.csr_matrix(g['X']))
    with pytest.raises(NotImplementedError):
        d.compute_fisher_info(np.ones(100))
    with pytest.raises(ValueError):
        chol_sample(d, np.ones(100), np.ones(51), np.ones(51))
    out = np.empty(51)
    assert d._lib.bbx_design_fisher_info(d._h, None, 1, out.ctypes.data) \
        == -1
    assert 'dense' in _lib.last_error()


def _bridge(g, model):
    from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,
                                 RegressionCoefPrior, RegressionModel)
    design = HipDenseDesignMatrix(g['X'], center_predictor=True,
                                  add_intercept=True)
    outcome = g['y'] if model == 'linear' else (g['n_success'], g['n_trial'])
    prior = RegressionCoefPrior(sd_for_intercept=2., regularizing_slab_size=1.,
                                bridge_exponent=.25)
    return BayesBridge(RegressionModel(outcome, design, model), prior)


_INIT = {'global_scale': 0.1, 'local_scale': np.ones(50)}


@pytest.mark.parametrize("model", ['linear', 'logit'])
def test_exact_seed_chain_reproduces_reference(golden_dir, model):
    g = _load(golden_dir, 'chain_%s_dense_cholesky.npz' % model)
    bridge = _bridge(g, model)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        samples, info = bridge.gibbs(
            10, init=dict(_INIT), seed=0, coef_sampler_type='cholesky',
            options={'rng': 'reference'}, params_to_save='all')
    assert info['options']['coef_sampler_type'] == 'cholesky'
    assert 'n_cg_iter' not in info['_reg_coef_sampling_info']
    assert np.allclose(samples['coef'], g['coef_samples'], rtol=1e-6,
                       atol=1e-8)
    assert np.allclose(samples['global_scale'], g['global_scale_samples'],
                       rtol=1e-6)
    assert np.allclose(samples['logp'], g['logp_samples'], rtol=1e-6)
    if model == 'logit':
        last = np.load(os.path.join(
            golden_dir, 'reference_logit_cholesky_last_sample.npy'))
        assert np.allclose(samples['coef'][:, -1], last, rtol=1e-3,
                           atol=1e-5)


def test_exact_seed_chain_restart_in_middle(golden_dir):
    """test_gibb.py:15: ('logit', 'cholesky', 'dense', restart_in_middle)."""
    g = _load(golden_dir, 'chain_logit_dense_cholesky.npz')
    last = np.load(os.path.join(golden_dir,
                                'reference_logit_cholesky_last_sample.npy'))
    bridge = _bridge(g, 'logit')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        s1, info1 = bridge.gibbs(
            5, init=dict(_INIT), seed=0, coef_sampler_type='cholesky',
            options={'rng': 'reference'}, params_to_save='all')
        s2, info2 = _bridge(g, 'logit').gibbs_resume(info1, 5, merge=True,
                                                     prev_samples=s1)
    assert info2['options']['coef_sampler_type'] == 'cholesky'
    assert s2['coef'].shape == (51, 10)
    assert np.allclose(s2['coef'][:, -1], last, rtol=1e-3, atol=1e-5)
    assert np.allclose(s2['coef'], g['coef_samples'], rtol=1e-6, atol=1e-8)


def test_cholesky_refused_where_unsupported(golden_dir):
    g = _load(golden_dir, 'chain_logit_dense_cholesky.npz')
    bridge = _bridge(g, 'logit')
    opts = {'coef_sampler_type': 'cholesky'}
    with pytest.raises(ValueError, match='cg'):
        bridge.gibbs_batch([1, 2], 2, options=opts)
    with pytest.raises(ValueError, match='cg'):
        bridge.gibbs_multichain(2, 2, options=opts)


_BATCHED_GRAM = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from bayesbridge_amd import HipDenseDesignMatrix
rng = np.random.default_rng(3)
n, p = 6000, 256
X = rng.normal(size=(n, p)) + rng.normal(size=p)
w = rng.gamma(2., .3, n)
d = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                         storage_dtype='float32')
Xt = np.hstack((np.ones((n, 1)), X - X.mean(axis=0)))
Xt = Xt.astype(np.float32).astype(np.float64)
ref = Xt.T @ (w[:, None] * Xt)
F = d.compute_fisher_info(w)
assert np.abs(F - ref).max() <= 1e-12 * np.abs(ref).max()
assert np.array_equal(F, F.T) and np.array_equal(F, d.compute_fisher_info(w))
print("ok")
'''


def test_fisher_info_batched_tiles():
    """With the partial slab bounded below one tile's partials
    (BBX_GRAM_SLAB_BYTES, in a fresh process) the Gram runs one tile per
    batch: 15 batches at P = 257 -- the path of designs wider than ~8 000
    columns under the default 256 MB bound."""
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, BBX_GRAM_SLAB_BYTES='65536')
    out = subprocess.run(
        [sys.executable, '-c', _BATCHED_GRAM,
         os.path.join(ROOT, 'bayes-bridge_amd')],
        env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr[-2000:]


def test_release_sampler_memory(golden_dir):
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.reg_coef_sampler import chol_sample
    g = _load(golden_dir, 'chain_linear_dense_cholesky.npz')
    d = HipDenseDesignMatrix(g['X'], center_predictor=True, add_intercept=True)
    args = (g['draw_obs_prec'][0], g['draw_prior_prec_sqrt'][0],
            g['draw_z'][0])
    first = chol_sample(d, *args, normals=g['draw_normals'][0])
    d.release_sampler_memory()
    again = chol_sample(d, *args, normals=g['draw_normals'][0])
    assert np.array_equal(first, again)
