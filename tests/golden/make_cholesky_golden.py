"""Generates the fixtures of the 'cholesky' coefficient sampler by importing
the upstream reference (build container only; see ref_import.py).  Data only:
inputs and the reference's outputs.  Re-run with

    python tests/golden/make_cholesky_golden.py

Files written:
  chain_{linear,logit}_dense_cholesky.npz
      the dense combos of tests/regression_tests/test_gibb.py:11-17 with
      coef_sampler_type='cholesky' (seed 0, 10 iterations, params 'all'):
      data, all samples, and for every call of generate_gaussian_with_weight
      its inputs, the np.random.randn(P) it drew and its output.
  fisher_info_dense_100x50.npz
      DenseDesignMatrix.compute_fisher_info (dense_matrix.py:54-58) of a
      centred and an uncentred design with intercept, full and diag_only.
(reference_logit_cholesky_last_sample.npy is a copy of the reference's own
saved_outputs/logit_cholesky_samples.npy.)
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

warnings.simplefilter('ignore')
bb, refsim = ref_import.import_reference()
from bayesbridge import BayesBridge, RegressionModel, RegressionCoefPrior  # noqa
from bayesbridge.design_matrix import DenseDesignMatrix  # noqa: E402
from bayesbridge.model import LinearModel, LogisticModel  # noqa: E402
import bayesbridge.reg_coef_sampler.reg_coef_sampler as rcs  # noqa: E402


class Recorder:
    """Wraps generate_gaussian_with_weight to keep what went in and out."""

    def __init__(self):
        self.records = []
        self.orig = rcs.generate_gaussian_with_weight

    def __enter__(self):
        rec, orig = self.records, self.orig

        def wrapped(design, obs_prec, prior_prec_sqrt, z, rand_gen=None):
            before = np.random.get_state()
            coef = orig(design, obs_prec, prior_prec_sqrt, z, rand_gen)
            after = np.random.get_state()
            np.random.set_state(before)
            g = np.random.randn(design.shape[1])   # direct_gaussian_sampler.py:30
            np.random.set_state(after)
            rec.append(dict(obs_prec=np.array(obs_prec, dtype=float),
                            prior_prec_sqrt=np.array(prior_prec_sqrt),
                            z=np.array(z), normals=g, coef=np.array(coef)))
            return coef

        rcs.generate_gaussian_with_weight = wrapped
        return self

    def __exit__(self, *exc):
        rcs.generate_gaussian_with_weight = self.orig

    def stacked(self):
        return {'draw_' + k: np.stack([r[k] for r in self.records])
                for k in self.records[0]}


def regression_test_data(model):
    # tests/regression_tests/test_gibb.py:62-90 ('dense')
    np.random.seed(1)
    n, p = 100, 50
    beta_true = np.zeros(p)
    beta_true[:4] = 1
    beta_true[4:15] = 2 ** - np.linspace(0.0, 5, 11)
    X = np.random.randn(n, p)
    if model == 'linear':
        return LinearModel.simulate_outcome(X, beta_true, 2), X
    n_trial = np.ones(n, dtype=np.int32)
    return (LogisticModel.simulate_outcome(n_trial, X, beta_true), n_trial), X


def golden_chain(model):
    outcome, X = regression_test_data(model)
    prior = RegressionCoefPrior(sd_for_intercept=2., regularizing_slab_size=1.,
                                bridge_exponent=.25)
    bridge = BayesBridge(RegressionModel(outcome, X.copy(), model), prior)
    init = {'global_scale': 0.1, 'local_scale': np.ones(X.shape[1])}
    with Recorder() as rec:
        samples, info = bridge.gibbs(10, 0, init=init, thin=1,
                                     coef_sampler_type='cholesky', seed=0,
                                     params_to_save='all')
    out = rec.stacked()
    out.update(X=X, coef_samples=samples['coef'],
               global_scale_samples=samples['global_scale'],
               local_scale_samples=samples['local_scale'],
               logp_samples=samples['logp'])
    if model == 'linear':
        out['y'] = outcome
        out['obs_prec_samples'] = samples['obs_prec']
    else:
        out['n_success'], out['n_trial'] = outcome
    return out


def fisher_cases():
    rng = np.random.default_rng(7)
    X = rng.normal(size=(100, 50)) + rng.normal(size=50)
    w = rng.gamma(2., .3, 100)
    out = {'X': X, 'weight': w}
    for centred in (False, True):
        d = DenseDesignMatrix(X.copy(), center_predictor=centred,
                              add_intercept=True, copy_array=True)
        tag = 'centred' if centred else 'uncentred'
        out['full_' + tag] = d.compute_fisher_info(w)
        out['diag_' + tag] = d.compute_fisher_info(w, diag_only=True)
    return out


if __name__ == '__main__':
    for model in ('linear', 'logit'):
        np.savez(os.path.join(HERE, 'chain_%s_dense_cholesky.npz' % model),
                 **golden_chain(model))
    np.savez(os.path.join(HERE, 'fisher_info_dense_100x50.npz'),
             **fisher_cases())
    print('written')
