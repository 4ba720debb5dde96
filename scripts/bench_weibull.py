"""Weibull model on the device next to the Poisson handle on the same rows and
the plain Cox handle on the same outcome, in one process:

    python scripts/bench_weibull.py --shapes binary:1000000x50000 \\
        dense:100000x2000 [--steps 5 --warmup 2]

For each shape: simulated Weibull times (demo coefficients, shape 1.5, half
of the rows censored), then
  leapfrog_us            one step of a 64-step device trajectory (one host
                         wait) on the Weibull handle
  poisson_leapfrog_us    the same on a Poisson handle of the same rows (y = d,
                         exposure t): the row kernel's work without the one
                         multiply per row
  cox_leapfrog_us        the same on the plain Cox handle of the same outcome
                         (its own design: the rows sorted, no intercept)
  products_us            X~ v + X~^T w on device pointers, same stream
  ratio, ratio_to_poisson, ratio_to_cox
  grad_us / hvp_us       one loglik + gradient / one Hessian matvec call
                         (host pointers, synchronous)
  shape_us_k1, shape_us_k8  one shape_loglik call on the cached linear
                         predictor at 1 and at 8 values of k (one launch, one
                         wait), and shape_k8_over_k1
  shape_with_product_us  one call at 1 value with coefficients (the product
                         included)
  gibbs_it_s, mean_shape over `steps` Gibbs iterations after `warmup`
  (gibbs_resume), 'hmc', shape sampled.
One JSON line per shape.  --no-cox leaves the Cox handle (and its second
design) out.  --profile-steps N: only N-step trajectories of the handles and
20 shape calls at K = 1 and K = 8 after a short warm-up, for a kernel trace in
a run of its own.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_negbin import leapfrog_us, timed  # noqa: E402
from bench_poisson import make_X, products_us  # noqa: E402
from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,  # noqa: E402
                             HipSparseDesignMatrix, RegressionCoefPrior,
                             RegressionModel, WeibullModel, simulate)


def _design(kind, X, intercept):
    if kind == 'binary':
        return HipSparseDesignMatrix(X, add_intercept=intercept,
                                     center_predictor=True)
    return HipDenseDesignMatrix(X, add_intercept=intercept,
                                center_predictor=True,
                                storage_dtype='float32')


def cox_leapfrog_us(kind, X, et, ct, n_traj):
    """The plain Cox handle on the same outcome: rows sorted into the Cox
    model's order, a design of its own without an intercept column."""
    from bayesbridge_amd.model import cox_preprocess
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        et, ct, Xs, _ = cox_preprocess(et, ct, X)
        cox = RegressionModel((et, ct), _design(kind, Xs, False), 'cox')
    del Xs
    b = np.random.RandomState(1).randn(cox.design.shape[1]) * .01
    return leapfrog_us(cox, n_traj, b, np.random.RandomState(2))


def run(kind, n, p, steps, warmup, seed=0, profile_steps=0, with_cox=True):
    X = make_X(kind, n, p, seed)
    beta = simulate.demo_beta(p) * .25
    et, ct = WeibullModel.simulate_outcome(X, beta, 1.5, .5, seed=seed)
    n_traj = profile_steps or 64
    head = {'shape': '%s:%dx%d' % (kind, n, p),
            'event_frac': round(float(np.mean(np.isfinite(et))), 3)}
    if with_cox:
        head['cox_leapfrog_us'] = round(
            cox_leapfrog_us(kind, X, et, ct, n_traj), 1)
    design = _design(kind, X, True)
    del X
    d = np.isfinite(et).astype(np.float64)
    t = np.minimum(et, ct)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((et, ct), design, 'weibull')
        poisson = RegressionModel((d, t), design, 'poisson')
    model.shape = 1.5
    P = design.shape[1]
    rs = np.random.RandomState(1)
    b = rs.randn(P) * .01
    leap = {name: leapfrog_us(m, n_traj, b, np.random.RandomState(2))
            for name, m in (('weibull', model), ('poisson', poisson))}
    k8 = np.exp(np.linspace(-1., 1.5, 8))
    model.shape_loglik(b, 1.5)
    reps = 20
    us1 = timed(lambda: model.shape_loglik(None, 1.5), reps)
    us8 = timed(lambda: model.shape_loglik(None, k8), reps)
    head.update({'leapfrog_us': round(leap['weibull'], 1),
                 'poisson_leapfrog_us': round(leap['poisson'], 1),
                 'ratio_to_poisson': round(leap['weibull'] / leap['poisson'],
                                           3),
                 'shape_us_k1': round(us1, 1), 'shape_us_k8': round(us8, 1),
                 'shape_k8_over_k1': round(us8 / us1, 3)})
    if with_cox:
        head['ratio_to_cox'] = round(
            leap['weibull'] / head['cox_leapfrog_us'], 3)
    if profile_steps:
        return {**head, 'profile_steps': n_traj}
    prod_us = products_us(design, 50)
    head.update({
        'products_us': round(prod_us, 1),
        'ratio': round(leap['weibull'] / prod_us, 3),
        'grad_us': round(timed(
            lambda: model.compute_loglik_and_gradient(b), 10), 1),
        'shape_with_product_us': round(timed(
            lambda: model.shape_loglik(b, 1.5), 10), 1)})
    op = model.get_hessian_matvec_operator(b)
    v = rs.randn(P)
    head['hvp_us'] = round(timed(lambda: op(v), 10), 1)
    prior = RegressionCoefPrior(bridge_exponent=.25,
                                regularizing_slab_size=1.)
    bridge = BayesBridge(model, prior)
    coef = rs.randn(P) * .01
    coef[0] = model.calc_intercept_mle()
    init = {'global_scale': .1, 'local_scale': np.ones(P - 1), 'coef': coef,
            'weibull_shape': 1.5}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, info = bridge.gibbs(warmup, init=init, seed=0,
                               params_to_save=('weibull_shape',))
        tic = time.perf_counter()
        samples, info = bridge.gibbs_resume(info, steps)
    it_s = steps / (time.perf_counter() - tic)
    si = info['_reg_coef_sampling_info']
    return {**head, 'gibbs_it_s': round(it_s, 3),
            'mean_n_step': float(np.mean(si['n_integrator_step'])),
            'mean_shape': float(np.mean(samples['weibull_shape']))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+',
                    default=['binary:1000000x50000', 'dense:100000x2000'])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--profile-steps', type=int, default=0)
    ap.add_argument('--no-cox', action='store_true')
    a = ap.parse_args()
    for s in a.shapes:
        kind, size = s.split(':')
        n, p = (int(x) for x in size.split('x'))
        print(json.dumps(run(kind, n, p, a.steps, a.warmup,
                             profile_steps=a.profile_steps,
                             with_cox=not a.no_cox)), flush=True)


if __name__ == '__main__':
    main()
