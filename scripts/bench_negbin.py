"""Negative-binomial model on the device next to the Poisson and logit handles
on the same rows, in one process:

    python scripts/bench_negbin.py --shapes binary:1000000x50000 \\
        dense:100000x2000 [--steps 5 --warmup 2]

For each shape: simulated overdispersed counts with an exposure (demo
coefficients, dispersion 3), then
  leapfrog_us            one step of a 64-step device trajectory (one host
                         wait) on the negative-binomial handle
  poisson_leapfrog_us    the same on a Poisson handle of the same counts
  logit_leapfrog_us      the same on a logit handle of the rows (outcome
                         y > 0): its row kernel does the same transcendental
                         work per row (one exp, one log1p)
  products_us            X~ v + X~^T w on device pointers, same stream
  ratio, ratio_to_poisson
  grad_us / hvp_us       one loglik + gradient / one Hessian matvec call
                         (host pointers, synchronous)
  disp_us_k1, disp_us_k8 one dispersion_loglik call on the cached linear
                         predictor at 1 and at 8 values of r (one launch, one
                         wait), and disp_k8_over_k1
  disp_with_product_us   one call at 1 value with coefficients (the product
                         included)
  gibbs_it_s, mean_dispersion over `steps` Gibbs iterations after `warmup`
  (gibbs_resume), 'hmc', dispersion sampled.
One JSON line per shape.  --profile-steps N: only N-step trajectories of the
three handles and 20 dispersion calls at K = 1 and K = 8 after a short
warm-up, for a kernel trace in a run of its own.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_poisson import make_X, products_us  # noqa: E402
from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,  # noqa: E402
                             HipSparseDesignMatrix, NegBinModel,
                             RegressionCoefPrior, RegressionModel, simulate)


def leapfrog_us(model, n_traj, b, rs):
    """One step of an n_traj-step trajectory from b: the step is far too
    small for the stop rule to fire."""
    P = len(b)
    scale, pp = np.full(P, .05), np.ones(P)
    q0, p0 = b / scale, rs.randn(P)
    ll, g = model.hamiltonian_loglik_and_gradient(q0 * scale)
    logp0 = ll - np.sum(q0 ** 2) / 2
    grad0 = scale * g - q0
    model.hmc_trajectory(1e-5, 4, scale, pp, q0, p0, logp0, grad0, 1e300)
    tic = time.perf_counter()
    tr = model.hmc_trajectory(1e-5, n_traj, scale, pp, q0, p0, logp0, grad0,
                              1e300)
    elapsed = time.perf_counter() - tic
    assert tr['n_steps'] == n_traj, tr
    return elapsed / n_traj * 1e6


def timed(fn, reps):
    fn()
    tic = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - tic) / reps * 1e6


def run(kind, n, p, steps, warmup, seed=0, profile_steps=0):
    X = make_X(kind, n, p, seed)
    beta = simulate.demo_beta(p) * .25
    exposure = np.random.RandomState(seed).uniform(.5, 2., n)
    y = NegBinModel.simulate_outcome(X, beta, 3., exposure=exposure, seed=seed)
    if kind == 'binary':
        design = HipSparseDesignMatrix(X, add_intercept=True,
                                       center_predictor=True)
    else:
        design = HipDenseDesignMatrix(X, add_intercept=True,
                                      center_predictor=True,
                                      storage_dtype='float32')
    del X
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((y, exposure), design, 'negbin')
        poisson = RegressionModel((y, exposure), design, 'poisson')
        logit = RegressionModel((y > 0).astype(np.float64), design, 'logit')
    P = design.shape[1]
    rs = np.random.RandomState(1)
    b = rs.randn(P) * .01
    n_traj = profile_steps or 64
    head = {'shape': '%s:%dx%d' % (kind, n, p), 'max_count': int(y.max())}
    leap = {name: leapfrog_us(m, n_traj, b, np.random.RandomState(2))
            for name, m in (('negbin', model), ('poisson', poisson),
                            ('logit', logit))}
    r8 = np.exp(np.linspace(-1., 3., 8))
    model.dispersion_loglik(b, 3.)
    reps = 20
    k1 = timed(lambda: model.dispersion_loglik(None, 3.), reps)
    k8 = timed(lambda: model.dispersion_loglik(None, r8), reps)
    head.update({'leapfrog_us': round(leap['negbin'], 1),
                 'poisson_leapfrog_us': round(leap['poisson'], 1),
                 'logit_leapfrog_us': round(leap['logit'], 1),
                 'disp_us_k1': round(k1, 1), 'disp_us_k8': round(k8, 1),
                 'disp_k8_over_k1': round(k8 / k1, 3)})
    if profile_steps:
        return {**head, 'profile_steps': n_traj}
    prod_us = products_us(design, 50)
    head.update({
        'products_us': round(prod_us, 1),
        'ratio': round(leap['negbin'] / prod_us, 3),
        'ratio_to_poisson': round(leap['negbin'] / leap['poisson'], 3),
        'grad_us': round(timed(
            lambda: model.compute_loglik_and_gradient(b), 10), 1),
        'disp_with_product_us': round(timed(
            lambda: model.dispersion_loglik(b, 3.), 10), 1)})
    op = model.get_hessian_matvec_operator(b)
    v = rs.randn(P)
    head['hvp_us'] = round(timed(lambda: op(v), 10), 1)
    prior = RegressionCoefPrior(bridge_exponent=.25,
                                regularizing_slab_size=1.)
    bridge = BayesBridge(model, prior)
    coef = rs.randn(P) * .01
    coef[0] = model.calc_intercept_mle()
    init = {'global_scale': .1, 'local_scale': np.ones(P - 1), 'coef': coef}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, info = bridge.gibbs(warmup, init=init, seed=0,
                               params_to_save=('dispersion',))
        tic = time.perf_counter()
        samples, info = bridge.gibbs_resume(info, steps)
    it_s = steps / (time.perf_counter() - tic)
    si = info['_reg_coef_sampling_info']
    return {**head, 'gibbs_it_s': round(it_s, 3),
            'mean_n_step': float(np.mean(si['n_integrator_step'])),
            'mean_dispersion': float(np.mean(samples['dispersion']))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+',
                    default=['binary:1000000x50000', 'dense:100000x2000'])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--profile-steps', type=int, default=0)
    a = ap.parse_args()
    for s in a.shapes:
        kind, size = s.split(':')
        n, p = (int(x) for x in size.split('x'))
        print(json.dumps(run(kind, n, p, a.steps, a.warmup,
                             profile_steps=a.profile_steps)), flush=True)


if __name__ == '__main__':
    main()
