"""Ordinal (proportional-odds) model on the device next to the logit handle on
the same design, in one process:

    python scripts/bench_ordinal.py --shapes binary:1000000x50000 \\
        dense:100000x2000 [--steps 5 --warmup 2 --categories 7]

For each shape: a simulated outcome of `categories` levels (demo coefficients,
cutpoints spread 2 either side of the linear predictor's median), on a design
without an intercept column, then
  leapfrog_us            one step of a 64-step device trajectory (one host
                         wait) on the ordinal handle
  logit_leapfrog_us      the same on a logit handle of the same design with
                         the dichotomised outcome y >= 1: its row kernel does
                         half the transcendental work per row (one exp, one
                         log1p against two and two)
  products_us            X~ v + X~^T w on device pointers, same stream
  ratio, ratio_to_logit
  grad_us / hvp_us       one loglik + gradient / one Hessian matvec call
                         (host pointers, synchronous)
  cut_us_c1, cut_us_c8   one cutpoint_loglik call on the cached linear
                         predictor at 1 and at 8 cutpoint vectors (one launch,
                         one wait), and cut_c8_over_c1
  cut_with_product_us    one call at 1 vector with coefficients (the product
                         included)
  gibbs_it_s over `steps` Gibbs iterations after `warmup` (gibbs_resume),
  'hmc', cutpoints sampled; cutpoint_share: the share of that time spent in
  the K - 1 slice updates of the cutpoints (the driver's update_cutpoints,
  timed around its call), cutpoint_ms_per_it the same per iteration.
One JSON line per shape.  --profile-steps N: only N-step trajectories of the
two handles and 20 cutpoint calls at n_c = 1 and n_c = 8 after a short
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

from bench_negbin import leapfrog_us, timed  # noqa: E402
from bench_poisson import make_X, products_us  # noqa: E402
from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,  # noqa: E402
                             HipSparseDesignMatrix, OrdinalModel,
                             RegressionCoefPrior, RegressionModel, simulate)


def gibbs_it_s(model, P, steps, warmup, rs):
    """(it/s, seconds inside update_cutpoints, sampling info, samples)."""
    from bayesbridge_amd import bayesbridge
    spent, real = [0.], bayesbridge.update_cutpoints

    def clocked(*args, **kw):
        tic = time.perf_counter()
        out = real(*args, **kw)
        spent[0] += time.perf_counter() - tic
        return out

    prior = RegressionCoefPrior(bridge_exponent=.25,
                                regularizing_slab_size=1.)
    bridge = BayesBridge(model, prior)
    init = {'global_scale': .1, 'local_scale': np.ones(P),
            'coef': rs.randn(P) * .01}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, info = bridge.gibbs(warmup, init=init, seed=0,
                               params_to_save=('cutpoints',))
        bayesbridge.update_cutpoints = clocked
        try:
            tic = time.perf_counter()
            samples, info = bridge.gibbs_resume(info, steps)
            elapsed = time.perf_counter() - tic
        finally:
            bayesbridge.update_cutpoints = real
    return steps / elapsed, spent[0] / elapsed, \
        info['_reg_coef_sampling_info'], samples


def run(kind, n, p, steps, warmup, K, seed=0, profile_steps=0):
    X = make_X(kind, n, p, seed)
    beta = simulate.demo_beta(p) * .25
    eta = np.asarray(X.dot(beta), dtype=np.float64).ravel()
    cuts = np.median(eta) + np.linspace(-2., 2., K - 1)
    y = OrdinalModel.simulate_outcome(X, beta, cuts, seed=seed)
    assert len(np.unique(y)) == K
    if kind == 'binary':
        design = HipSparseDesignMatrix(X, add_intercept=False,
                                       center_predictor=True)
    else:
        design = HipDenseDesignMatrix(X, add_intercept=False,
                                      center_predictor=True,
                                      storage_dtype='float32')
    del X
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel(y, design, 'ordinal')
        logit = RegressionModel((y >= 1).astype(np.float64), design, 'logit')
    P = design.shape[1]
    rs = np.random.RandomState(1)
    b = rs.randn(P) * .01
    n_traj = profile_steps or 64
    head = {'shape': '%s:%dx%d' % (kind, n, p), 'categories': K}
    leap = {name: leapfrog_us(m, n_traj, b, np.random.RandomState(2))
            for name, m in (('ordinal', model), ('logit', logit))}
    c1 = model.cutpoints
    c8 = c1[None, :] + np.linspace(-.2, .2, 8)[:, None]
    model.cutpoint_loglik(b, c1)
    reps = 20
    k1 = timed(lambda: model.cutpoint_loglik(None, c1), reps)
    k8 = timed(lambda: model.cutpoint_loglik(None, c8), reps)
    head.update({'leapfrog_us': round(leap['ordinal'], 1),
                 'logit_leapfrog_us': round(leap['logit'], 1),
                 'cut_us_c1': round(k1, 1), 'cut_us_c8': round(k8, 1),
                 'cut_c8_over_c1': round(k8 / k1, 3)})
    if profile_steps:
        return {**head, 'profile_steps': n_traj}
    prod_us = products_us(design, 50)
    head.update({
        'products_us': round(prod_us, 1),
        'ratio': round(leap['ordinal'] / prod_us, 3),
        'ratio_to_logit': round(leap['ordinal'] / leap['logit'], 3),
        'grad_us': round(timed(
            lambda: model.compute_loglik_and_gradient(b), 10), 1),
        'cut_with_product_us': round(timed(
            lambda: model.cutpoint_loglik(b, c1), 10), 1)})
    op = model.get_hessian_matvec_operator(b)
    v = rs.randn(P)
    head['hvp_us'] = round(timed(lambda: op(v), 10), 1)
    it_s, share, si, samples = gibbs_it_s(model, P, steps, warmup,
                                          np.random.RandomState(3))
    return {**head, 'gibbs_it_s': round(it_s, 3),
            'cutpoint_share': round(share, 4),
            'cutpoint_ms_per_it': round(share / it_s * 1e3, 2),
            'mean_n_step': float(np.mean(si['n_integrator_step'])),
            'last_cutpoints': [round(float(c), 3)
                               for c in samples['cutpoints'][:, -1]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+',
                    default=['binary:1000000x50000', 'dense:100000x2000'])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--categories', type=int, default=7)
    ap.add_argument('--profile-steps', type=int, default=0)
    a = ap.parse_args()
    for s in a.shapes:
        kind, size = s.split(':')
        n, p = (int(x) for x in size.split('x'))
        print(json.dumps(run(kind, n, p, a.steps, a.warmup, a.categories,
                             profile_steps=a.profile_steps)), flush=True)


if __name__ == '__main__':
    main()
