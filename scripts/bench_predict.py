"""Posterior prediction of the logit model on its training rows
(LogisticModel.predict on bbx_design_predictive_summary, csrc/predict.hip):

    python scripts/bench_predict.py [--shape 1000000x50000] [--draws 256]

A simulated binary design and outcome (demo coefficients), S draws scattered
around them, then per draw, the best of --repeat runs:
  products_us       the yardstick: the S products X~ beta_s enqueued back to
                    back on device pointers (bbx_design_dot_dev) with ONE
                    synchronisation, and nothing else
  predict_us        one prediction of the training rows without their outcome
                    (mean and sd of the success probability) from draw-major
                    draws, wall time / S
  predict_score_us  the same with the training outcome (also lpd,
                    loglik_mean, loglik_var), wall time / S
  ratio, ratio_score  the two over products_us
  public_us         model.predict(coef) as a user calls it on (P, S) draws:
                    predict_score_us plus the transposition of the draws into
                    draw-major order (transpose_us) and the checks and
                    the log binomial coefficient of the outcome
  upload_us         what moving the S x P draws from pageable host memory to
                    the device costs on its own (torch), per draw: part of
                    both predict figures, absent from the yardstick
  launches          kernel launches per draw of a predict call / of a product
One JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayes-bridge_amd"))

from bayesbridge_amd import (HipSparseDesignMatrix, RegressionModel,  # noqa: E402
                             _lib, simulate)


def best(fn, repeat):
    times = []
    for _ in range(repeat):
        tic = time.perf_counter()
        fn()
        times.append(time.perf_counter() - tic)
    return min(times)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='1000000x50000')
    ap.add_argument('--draws', type=int, default=256)
    ap.add_argument('--repeat', type=int, default=3)
    a = ap.parse_args()
    n, p = (int(x) for x in a.shape.split('x'))
    S = a.draws
    indptr, indices = simulate.simulate_binary_csr_device(n, p, .002, seed=0)
    indptr, indices = indptr.cpu().numpy(), indices.cpu().numpy()
    X = sparse.csr_matrix((np.ones(len(indices)), indices, indptr),
                          shape=(n, p))
    outcome = simulate.simulate_outcome(X, simulate.demo_beta(p), 'logit',
                                        seed=0)
    design = HipSparseDesignMatrix(X, add_intercept=True,
                                   center_predictor=True)
    del X
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel(outcome, design, 'logit')
    P = design.shape[1]
    rs = np.random.RandomState(1)
    beta = np.concatenate(([0.], simulate.demo_beta(p)))
    coef = beta[:, None] + .01 * rs.randn(P, S)
    lib = _lib.load()

    # the yardstick: S products, one synchronisation
    pitch = (P + 31) // 32 * 32
    d_coef = torch.zeros((S, pitch), dtype=torch.float64, device='cuda')
    d_coef[:, :P] = torch.from_numpy(np.ascontiguousarray(coef.T)).cuda()
    d_eta = torch.empty((16, n), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()

    def products():
        for s in range(S):
            _lib.check(lib.bbx_design_dot_dev(
                design.handle, d_coef[s].data_ptr(), d_eta[s % 16].data_ptr()))
        design.synchronize()

    products()
    count = lib.bbx_launch_count()
    products_s = best(products, a.repeat)
    launches_product = (lib.bbx_launch_count() - count) / (a.repeat * S)

    host = np.ascontiguousarray(coef.T)

    def upload():
        torch.from_numpy(host).cuda()
        torch.cuda.synchronize()

    upload()
    upload_s = best(upload, a.repeat)

    from bayesbridge_amd.model import _coef_draws
    draws = _coef_draws(coef, P)[0]
    transpose_s = best(lambda: _coef_draws(coef, P), a.repeat)
    y, m = model.n_success, model.n_trial
    const = np.zeros(n)          # log C(1, y): a binary outcome

    def plain():
        model._predictive_summary(draws, None, n)

    def scored():
        return model._predictive_summary(draws, None, n, y=y, n_trial=m,
                                         ll_const=const)

    plain()
    count = lib.bbx_launch_count()
    plain_s = best(plain, a.repeat)
    launches = (lib.bbx_launch_count() - count) / (a.repeat * S)
    scored()
    score_s = best(scored, a.repeat)
    res = model.predict(coef)
    public_s = best(lambda: model.predict(coef), a.repeat)
    us = 1e6 / S
    print(json.dumps({
        'shape': 'binary:%dx%d' % (n, p), 'draws': S,
        'products_us': round(products_s * us, 1),
        'predict_us': round(plain_s * us, 1),
        'predict_score_us': round(score_s * us, 1),
        'ratio': round(plain_s / products_s, 3),
        'ratio_score': round(score_s / products_s, 3),
        'upload_us': round(upload_s * us, 1),
        'public_us': round(public_s * us, 1),
        'transpose_us': round(transpose_s * us, 1),
        'launches': round(launches, 3),
        'launches_product': round(launches_product, 3),
        'waic': res['waic'], 'p_waic': res['p_waic']}), flush=True)


if __name__ == '__main__':
    main()
