"""Gibbs iterations per second of the device-resident chain with the
'cholesky' coefficient draw against the 'cg' draw, on dense f32-stored
designs (N(0, 1) entries, demo coefficients), logit and linear:

    python scripts/bench_cholesky.py --sizes 100000x500 100000x2000 \
        --steps 10 --warmup 3

Each run starts from coef = 0 with global_scale .01 (no mode search), runs
`warmup` untimed iterations, then `steps` timed ones (gibbs_resume).  One JSON
line per (size, model, sampler).
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayes-bridge_amd"))

from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,  # noqa: E402
                             RegressionCoefPrior, RegressionModel, simulate)


def run(n, p, steps, warmup, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p), dtype=np.float32)
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                                  storage_dtype='float32')
    beta = simulate.demo_beta(p)
    eta = (X @ beta.astype(np.float32)).astype(np.float64)
    outcomes = {
        'linear': eta + rng.standard_normal(n),
        'logit': (rng.binomial(1, 1 / (1 + np.exp(-eta))).astype(float),
                  np.ones(n)),
    }
    del X
    for model, y in outcomes.items():
        for sampler in ('cg', 'cholesky'):
            bridge = BayesBridge(RegressionModel(y, design, model),
                                 RegressionCoefPrior(bridge_exponent=.5,
                                                     regularizing_slab_size=2.))
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                _, info = bridge.gibbs(
                    warmup, seed=1, coef_sampler_type=sampler,
                    init={'global_scale': .01, 'coef': np.zeros(p + 1)})
                design.synchronize()
                t = time.perf_counter()
                _, info2 = bridge.gibbs_resume(info, steps)
                design.synchronize()
                dt = time.perf_counter() - t
            ncg = info2['_reg_coef_sampling_info'].get('n_cg_iter')
            print(json.dumps({
                'n': n, 'P': p + 1, 'model': model, 'sampler': sampler,
                'gibbs_it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps,
                'mean_n_cg_iter': None if ncg is None else float(np.mean(ncg)),
            }), flush=True)
            bridge._destroy_chain()
    design.release_sampler_memory()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', default=['100000x500'])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    for s in a.sizes:
        n, p = (int(v) for v in s.split('x'))
        run(n, p, a.steps, a.warmup)
