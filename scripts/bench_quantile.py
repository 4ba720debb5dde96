"""Gibbs iterations per second of the quantile chain (family='quantile', q =
--quantile, default 0.9) beside the Student-t and linear chains of the same
library, and the cost of its two row passes:

    python scripts/bench_quantile.py --case sparse --steps 20 --warmup 5
    python scripts/bench_quantile.py --case dense  --steps 20 --warmup 5
    python scripts/bench_quantile.py --case sparse --profile DIR

  sparse  binary CSR 1 000 000 x 50 000 (bench.py's config3: column
          frequency .002), 'cg': quantile, student_t and linear
          -- it/s and the mean number of CG iterations;
  dense   f32 storage 100 000 x 2 000, 'cholesky' and 'cg': quantile,
          student_t and linear (the weighted Gram of every iteration is the
          logit model's cost).

The kernel times (pass A quantile_sum_kernel, pass B
latent_row_kernel<QuantileRows>, beside Student-t's pass B
latent_row_kernel<StudentTRows>) come from a `rocprofv3 --kernel-trace
--stats` run of a case on its own (--profile wraps it; its rates are not the
timed ones).

The outcome is eta + t_4 noise for all three models.  Each chain starts
from coef = 0 with global_scale .01 (no mode search), runs `warmup` untimed
iterations, then `steps` timed ones (gibbs_resume).  One JSON line per (case,
model, sampler).  Every leg runs as a child process under a time limit of its
own (--limit seconds); a leg that fails or runs out ends the script.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayes-bridge_amd"))


def _chain_rate(design, model, y, sampler, steps, warmup, quantile):
    from bayesbridge_amd import (BayesBridge, RegressionCoefPrior,
                                 RegressionModel)
    kw = {'quantile': quantile} if model == 'quantile' else {}
    bridge = BayesBridge(RegressionModel(y, design, model, **kw),
                         RegressionCoefPrior(bridge_exponent=.5,
                                             regularizing_slab_size=2.))
    P = design.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, info = bridge.gibbs(warmup, seed=1, coef_sampler_type=sampler,
                               init={'global_scale': .01, 'coef': np.zeros(P)})
        design.synchronize()
        t = time.perf_counter()
        _, info2 = bridge.gibbs_resume(info, steps)
        design.synchronize()
        dt = time.perf_counter() - t
    ncg = info2['_reg_coef_sampling_info'].get('n_cg_iter')
    return {'model': model, 'sampler': sampler, 'n': design.shape[0], 'P': P,
            'gibbs_it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps,
            'mean_n_cg_iter': None if ncg is None else float(np.mean(ncg))}


def leg_sparse(args):
    from bayesbridge_amd import HipSparseDesignMatrix, simulate
    X = simulate.simulate_binary_csr_fast(args.n or 1000000, args.p or 50000,
                                          .002, seed=3)
    beta = simulate.demo_beta(X.shape[1])
    rng = np.random.default_rng(1)
    y = X.dot(beta) + rng.standard_t(4., X.shape[0])
    design = HipSparseDesignMatrix(X, center_predictor=True,
                                   add_intercept=True)
    for model in args.models or ('quantile', 'student_t', 'linear'):
        out = _chain_rate(design, model, y, 'cg', args.steps, args.warmup,
                          args.quantile)
        print(json.dumps(dict(out, case='sparse')), flush=True)


def leg_dense(args):
    from bayesbridge_amd import HipDenseDesignMatrix, simulate
    n, p = args.n or 100000, args.p or 2000
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, p), dtype=np.float32)
    beta = simulate.demo_beta(p)
    eta = (X @ beta.astype(np.float32)).astype(np.float64)
    y = eta + rng.standard_t(4., n)
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                                  storage_dtype='float32')
    del X
    for model in args.models or ('quantile', 'student_t', 'linear'):
        for sampler in args.samplers or ('cholesky', 'cg'):
            out = _chain_rate(design, model, y, sampler, args.steps,
                              args.warmup, args.quantile)
            print(json.dumps(dict(out, case='dense')), flush=True)


LEGS = {'sparse': leg_sparse, 'dense': leg_dense}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=sorted(LEGS), required=True)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--p', type=int, default=0)
    ap.add_argument('--models', nargs='*')
    ap.add_argument('--samplers', nargs='*',
                    help="dense case: 'cholesky' and / or 'cg' (default both)")
    ap.add_argument('--quantile', type=float, default=.9)
    ap.add_argument('--limit', type=int, default=420,
                    help="seconds the leg's child process may run")
    ap.add_argument('--profile', metavar='DIR',
                    help="run the leg under rocprofv3 --kernel-trace --stats "
                         "with its output in DIR (a run of its own: its rates "
                         "are not the timed ones)")
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        LEGS[args.case](args)
        return 0
    own = [sys.executable, os.path.abspath(__file__), '--child',
           '--case', args.case, '--steps', str(args.steps),
           '--warmup', str(args.warmup), '--n', str(args.n),
           '--p', str(args.p), '--quantile', str(args.quantile)]
    if args.models:
        own += ['--models'] + list(args.models)
    if args.samplers:
        own += ['--samplers'] + list(args.samplers)
    cmd = own
    if args.profile:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format',
               'csv', '-d', args.profile, '--'] + own
    cmd = ['timeout', '-k', '10', str(args.limit)] + cmd
    status = subprocess.call(cmd)
    if status != 0:
        print("bench_quantile: the %s leg ended with status %d"
              % (args.case, status), file=sys.stderr)
    return status


if __name__ == "__main__":
    sys.exit(main())
