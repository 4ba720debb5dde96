"""Gibbs iterations per second of the censored-outcome chain (family='lognormal',
the log-normal AFT model) beside the linear chain on the same rows and the
Weibull chain under 'hmc' on the same simulated times, all from the same
library in the same process, and the cost of its latent kernel and its extra
product:

    python scripts/bench_censored.py --case sparse --steps 20 --warmup 5
    python scripts/bench_censored.py --case dense  --steps 20 --warmup 5
    python scripts/bench_censored.py --case sparse --profile DIR

  sparse  binary CSR 1 000 000 x 50 000 (bench.py's config3: column
          frequency .002), 'cg': lognormal and linear; weibull under 'hmc'
          -- it/s and the mean number of CG iterations (of integrator steps);
  dense   f32 storage 100 000 x 2 000, 'cholesky' and 'cg': lognormal and
          linear; weibull under 'hmc'.

The kernel times (latent_row_kernel<CensoredRows>, the rss pass and the finish kernels,
the fold, the extra X~^T w) come from a `rocprofv3 --kernel-trace --stats` run
of a case on its own (--profile wraps it; its rates are not the timed ones).

The times are log-normal around exp(eta) with unit spread, half of them
censored (LogNormalAFTModel.simulate_outcome); the linear chain takes log t of
every row as observed.  The lognormal and linear chains start from coef = 0
with global_scale .01, the Weibull chain from scripts/bench_weibull.py's start
(small random coefficients, the intercept's MLE, shape 1.5); no mode search.
Each runs `warmup` untimed iterations, then `steps` timed ones (gibbs_resume).
One JSON line per (case, model, sampler).  Every leg runs as a child process
under a time limit of its own (--limit seconds); a leg that fails or runs out
ends the script.
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


def _chain_rate(design, model, outcome, sampler, steps, warmup):
    from bayesbridge_amd import (BayesBridge, RegressionCoefPrior,
                                 RegressionModel)
    bridge = BayesBridge(RegressionModel(outcome, design, model),
                         RegressionCoefPrior(bridge_exponent=.5,
                                             regularizing_slab_size=2.))
    P = design.shape[1]
    init = {'global_scale': .01, 'coef': np.zeros(P)}
    if model == 'weibull':
        # (its host-side scale updates need non-zero coefficients: the start of
        # scripts/bench_weibull.py)
        coef = np.random.RandomState(0).randn(P) * .01
        coef[0] = bridge.model.calc_intercept_mle()
        init = {'global_scale': .1, 'local_scale': np.ones(P - 1),
                'coef': coef, 'weibull_shape': 1.5}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, info = bridge.gibbs(warmup, seed=1, coef_sampler_type=sampler,
                               init=init)
        design.synchronize()
        t = time.perf_counter()
        samples, info2 = bridge.gibbs_resume(info, steps)
        design.synchronize()
        dt = time.perf_counter() - t
    si = info2['_reg_coef_sampling_info']
    work = si.get('n_cg_iter', si.get('n_integrator_step'))
    censored = getattr(bridge.model, 'status', None)
    return {'model': model, 'sampler': sampler, 'n': design.shape[0], 'P': P,
            'gibbs_it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps,
            'mean_n_cg_iter' if 'n_cg_iter' in si else 'mean_n_step':
            None if work is None else float(np.mean(work)),
            'censored_share': None if censored is None
            else float(np.mean(censored != 0))}


def _outcomes(X, beta):
    from bayesbridge_amd import LogNormalAFTModel
    event, censoring = LogNormalAFTModel.simulate_outcome(X, beta, 1., .5,
                                                          seed=1)
    return {'lognormal': (event, censoring), 'weibull': (event, censoring),
            'linear': np.log(np.minimum(event, censoring))}


def _run(design, outcomes, samplers, args, case):
    for model in args.models or ('lognormal', 'linear', 'weibull'):
        for sampler in (('hmc',) if model == 'weibull' else samplers):
            out = _chain_rate(design, model, outcomes[model], sampler,
                              args.steps, args.warmup)
            print(json.dumps(dict(out, case=case)), flush=True)


def leg_sparse(args):
    from bayesbridge_amd import HipSparseDesignMatrix, simulate
    X = simulate.simulate_binary_csr_fast(args.n or 1000000, args.p or 50000,
                                          .002, seed=3)
    outcomes = _outcomes(X, simulate.demo_beta(X.shape[1]))
    design = HipSparseDesignMatrix(X, center_predictor=True,
                                   add_intercept=True)
    _run(design, outcomes, ('cg',), args, 'sparse')


def leg_dense(args):
    from bayesbridge_amd import HipDenseDesignMatrix, simulate
    n, p = args.n or 100000, args.p or 2000
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, p), dtype=np.float32)
    outcomes = _outcomes(X, simulate.demo_beta(p).astype(np.float32))
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                                  storage_dtype='float32')
    del X
    _run(design, outcomes, ('cholesky', 'cg'), args, 'dense')


LEGS = {'sparse': leg_sparse, 'dense': leg_dense}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', choices=sorted(LEGS), required=True)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--n', type=int, default=0)
    ap.add_argument('--p', type=int, default=0)
    ap.add_argument('--models', nargs='*')
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
           '--p', str(args.p)]
    if args.models:
        own += ['--models'] + list(args.models)
    cmd = own
    if args.profile:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', args.profile,
               '--'] + own
    cmd = ['timeout', '-k', '10', str(args.limit)] + cmd
    status = subprocess.call(cmd)
    if status != 0:
        print("bench_censored: the %s leg ended with status %d"
              % (args.case, status), file=sys.stderr)
    return status


if __name__ == "__main__":
    sys.exit(main())
