"""Gibbs iterations per second of the probit chain (family='probit') beside
the logit and linear chains of the same library, and the cost of its latent
update:

    python scripts/bench_probit.py --case sparse --steps 20 --warmup 5
    python scripts/bench_probit.py --case dense  --steps 20 --warmup 5
    python scripts/bench_probit.py --case latent --n 1000000

  sparse  binary CSR 1 000 000 x 50 000 (bench.py's config3: column
          frequency .002), 'cg': probit and logit
          -- it/s and the mean number of CG iterations;
  dense   f32 storage 100 000 x 2 000, 'cholesky' and 'cg': probit, logit and
          linear;
  latent  bbx_device_truncated_normal and bbx_device_polya_gamma on n rows at
          psi ~ N(0, 1.5^2): wall time per call, uploads included, so only the
          difference of two sizes says anything about the kernels -- their
          times (the chain's is latent_row_kernel<ProbitRows<double>>) come
          from a `rocprofv3 --kernel-trace --stats` run of the sparse case on
          its own (--profile wraps it).

Each chain starts from coef = 0 with global_scale .01 (no mode search), runs
`warmup` untimed iterations, then `steps` timed ones (gibbs_resume).  One JSON
line per (case, model, sampler).  Every leg runs as a child process under a
time limit of its own (--limit seconds); a leg that fails or runs out ends the
script.
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


def _chain_rate(design, model, y, sampler, steps, warmup):
    from bayesbridge_amd import (BayesBridge, RegressionCoefPrior,
                                 RegressionModel)
    bridge = BayesBridge(RegressionModel(y, design, model),
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
    from scipy.special import ndtr
    from bayesbridge_amd import HipSparseDesignMatrix, simulate
    X = simulate.simulate_binary_csr_fast(args.n or 1000000, args.p or 50000,
                                          .002, seed=3)
    beta = simulate.demo_beta(X.shape[1])
    eta = X.dot(beta)
    rng = np.random.default_rng(1)
    u = rng.random(X.shape[0])
    y = {'probit': (u < ndtr(eta)).astype(float),
         'logit': ((u < 1 / (1 + np.exp(-eta))).astype(float),
                   np.ones(X.shape[0]))}
    design = HipSparseDesignMatrix(X, center_predictor=True,
                                   add_intercept=True)
    for model in args.models or ('probit', 'logit'):
        out = _chain_rate(design, model, y[model], 'cg', args.steps,
                          args.warmup)
        print(json.dumps(dict(out, case='sparse')), flush=True)


def leg_dense(args):
    from scipy.special import ndtr
    from bayesbridge_amd import HipDenseDesignMatrix, simulate
    n, p = args.n or 100000, args.p or 2000
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, p), dtype=np.float32)
    beta = simulate.demo_beta(p)
    eta = (X @ beta.astype(np.float32)).astype(np.float64)
    u = rng.random(n)
    y = {'probit': (u < ndtr(eta)).astype(float),
         'logit': ((u < 1 / (1 + np.exp(-eta))).astype(float), np.ones(n)),
         'linear': eta + rng.standard_normal(n)}
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                                  storage_dtype='float32')
    del X
    for model in args.models or ('probit', 'logit', 'linear'):
        for sampler in ('cholesky', 'cg'):
            out = _chain_rate(design, model, y[model], sampler, args.steps,
                              args.warmup)
            print(json.dumps(dict(out, case='dense')), flush=True)


def leg_latent(args):
    from ctypes import c_void_p
    from bayesbridge_amd import _lib
    lib = _lib.load()
    n = args.n or 1000000
    rng = np.random.default_rng(2)
    psi = 1.5 * rng.standard_normal(n)
    y = (rng.random(n) < .5).astype(np.uint8)
    shape = np.ones(n, dtype=np.int32)
    out = np.empty(n)

    def p(a):
        return a.ctypes.data_as(c_void_p)
    calls = {
        'truncated_normal': lambda: lib.bbx_device_truncated_normal(
            0, 1, n, p(psi), p(y), p(out)),
        'polya_gamma': lambda: lib.bbx_device_polya_gamma(
            0, 1, n, p(shape), p(psi), p(out)),
    }
    for name, call in calls.items():
        _lib.check(call())
        t = time.perf_counter()
        for _ in range(args.steps):
            _lib.check(call())
        dt = (time.perf_counter() - t) / args.steps
        print(json.dumps({'case': 'latent', 'sampler': name, 'n': n,
                          'ms_per_call_with_copies': 1e3 * dt}), flush=True)


LEGS = {'sparse': leg_sparse, 'dense': leg_dense, 'latent': leg_latent}


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
        print("bench_probit: the %s leg ended with status %d"
              % (args.case, status), file=sys.stderr)
    return status


if __name__ == "__main__":
    sys.exit(main())
