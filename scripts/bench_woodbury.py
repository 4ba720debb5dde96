"""Gibbs iterations per second of the device-resident chain with the 'cg',
'cholesky' (where P <= 19 200) and 'woodbury' coefficient draws in ONE run, on
wide dense f32-stored designs (N(0, 1) entries, demo coefficients), linear and
logit, and the time and f64 TFLOP/s of the Gram kernel of the 'woodbury' draw
(wb_gram_tiles_kernel, 2 n^2 P flops over the lower tiles' mirror = n^2 P):

    python scripts/bench_woodbury.py --steps 5 --warmup 2
    python scripts/bench_woodbury.py --sizes 2000x16000 --gram-trace

Each chain starts from coef = 0 with global_scale .01 (no mode search), runs
`warmup` untimed iterations, then `steps` timed ones (gibbs_resume).  One JSON
line per (size, model, sampler).  `--gram-trace` starts a child process under
`rocprofv3 --kernel-trace --stats` that calls compute_transposed_fisher_info a
few times on each size, reads the kernel's rows from the stats CSV and prints
one JSON line per size (the host-side wall time of the call is printed too, so
that the line means something where rocprofv3 is missing).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayes-bridge_amd"))

from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,  # noqa: E402
                             RegressionCoefPrior, RegressionModel, simulate)

SIZES = ['2000x16000', '4000x16000', '1000x100000']


def make_design(n, p, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p), dtype=np.float32)
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                                  storage_dtype='float32')
    return rng, X, design


def run(n, p, steps, warmup, samplers):
    rng, X, design = make_design(n, p)
    beta = simulate.demo_beta(p)
    eta = (X @ beta.astype(np.float32)).astype(np.float64)
    outcomes = {
        'linear': eta + rng.standard_normal(n),
        'logit': (rng.binomial(1, 1 / (1 + np.exp(-eta))).astype(float),
                  np.ones(n)),
    }
    del X
    for model, y in outcomes.items():
        for sampler in samplers:
            if sampler == 'cholesky' and p + 1 > 19200:
                continue
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


def gram_child(sizes, reps):
    """Runs under rocprofv3: `reps` Gram calls per size, wall time printed."""
    for s in sizes:
        n, p = (int(v) for v in s.split('x'))
        rng, X, design = make_design(n, p)
        del X
        w = rng.gamma(2., .3, p + 1)
        design.compute_transposed_fisher_info(w)          # allocations
        design.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            design.compute_transposed_fisher_info(w)
        dt = (time.perf_counter() - t) / reps
        print(json.dumps({'gram_wall': True, 'n': n, 'P': p + 1,
                          'wall_ms_per_call_with_copy_out': 1e3 * dt}),
              flush=True)
        design.release_sampler_memory()


def gram_trace(sizes, reps):
    """One rocprofv3 run per size, so that the stats rows belong to it."""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    for s in sizes:
        n, p = (int(v) for v in s.split('x'))
        out = tempfile.mkdtemp(prefix='bbx_gram_trace_')
        cmd = [prof, '--kernel-trace', '--stats', '-d', out, '-o', 'gram',
               '--output-format', 'csv', '--', sys.executable,
               os.path.abspath(__file__), '--gram-child', '--sizes', s,
               '--reps', str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        for line in r.stdout.splitlines():
            if line.startswith('{'):
                print(line, flush=True)
        rows = []
        for path in glob.glob(os.path.join(out, '**', '*kernel_stats.csv'),
                              recursive=True):
            with open(path) as f:
                rows += [row for row in csv.DictReader(f)
                         if 'wb_gram_tiles_kernel' in row.get('Name', '')]
        if r.returncode != 0 or not rows:
            print(json.dumps({'gram_trace': False, 'n': n, 'P': p + 1,
                              'rc': r.returncode,
                              'stderr_tail': r.stderr[-300:]}), flush=True)
            continue
        calls = sum(int(row['Calls']) for row in rows)
        total_ns = sum(float(row['TotalDurationNs']) for row in rows)
        # launches per Gram: one per tile batch; time per Gram = total / (reps + 1)
        ms = total_ns / (reps + 1) / 1e6
        print(json.dumps({
            'gram_trace': True, 'n': n, 'P': p + 1, 'kernel_launches': calls,
            'gram_kernel_ms': ms,
            'f64_tflops_full_matrix': 2. * n * n * (p + 1) / (ms * 1e-3) / 1e12,
            'f64_tflops_computed_tiles':
                2. * (-(-n // 64) * (-(-n // 64) + 1) // 2) * 64 * 64 * (p + 1)
                / (ms * 1e-3) / 1e12,
        }), flush=True)
        shutil.rmtree(out, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', default=SIZES)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--samplers', nargs='+',
                    default=['cg', 'cholesky', 'woodbury'])
    ap.add_argument('--gram-trace', action='store_true')
    ap.add_argument('--gram-child', action='store_true')
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    if a.gram_child:
        gram_child(a.sizes, a.reps)
    elif a.gram_trace:
        gram_trace(a.sizes, a.reps)
    else:
        for s in a.sizes:
            n, p = (int(v) for v in s.split('x'))
            run(n, p, a.steps, a.warmup, a.samplers)
