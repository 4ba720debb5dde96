"""Poisson model with the HMC or the NUTS coefficient sampler on the device
(rng='reference'):

    python scripts/bench_poisson.py --shapes binary:1000000x50000 \\
        dense:100000x2000 --steps 5 --warmup 2 [--sampler nuts]

For each shape: simulated counts with an exposure (demo coefficients), then
  grad_us / hvp_us    one device loglik + gradient / one Hessian matvec call
                      (host pointers, synchronous: what eigsh and the HMC
                      start see)
  leapfrog_us         one step of a 64-step device trajectory (one host wait)
  products_us         X~ v + X~^T w on device pointers, same process, same
                      stream
  ratio               leapfrog_us / products_us
  gibbs_it_s, mean_n_step, mean_dt over `steps` Gibbs iterations after
  `warmup` (gibbs_resume), from global_scale .1, unit local scales and small
  random coefficients (no mode search).
One JSON line per shape.

--sampler nuts: leapfrog_us is one step of a 64-step half-tree (one doubling
of height 6: the leaf and merge kernels included, one host wait), the Gibbs
chain draws with 'nuts' from the same seeded start, mean_n_step is the mean
number of leapfrog steps per draw, and mean_tree_height / mean_accept_prob
replace accept_rate.

--strata K | sccs: the conditional Poisson model on K strata of equal size
(K must divide n) or, with `sccs`, on strata of 2 to 8 rows as in a
self-controlled case series; the outcome is simulated with a baseline rate
exp(alpha_s), alpha_s ~ N(0, 2^2), per stratum, and the design has no
intercept column.  The output is the same.

--profile-steps N: only the trajectory (--sampler nuts: one half-tree of N
steps, N a power of two up to 1024) and N X~ v + X~^T w pairs after a short
warm-up, for a kernel trace in a run of its own.
"""
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

from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,  # noqa: E402
                             HipSparseDesignMatrix, PoissonModel,
                             RegressionCoefPrior, RegressionModel, _lib,
                             simulate)


def make_X(kind, n, p, seed):
    if kind == 'binary':
        indptr, indices = simulate.simulate_binary_csr_device(
            n, p, .002, seed=seed)
        indptr, indices = indptr.cpu().numpy(), indices.cpu().numpy()
        return sparse.csr_matrix(
            (np.ones(len(indices)), indices, indptr), shape=(n, p))
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, p), dtype=np.float32)


def products_us(design, reps):
    import torch
    n, P = design.shape
    v = torch.randn(P, dtype=torch.float64, device='cuda')
    w = torch.randn(n, dtype=torch.float64, device='cuda')
    t = torch.empty(n, dtype=torch.float64, device='cuda')
    g = torch.empty(P, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    lib = _lib.load()
    for k in range(reps + 2):
        if k == 2:
            design.synchronize()
            tic = time.perf_counter()
        _lib.check(lib.bbx_design_dot_dev(design.handle, v.data_ptr(),
                                          t.data_ptr()))
        _lib.check(lib.bbx_design_tdot_dev(design.handle, w.data_ptr(),
                                           g.data_ptr()))
    design.synchronize()
    return (time.perf_counter() - tic) / reps * 1e6


def nuts_half_tree(model, dt, height, scale, pp, q0, p0, logp0, grad0):
    """One doubling of 2^height steps from a fresh tree; the step size is
    far too small for a U-turn, so every step and every merge runs."""
    joint = -(-logp0 + 0.5 * np.dot(p0, p0))
    model.nuts_begin(scale, pp, q0, p0, logp0, grad0, joint, joint - 1., 1e300)
    uniforms = np.random.RandomState(2).rand(2 ** height)
    model.design.synchronize()
    tic = time.perf_counter()
    out = model.nuts_doubling(dt, 1, height, uniforms)
    elapsed = time.perf_counter() - tic
    assert out['n_steps'] == 2 ** height and not out['doubling_rejected'], out
    return elapsed


def stratum_sizes(strata, n, seed):
    """Row counts of the strata, stratum-major: K equal ones, or ('sccs')
    2 to 8 rows each."""
    if strata == 'sccs':
        sizes = np.random.RandomState(seed + 7).randint(2, 9, n // 2)
        sizes = sizes[:np.searchsorted(np.cumsum(sizes), n - 2, 'right')]
        rest = n - sizes.sum()                   # 2 .. 9 rows are left
        tail = [rest] if rest <= 8 else [rest // 2, rest - rest // 2]
        return np.append(sizes, tail)
    k = int(strata)
    if k < 1 or n % k or n // k < 2:
        raise SystemExit("--strata K: K must divide n into strata of 2 or "
                         "more rows")
    return np.full(k, n // k)


def run(kind, n, p, steps, warmup, seed=0, profile_steps=0, sampler='hmc',
        strata=None):
    X = make_X(kind, n, p, seed)
    # demo coefficients scaled down: a count model's mean is exp(eta)
    beta = simulate.demo_beta(p) * .25
    exposure = np.random.RandomState(seed).uniform(.5, 2., n)
    intercept = strata is None
    if strata is None:
        y = PoissonModel.simulate_outcome(X, beta, exposure=exposure,
                                          seed=seed)
        outcome = (y, exposure)
    else:
        sizes = stratum_sizes(strata, n, seed)
        label = np.repeat(np.arange(len(sizes)), sizes)
        alpha = np.random.RandomState(seed + 3).randn(len(sizes)) * 2.
        y = PoissonModel.simulate_outcome(
            X, beta, exposure=exposure * np.exp(alpha[label]), seed=seed)
        # a prebuilt design takes no stratum without a count: give each such
        # stratum one (the timing does not depend on the counts)
        empty = np.add.reduceat(y, np.cumsum(sizes) - sizes) == 0
        y[(np.cumsum(sizes) - sizes)[empty]] = 1
        outcome = (y, exposure, label)
    if kind == 'binary':
        design = HipSparseDesignMatrix(X, add_intercept=intercept,
                                       center_predictor=True)
    else:
        design = HipDenseDesignMatrix(X, add_intercept=intercept,
                                      center_predictor=True,
                                      storage_dtype='float32')
    del X
    model = RegressionModel(outcome, design, 'poisson')
    P = design.shape[1]
    rs = np.random.RandomState(1)
    b = rs.randn(P) * .01
    head = {'shape': '%s:%dx%d' % (kind, n, p), 'sampler': sampler}
    if strata is not None:
        head['strata'] = len(model.stratum_ptr) - 1
    model.compute_loglik_and_gradient(b)
    tic = time.perf_counter()
    for _ in range(10):
        model.compute_loglik_and_gradient(b)
    grad_us = (time.perf_counter() - tic) / 10 * 1e6
    op = model.get_hessian_matvec_operator(b)
    v = rs.randn(P)
    op(v)
    tic = time.perf_counter()
    for _ in range(10):
        op(v)
    hvp_us = (time.perf_counter() - tic) / 10 * 1e6
    scale, pp = np.full(P, .05), np.ones(P)
    q0, p0 = b / scale, rs.randn(P)
    ll, g = model.compute_loglik_and_gradient(q0 * scale)
    logp0 = ll - np.sum(q0 ** 2) / 2
    grad0 = scale * g - q0
    n_traj = profile_steps or 64
    if sampler == 'nuts':
        height = n_traj.bit_length() - 1
        if n_traj != 2 ** height or height > 10:
            raise SystemExit("--profile-steps must be a power of two <= "
                             "1024 with --sampler nuts")
        nuts_half_tree(model, 1e-5, 2, scale, pp, q0, p0, logp0, grad0)
        leap_us = nuts_half_tree(model, 1e-5, height, scale, pp, q0, p0,
                                 logp0, grad0) / n_traj * 1e6
    else:
        model.hmc_trajectory(1e-5, 4, scale, pp, q0, p0, logp0, grad0, 1e300)
        tic = time.perf_counter()
        tr = model.hmc_trajectory(1e-5, n_traj, scale, pp, q0, p0, logp0,
                                  grad0, 1e300)
        leap_us = (time.perf_counter() - tic) / n_traj * 1e6
        assert tr['n_steps'] == n_traj, tr
    prod_us = products_us(design, profile_steps or 50)
    if profile_steps:
        return {**head, 'profile_steps': n_traj,
                'leapfrog_us': round(leap_us, 1),
                'products_us': round(prod_us, 1)}
    head.update({'grad_us': round(grad_us, 1), 'hvp_us': round(hvp_us, 1),
                 'leapfrog_us': round(leap_us, 1),
                 'products_us': round(prod_us, 1),
                 'ratio': round(leap_us / prod_us, 3)})
    prior = RegressionCoefPrior(bridge_exponent=.25,
                                regularizing_slab_size=1.)
    bridge = BayesBridge(model, prior)
    coef = rs.randn(P) * .01
    if intercept:
        coef[0] = model.calc_intercept_mle()
    init = {'global_scale': .1, 'local_scale': np.ones(P - int(intercept)),
            'coef': coef}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, info = bridge.gibbs(warmup, init=init, seed=0,
                               coef_sampler_type=sampler)
        tic = time.perf_counter()
        _, info = bridge.gibbs_resume(info, steps)
    it_s = steps / (time.perf_counter() - tic)
    si = info['_reg_coef_sampling_info']
    if sampler == 'nuts':
        tail = {'mean_n_step': float(np.mean(si['n_grad_evals'] - 1)),
                'mean_dt': float(np.mean(si['stepsize'])),
                'mean_tree_height': float(np.mean(si['tree_height'])),
                'mean_accept_prob': float(np.mean(si['ave_accept_prob']))}
    else:
        tail = {'mean_n_step': float(np.mean(si['n_integrator_step'])),
                'mean_dt': float(np.mean(si['stepsize'])),
                'accept_rate': float(np.mean(si['accepted']))}
    return {**head, 'gibbs_it_s': round(it_s, 3), **tail}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+',
                    default=['binary:1000000x50000', 'dense:100000x2000'])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--profile-steps', type=int, default=0)
    ap.add_argument('--sampler', choices=['hmc', 'nuts'], default='hmc')
    ap.add_argument('--strata', default=None,
                    help="K equal strata, or 'sccs': strata of 2 to 8 rows")
    a = ap.parse_args()
    for s in a.shapes:
        kind, size = s.split(':')
        n, p = (int(x) for x in size.split('x'))
        print(json.dumps(run(kind, n, p, a.steps, a.warmup,
                             profile_steps=a.profile_steps,
                             sampler=a.sampler, strata=a.strata)),
              flush=True)


if __name__ == '__main__':
    main()
