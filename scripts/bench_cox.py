"""Cox model with the HMC or the NUTS coefficient sampler on the device:

    python scripts/bench_cox.py --shapes binary:1000000x50000 dense:100000x2000 \
        --steps 5 --warmup 2 [--sampler nuts]

For each shape: a simulated Cox outcome (cox_model.py:275-298, demo
coefficients, 90 % censored), then
  preprocess_s        sorting, dropping uninformative rows, risk-set indices
  grad_us / hvp_us    one loglik + gradient / one Hessian matvec call (host
                      pointers, synchronous: what eigsh and the HMC start see)
  leapfrog_us         one step of a 64-step device trajectory (one host wait)
  products_us         X~ v + X~^T w on device pointers, same run, same stream
  ratio               leapfrog_us / products_us
  gibbs_it_s, mean_n_step, mean_dt over `steps` Gibbs iterations after
  `warmup` (gibbs_resume), from global_scale .1, unit local scales and
  small random coefficients (no mode search).
One JSON line per shape.

--sampler nuts: leapfrog_us is one step of a 64-step half-tree (one doubling
of height 6: the leaf and merge kernels included, one host wait), the Gibbs
chain draws with 'nuts' from the same seeded start, mean_n_step is the mean
number of leapfrog steps per draw, and mean_tree_height / mean_accept_prob
replace accept_rate.  --profile-steps N then runs one half-tree of N steps
(N a power of two up to 1024).

--profile-steps N: only the trajectory and the products, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -o cox -- \
        python scripts/bench_cox.py --shapes binary:1000000x50000 \
        --profile-steps 200

runs one N-step trajectory and N X~ v + X~^T w pairs (after a 4-step warm-up
trajectory); the design's product kernels then run 2N (+ a few) times, every
Cox kernel N (+ a few) times, so per step: product kernels = their total / 2N,
the Cox kernels = their total / N.

--strata K: the stratified model (csrc/cox_strat.hpp) on K strata of equal
expected size (labels drawn uniformly), the same outcome otherwise.
--strata pairs: n / 2 matched pairs -- rows 2j and 2j + 1 form a stratum, the
one with the earlier simulated event time is the event, the other is censored
at its own later time, so no row is dropped.  Every figure above is then that
of the stratified handle; `n_strata` is added to the JSON line.

--entry FRAC: the counting-process model (csrc/cox_interval.hip): a fraction
FRAC of the rows gets an entry time drawn uniformly below its exit time, the
others are at risk from the start; the same outcome otherwise.  Every figure
above is then that of the bbx_coxcp handle; `entry_frac` and `n_delayed` (rows
with a finite entry time after preprocessing) are added to the JSON line.
--entry 0 runs that handle without delayed entry.  Not together with --strata.

--ties efron | breslow: the simulated times are rounded up to a grid of
--grid points (default 3650: ten years of days) over the span of the observed
times, so that events tie, and `mean_tie_group` (the mean over the events of
the size of their tie group) and `n_tie_group` are added to the JSON line.
efron: every figure above is that of the bbx_coxef handle
(csrc/cox_efron.hip), and `plain_leapfrog_us` is the same trajectory on the
plain handle (Breslow's rule) on the same design and rows, from the same
library.  breslow: the plain handle on the gridded times.  With
--profile-steps only the chosen handle runs, so that a kernel trace holds one
handle's kernels: trace each in a run of its own.  Not together with --strata
or --entry.

--weights iptw: the weighted model (csrc/cox_weighted.hip) with stabilised
inverse-probability-of-treatment weights: a treatment is drawn for every row
from a simulated propensity e_i = expit(x_i . gamma - c) (gamma on the first
five columns, c set so that the mean propensity is about 0.3), and a_i =
P(z = z_i) / P(z = z_i | x_i).  `weight_min`, `weight_max` and `weight_mean`
are added to the JSON line.  Every figure above is then that of the bbx_coxw
handle, and `plain_leapfrog_us` is the same trajectory on the plain handle
(no weights) on the same design and rows, from the same library, in the same
process -- with --profile-steps too: in a kernel trace the two handles' own
kernels differ in their policy argument (cox_risk_sum_kernel<CoxWeighted, ..>
against cox_risk_sum_kernel<CoxPlain, ..>, and so on for cox_event_sum_kernel
and cox_row_weight_kernel), and cox_max_kernel and cox_scan_out_kernel are the
same code on the same sizes in both, so their per-call average is either
handle's.
Not together with --strata, --entry or --ties.

--competing FRAC: the Fine-Gray competing-risks model (csrc/cox_finegray.hip):
a fraction FRAC of the censored rows is recoded as competing events at their
censoring times; the same outcome otherwise.  `competing_frac`, `n_competing`
and `n_censored` (after preprocessing) are added to the JSON line.  Every
figure above is then that of the bbx_coxfg handle, and `plain_leapfrog_us` is
the same trajectory on the plain handle that censors at the competing event,
on the same rows (in its own row order, so on a second design), from the same
library, in the same process -- with --profile-steps too: in a kernel trace
the two handles' own kernels differ in their policy argument (CoxFineGray
against CoxPlain).  `launches` and `plain_launches` count the kernel launches
of one loglik + gradient call of either handle.
Not together with --strata, --entry, --ties or --weights.

--predict S: prediction instead of sampling, on the handle the
other options select: `hazard_us_per_draw`, the wall time per draw of one
S-draw cumulative_baseline_hazard call on a 257-point grid (one host
synchronisation for all the draws), against `loglik_only_us`, one synchronous
loglik-only evaluation of the same handle in the same process (mean of 10);
the launches of either per draw; `residuals_us`, one martingale_residuals
call; `survival_ms`, three bbx_cox_survival_summary calls of 100 000 rows x 10
times x 256 draws from host memory, uploads and read-back included, with the
bytes in and out.  Not together with --strata.
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
                             HipSparseDesignMatrix, RegressionCoefPrior,
                             RegressionModel, _lib, simulate)
from bayesbridge_amd.model import (CoxModel, cox_preprocess,  # noqa: E402
                                   cox_preprocess_finegray,
                                   cox_preprocess_interval,
                                   cox_preprocess_stratified, cox_tie_groups)


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


def strata_outcome(X, beta, strata, seed):
    """(event_time, censoring_time, labels) of --strata."""
    n = X.shape[0]
    if strata != 'pairs':
        et, ct = CoxModel.simulate_outcome(X, beta, seed=seed)
        labels = np.random.RandomState(seed + 1).randint(0, int(strata), n)
        return et, ct, labels
    eta = np.asarray(X.dot(beta), dtype=np.float64).ravel()
    time_ = np.random.RandomState(seed).exponential(np.exp(eta.max() - eta))
    m = n - n % 2                  # an odd last row: a stratum of one event
    t = time_[:m].reshape(-1, 2)
    first = t[:, 0] <= t[:, 1]
    event = np.column_stack((first, ~first))
    et = np.append(np.where(event, t, np.inf).ravel(), time_[m:])
    ct = np.append(np.where(event, np.inf, t).ravel(), np.full(n - m, np.inf))
    return et, ct, np.arange(n) // 2


def entry_times(et, ct, frac, seed):
    """Entry times of --entry: uniform on (0, exit) for a fraction of the
    rows, -inf for the others."""
    rs = np.random.RandomState(seed + 2)
    x = np.minimum(et, ct)
    entry = np.where(rs.rand(len(x)) < frac, x * rs.rand(len(x)), -np.inf)
    return np.where(entry < x, entry, -np.inf)


def on_grid(et, ct, n_grid):
    """Both times rounded up to a grid of n_grid points over the span of the
    observed times (inf stays inf)."""
    step = np.max(np.minimum(et, ct)) / n_grid
    with np.errstate(invalid='ignore'):
        return np.ceil(et / step) * step, np.ceil(ct / step) * step


def iptw_weights(X, seed):
    """Stabilised inverse-probability-of-treatment weights of --weights."""
    rs = np.random.RandomState(seed + 3)
    k = min(5, X.shape[1])
    gamma = rs.randn(k)
    score = np.asarray(X[:, :k].dot(gamma), dtype=np.float64).ravel()
    score = (score - score.mean()) / (score.std() or 1.)
    e = 1. / (1. + np.exp(-(score + np.log(.3 / .7))))
    z = rs.rand(len(e)) < e
    return np.where(z, z.mean() / e, (1. - z.mean()) / (1. - e))


def competing_times(ct, frac, seed):
    """(censoring, competing) times of --competing: a fraction of the censored
    rows becomes competing events at the same times."""
    recode = np.isfinite(ct) & (np.random.RandomState(seed + 4).rand(len(ct))
                                < frac)
    return np.where(recode, np.inf, ct), np.where(recode, ct, np.inf)


def launches(model, beta):
    """Kernel launches of one loglik + gradient call."""
    from ctypes import c_uint64
    lib = _lib.load()
    lib.bbx_launch_count.restype = c_uint64
    before = lib.bbx_launch_count()
    model.compute_loglik_and_gradient(beta)
    return int(lib.bbx_launch_count() - before)


def make_design(kind, X):
    if kind == 'binary':
        return HipSparseDesignMatrix(X, add_intercept=False,
                                     center_predictor=True)
    return HipDenseDesignMatrix(X, add_intercept=False, center_predictor=True,
                                storage_dtype='float32')


def leapfrog_us(model, n_traj, scale, pp, q0, p0, logp0, grad0):
    model.hmc_trajectory(1e-3, 4, scale, pp, q0, p0, logp0, grad0, 1e300)
    tic = time.perf_counter()
    tr = model.hmc_trajectory(1e-3, n_traj, scale, pp, q0, p0, logp0, grad0,
                              1e300)
    assert tr['n_steps'] == n_traj
    return (time.perf_counter() - tic) / n_traj * 1e6


def predict_figures(model, n_draw, n_grid=257, seed=0):
    """--predict: one n_draw-draw baseline-hazard call against the synchronous
    loglik-only evaluation of the same handle, and the survival summary of
    100 000 rows x 10 times x 256 draws."""
    from ctypes import c_uint64, c_void_p
    lib = _lib.load()
    lib.bbx_launch_count.restype = c_uint64
    P = model.n_pred
    rs = np.random.RandomState(seed + 5)
    coef = rs.randn(P, n_draw) * .01
    ev = model.event_time[np.isfinite(model.event_time)]
    grid = np.sort(rs.uniform(ev.min(), ev.max(), n_grid))
    b = np.ascontiguousarray(coef[:, 0])
    model.compute_loglik_and_gradient(b, loglik_only=True)
    before = lib.bbx_launch_count()
    tic = time.perf_counter()
    for _ in range(10):
        model.compute_loglik_and_gradient(b, loglik_only=True)
    loglik_us = (time.perf_counter() - tic) / 10 * 1e6
    loglik_launches = int(lib.bbx_launch_count() - before) // 10
    model.cumulative_baseline_hazard(coef[:, :2], grid)
    before = lib.bbx_launch_count()
    tic = time.perf_counter()
    model.cumulative_baseline_hazard(coef, grid, log=True)
    hazard_us = (time.perf_counter() - tic) / n_draw * 1e6
    hazard_launches = int(lib.bbx_launch_count() - before) / n_draw
    tic = time.perf_counter()
    model.martingale_residuals(b)
    resid_us = (time.perf_counter() - tic) * 1e6
    n_row, n_time, n_d = 100000, 10, 256
    eta = np.ascontiguousarray(rs.randn(n_d, n_row))
    lh = np.ascontiguousarray(np.sort(rs.randn(n_d, 1, n_time), axis=2) - 1.)
    mean, sd = np.empty((n_row, n_time)), np.empty((n_row, n_time))

    def ptr(a):
        return a.ctypes.data_as(c_void_p)

    surv_ms = []
    for _ in range(3):
        tic = time.perf_counter()
        _lib.check(lib.bbx_cox_survival_summary(
            model.design.device, n_row, n_time, n_d, 1, ptr(eta), ptr(lh),
            None, ptr(mean), ptr(sd), None))
        surv_ms.append((time.perf_counter() - tic) * 1e3)
    return {'predict_draws': n_draw, 'n_grid': n_grid,
            'hazard_us_per_draw': round(hazard_us, 1),
            'loglik_only_us': round(loglik_us, 1),
            'hazard_launches_per_draw': hazard_launches,
            'loglik_only_launches': loglik_launches,
            'residuals_us': round(resid_us, 1),
            'survival_ms': [round(x, 2) for x in surv_ms],
            'survival_shape': [n_row, n_time, n_d],
            'survival_bytes_in': eta.nbytes + lh.nbytes,
            'survival_bytes_out': mean.nbytes + sd.nbytes}


def run(kind, n, p, steps, warmup, seed=0, profile_steps=0, sampler='hmc',
        strata=None, entry=None, ties=None, n_grid=3650, weights=None,
        competing=None, predict=0):
    X = make_X(kind, n, p, seed)
    beta = simulate.demo_beta(p)
    labels = None
    if strata is None:
        et, ct = CoxModel.simulate_outcome(X, beta, seed=seed)
    else:
        et, ct, labels = strata_outcome(X, beta, strata, seed)
    if ties is not None:
        et, ct = on_grid(et, ct, n_grid)
    entry_time = None
    if weights is not None:
        weights = iptw_weights(X, seed)
    comp = plain_outcome = plain_design = None
    if competing is not None:
        ct, comp = competing_times(ct, competing, seed)
    tic = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if comp is not None:
            et, ct, comp, X, _, _, _ = cox_preprocess_finegray(et, ct, comp, X)
        elif entry is not None:
            entry_time, et, ct, X, _ = cox_preprocess_interval(
                entry_times(et, ct, entry, seed), et, ct, X)
        elif labels is None:
            et, ct, X, keep = cox_preprocess(et, ct, X)
            if weights is not None:
                weights = weights[keep]
        else:
            et, ct, labels, X, _ = cox_preprocess_stratified(et, ct, labels, X)
    design = make_design(kind, X)
    t_design = time.perf_counter() - tic
    if comp is not None:
        # the plain handle censors at the competing event; its own row order
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            pet, pct, Xp, _ = cox_preprocess(et, np.minimum(ct, comp), X)
        plain_outcome, plain_design = (pet, pct), make_design(kind, Xp)
        del Xp
    del X
    tic = time.perf_counter()
    outcome = (et, ct) if labels is None else (et, ct, labels)
    model = RegressionModel(outcome, design, 'cox', entry_time=entry_time,
                            ties=ties or 'breslow', weights=weights,
                            competing_time=comp)
    n_strata = {} if labels is None else {
        'n_strata': len(model.stratum_n_event)}
    if entry is not None:
        n_strata = {'entry_frac': entry,
                    'n_delayed': int(np.isfinite(entry_time).sum())}
    if ties is not None:
        gstart, gsize = cox_tie_groups(et)
        n_strata = {'ties': ties, 'mean_tie_group': round(gsize.mean(), 1),
                    'n_tie_group': len(np.unique(gstart))}
    if weights is not None:
        n_strata = {'weights': 'iptw',
                    'weight_min': float('%.4g' % weights.min()),
                    'weight_max': float('%.4g' % weights.max()),
                    'weight_mean': float('%.4g' % weights.mean())}
    if comp is not None:
        n_strata = {'competing_frac': competing,
                    'n_competing': int(np.isfinite(comp).sum()),
                    'n_censored': int(np.isfinite(ct).sum())}
    preprocess_s = t_design + time.perf_counter() - tic
    if predict:
        return {'shape': '%s:%dx%d' % (kind, n, p), 'n_event': model.n_event,
                **n_strata, **predict_figures(model, predict, seed=seed)}
    P = design.shape[1]
    rs = np.random.RandomState(1)
    b = rs.randn(P) * .01
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
            raise SystemExit("--profile-steps must be a power of two <= 1024 "
                             "with --sampler nuts")
        nuts_half_tree(model, 1e-3, 2, scale, pp, q0, p0, logp0, grad0)
        leap_us = nuts_half_tree(model, 1e-3, height, scale, pp, q0, p0,
                                 logp0, grad0) / n_traj * 1e6
    else:
        leap_us = leapfrog_us(model, n_traj, scale, pp, q0, p0, logp0, grad0)
        if (ties == 'efron' and not profile_steps) or weights is not None:
            # the plain handle on the same design and rows: its own f(q0)
            plain = RegressionModel(outcome, design, 'cox')
            pll, pg = plain.compute_loglik_and_gradient(q0 * scale)
            n_strata['plain_leapfrog_us'] = round(leapfrog_us(
                plain, n_traj, scale, pp, q0, p0, pll - np.sum(q0 ** 2) / 2,
                scale * pg - q0), 1)
            del plain
        if comp is not None:
            plain = RegressionModel(plain_outcome, plain_design, 'cox')
            pll, pg = plain.compute_loglik_and_gradient(q0 * scale)
            n_strata['plain_leapfrog_us'] = round(leapfrog_us(
                plain, n_traj, scale, pp, q0, p0, pll - np.sum(q0 ** 2) / 2,
                scale * pg - q0), 1)
            n_strata['launches'] = launches(model, b)
            n_strata['plain_launches'] = launches(plain, b)
            del plain
    prod_us = products_us(design, profile_steps or 50)
    if profile_steps:
        return {'shape': '%s:%dx%d' % (kind, n, p), 'sampler': sampler,
                'profile_steps': n_traj, **n_strata,
                'leapfrog_us': round(leap_us, 1),
                'products_us': round(prod_us, 1)}
    prior = RegressionCoefPrior(bridge_exponent=.25,
                                regularizing_slab_size=1.)
    bridge = BayesBridge(model, prior)
    init = {'global_scale': .1, 'local_scale': np.ones(P),
            'coef': rs.randn(P) * .01}
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
    return {'shape': '%s:%dx%d' % (kind, n, p), 'sampler': sampler,
            'n_event': model.n_event, **n_strata,
            'preprocess_s': round(preprocess_s, 2),
            'grad_us': round(grad_us, 1), 'hvp_us': round(hvp_us, 1),
            'leapfrog_us': round(leap_us, 1),
            'products_us': round(prod_us, 1),
            'ratio': round(leap_us / prod_us, 3),
            'gibbs_it_s': round(it_s, 3), **tail}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+',
                    default=['binary:1000000x50000', 'dense:100000x2000'])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--profile-steps', type=int, default=0)
    ap.add_argument('--sampler', choices=['hmc', 'nuts'], default='hmc')
    ap.add_argument('--strata', default=None,
                    help="a number of strata, or 'pairs'")
    ap.add_argument('--entry', type=float, default=None, metavar='FRAC',
                    help="the counting-process model; the fraction of rows "
                         "with a delayed entry time")
    ap.add_argument('--ties', choices=['breslow', 'efron'], default=None,
                    help="times on a grid, tied events by this rule")
    ap.add_argument('--weights', choices=['iptw'], default=None,
                    help="the weighted model, stabilised IPT weights")
    ap.add_argument('--competing', type=float, default=None, metavar='FRAC',
                    help="the Fine-Gray model; the fraction of the censored "
                         "rows recoded as competing events")
    ap.add_argument('--predict', type=int, default=0, metavar='S',
                    help="prediction instead of sampling: one S-draw "
                         "baseline-hazard call against a loglik-only "
                         "evaluation, and the survival summary")
    ap.add_argument('--grid', type=int, default=3650, metavar='N',
                    help="grid points of --ties")
    a = ap.parse_args()
    if a.ties is not None and (a.strata is not None or a.entry is not None):
        raise SystemExit("--ties does not combine with --strata or --entry")
    if a.weights is not None and (a.strata is not None or a.entry is not None
                                  or a.ties is not None):
        raise SystemExit("--weights does not combine with --strata, --entry "
                         "or --ties")
    if a.competing is not None and (
            a.strata is not None or a.entry is not None or a.ties is not None
            or a.weights is not None):
        raise SystemExit("--competing does not combine with --strata, "
                         "--entry, --ties or --weights")
    if a.competing is not None and not 0. <= a.competing <= 1.:
        raise SystemExit("--competing takes a fraction in [0, 1]")
    if a.predict < 0 or (a.predict and a.strata is not None):
        raise SystemExit("--predict takes a number of draws and does not "
                         "combine with --strata")
    if a.grid < 1:
        raise SystemExit("--grid takes a positive number")
    if a.strata not in (None, 'pairs') and int(a.strata) < 1:
        raise SystemExit("--strata takes a positive number or 'pairs'")
    if a.entry is not None and not 0. <= a.entry <= 1.:
        raise SystemExit("--entry takes a fraction in [0, 1]")
    if a.entry is not None and a.strata is not None:
        raise SystemExit("--entry and --strata do not combine")
    for s in a.shapes:
        kind, size = s.split(':')
        n, p = (int(x) for x in size.split('x'))
        print(json.dumps(run(kind, n, p, a.steps, a.warmup,
                             profile_steps=a.profile_steps,
                             sampler=a.sampler, strata=a.strata,
                             entry=a.entry, ties=a.ties,
                             n_grid=a.grid, weights=a.weights,
                             competing=a.competing, predict=a.predict)),
              flush=True)


if __name__ == '__main__':
    main()
