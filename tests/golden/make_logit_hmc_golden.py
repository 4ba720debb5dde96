"""Generates the fixtures of the 'hmc' and 'nuts' coefficient samplers of the
logit model by importing the upstream reference (build container only; see
ref_import.py).  Data only: inputs and the reference's outputs.  Re-run with

    python tests/golden/make_logit_hmc_golden.py

Nothing of the reference is edited.  'hmc' is a name its option check lets
through for the logit model (gibbs_util.py:52-75); 'nuts' takes the route of
make_nuts_golden.py (a SamplerOptions object renamed after the check).

The problem: 200 rows x 30 standard-normal columns plus the intercept,
n_trial in 1..3, the prior and initial state of the Cox chain fixtures.

Files written:
  chain_logit_{hmc,nuts}_{dense,sparse}.npz
      the seeded chain (params 'all') and every sample_by_hmc call's info.
      A chain is accepted only if the reference keeps its step counts, tree
      heights and n_hessian_matvec exactly, and its coefficients to rtol 1e-6
      / atol 1e-9, when f's gradient is perturbed by 1e-12 relative: 20
      iterations with the seeds 0..119 are tried first, then 15 and 10
      iterations (`seed`, `n_iter` in the file say which was kept: 'nuts'
      seed 0 with 20 iterations, 'hmc' seed 9 with 15).
  logit_nuts_calls.npz
      single NoUTurnSampler.generate_next_state calls with the momentum given
      on the dense and the sparse problem, over the plans of
      make_nuts_golden.py; a call is kept only if its decisions survive a
      1e-12 relative perturbation of q and p.  The likelihood and its
      gradient / Hessian matvec at a few points are stored too
      (`lik_*`: the reference's values for tests/logit_oracle.py).
"""
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
import make_nuts_golden as mng  # noqa: E402  (imports the reference)
from make_nuts_golden import one_call  # noqa: E402

warnings.simplefilter('ignore')
from bayesbridge import BayesBridge, RegressionModel, RegressionCoefPrior  # noqa
from bayesbridge.gibbs_util import SamplerOptions  # noqa: E402
import bayesbridge.reg_coef_sampler.reg_coef_sampler as rcs  # noqa: E402

KEYS = {
    'hmc': ('stepsize', 'n_integrator_step', 'accepted', 'accept_prob',
            'stability_limit_est', 'stability_adjustment_factor',
            'n_hessian_matvec', 'n_grad_evals', 'instability_detected'),
    'nuts': mng.NUTS_KEYS,
}
N, P = 200, 30


def simulate(fmt):
    np.random.seed(1)
    beta_true = np.zeros(P)
    beta_true[:4] = 1
    beta_true[4:15] = 2 ** - np.linspace(0.0, 5, 11)
    X = np.random.randn(N, P)
    n_trial = np.random.randint(1, 4, N).astype(np.float64)
    prob = 1 / (1 + np.exp(-(X.dot(beta_true) - .5)))
    n_success = np.random.binomial(n_trial.astype(int), prob).astype(
        np.float64)
    if fmt == 'sparse':
        X = sparse.csr_matrix(X)
    return (n_success, n_trial), X


class Recorder(mng.Recorder):
    """make_nuts_golden.Recorder keeping the info keys of `method`."""

    def __init__(self, method, perturb=0.):
        super().__init__(perturb)
        self.keys = KEYS[method]

    def __enter__(self):
        super().__enter__()
        rec, C = self, rcs.SparseRegressionCoefficientSampler

        def wrapped(sampler, coef, gscale, lscale, model, **kw):
            out, info = rec._orig(sampler, coef, gscale, lscale, model, **kw)
            rec.calls.append(dict(coef_out=np.array(out), **{
                k: info[k] for k in rec.keys}))
            return out, info
        C.sample_by_hmc = wrapped
        return self


def run_chain(method, fmt, seed=0, n_iter=20, perturb=0.):
    outcome, X = simulate(fmt)
    prior = RegressionCoefPrior(sd_for_intercept=2., regularizing_slab_size=1.,
                                bridge_exponent=.25)
    model = RegressionModel(outcome, X, 'logit')
    init = {'global_scale': 0.1, 'local_scale': np.ones(X.shape[1])}
    options = SamplerOptions('hmc')
    options.coef_sampler_type = method
    with Recorder(method, perturb) as rec:
        samples, info = BayesBridge(model, prior).gibbs(
            n_iter, 0, init=init, seed=seed, params_to_save='all',
            options=options)
    return outcome, X, samples, info, rec


def stable_chain(method, fmt):
    """The first chain that the reference itself reproduces under a 1e-12
    relative perturbation of f's gradient: 20 iterations with the seeds
    0..119, then 15, then 10.  (The logit 'hmc' chain multiplies a
    perturbation by 10-300 per iteration -- the ARPACK estimate at tol=.1 sets
    the step size, and a trajectory runs for a quarter period or more: none of
    the 120 seeds keeps 20 iterations to rtol 1e-6; 'nuts' keeps every one.)"""
    steps = 'n_integrator_step' if method == 'hmc' else 'tree_height'
    candidates = [(sd, n) for n in (20, 15, 10) for sd in range(120)]
    for seed, n_iter in candidates:
        outcome, X, samples, info, rec = run_chain(method, fmt, seed, n_iter)
        _, _, s2, i2, _ = run_chain(method, fmt, seed, n_iter, perturb=1e-12)
        si = info['_reg_coef_sampling_info']
        si2 = i2['_reg_coef_sampling_info']
        kept = all(np.array_equal(si[key], si2[key])
                   for key in (steps, 'n_grad_evals', 'n_hessian_matvec')) \
            and np.allclose(s2['coef'], samples['coef'], rtol=1e-6, atol=1e-9)
        if kept:
            print(method, fmt, 'seed', seed, 'n_iter', n_iter, 'kept')
            return seed, n_iter, outcome, X, samples, si, rec
    raise AssertionError((method, fmt))


def chain_file(method, fmt):
    seed, n_iter, outcome, X, samples, si, rec = stable_chain(method, fmt)
    steps = 'n_integrator_step' if method == 'hmc' else 'tree_height'
    Xd = X.toarray() if sparse.issparse(X) else X
    out = dict(n_success=outcome[0], n_trial=outcome[1], X=Xd, seed=seed,
               n_iter=n_iter,
               **{'samples_' + k: v for k, v in samples.items()},
               **{'info_' + k: np.asarray(v, dtype=np.float64)
                  for k, v in si.items()})
    for key in rec.calls[0]:
        out['call_' + key] = np.array([c[key] for c in rec.calls])
    np.savez_compressed(
        os.path.join(HERE, 'chain_logit_%s_%s.npz' % (method, fmt)), **out)
    print(method, fmt, steps, si[steps], 'n_hessian_matvec',
          si['n_hessian_matvec'])


def calls_file():
    rs = np.random.RandomState(11)
    out, kinds, min_margin, k = {}, set(), np.inf, 0
    for fmt in ('dense', 'sparse'):
        name = 'chain_' + fmt
        outcome, X = simulate(fmt)
        model = RegressionModel(outcome, X, 'logit')
        P1 = P + 1
        Xd = X.toarray() if sparse.issparse(X) else X
        out.update({name + '_n_success': outcome[0],
                    name + '_n_trial': outcome[1], name + '_X': Xd})
        scale = np.exp(rs.randn(P1) * .3) * .3
        prior_prec = np.ones(P1)
        f = rcs.SparseRegressionCoefficientSampler \
            .get_precond_logprob_and_gradient(model, scale, prior_prec)
        out.update({name + '_scale': scale, name + '_prior_prec': prior_prec})
        # the reference's likelihood at a few points, |eta| up to ~700
        for j, size in enumerate((.1, 1., 25.)):
            beta, v = rs.randn(P1) * size, rs.randn(P1)
            ll, grad = model.compute_loglik_and_gradient(beta)
            hv = model.get_hessian_matvec_operator(beta)(v)
            out.update({'lik_%s_%d_%s' % (fmt, j, key): val for key, val in (
                ('beta', beta), ('v', v), ('loglik', ll), ('grad', grad),
                ('hv', hv))})
        plans = [(.02, 3, 100.), (.05, 6, 100.), (.1, 9, 100.),
                 (.2, 9, 100.), (.3, 9, 100.), (.03, 2, 100.),
                 (.6, 9, 100.), (1.5, 9, 100.), (3., 9, 100.),
                 (.25, 9, 2.)]
        for dt, mh, tol in plans:
            for rep in range(3):
                seed = 1000 * k + rep
                q = rs.randn(P1) * .1
                p = rs.randn(P1)
                with np.errstate(all='ignore'):
                    q_out, info, log, rec = one_call(f, seed, dt, q, p, mh,
                                                     tol)
                    stable = True
                    for trial in range(4):
                        qq = q * (1 + 1e-12 * rs.randn(P1))
                        pp = p * (1 + 1e-12 * rs.randn(P1))
                        _, i2, l2, _ = one_call(f, seed, dt, qq, pp, mh, tol)
                        stable &= (l2.decisions == log.decisions
                                   and l2.n_uniform == log.n_uniform
                                   and i2['tree_height']
                                   == info['tree_height']
                                   and i2['n_grad_evals']
                                   == info['n_grad_evals'])
                if not stable or not np.isfinite(info['logp']):
                    continue
                maxed = info['tree_height'] >= mh \
                    and not info['u_turn_detected']
                kinds.add(('u_turn_inside', info['u_turn_detected']
                           and info['last_doubling_rejected']))
                kinds.add(('u_turn_top', info['u_turn_detected']
                           and not info['last_doubling_rejected']))
                kinds.add(('maxed', maxed))
                kinds.add(('instability', info['instability_detected']))
                min_margin = min(min_margin, log.margin)
                pre = 'call%03d_' % k
                out.update({
                    pre + 'problem': name, pre + 'seed': seed, pre + 'dt': dt,
                    pre + 'max_height': mh, pre + 'tol': tol, pre + 'q': q,
                    pre + 'p': p, pre + 'q_out': q_out,
                    pre + 'logp': info['logp'], pre + 'grad': info['grad'],
                    pre + 'n_uniform': log.n_uniform,
                    **{pre + key: rec[key] for key in rec},
                    **{pre + key: info[key] for key in (
                        'tree_height', 'n_grad_evals', 'u_turn_detected',
                        'instability_detected', 'last_doubling_rejected',
                        'ave_accept_prob', 'ave_hamiltonian_error')}})
                k += 1
    for kind in ('u_turn_inside', 'u_turn_top', 'maxed', 'instability'):
        assert (kind, True) in kinds, kind
    out['n_call'] = k
    out['min_margin'] = min_margin
    np.savez_compressed(os.path.join(HERE, 'logit_nuts_calls.npz'), **out)
    print('logit_nuts_calls.npz: %d calls kept, min margin %.3g'
          % (k, min_margin))


if __name__ == '__main__':
    if '--chains-only' not in sys.argv:
        calls_file()
    for method in ('hmc', 'nuts'):
        for fmt in ('sparse', 'dense'):
            chain_file(method, fmt)
    print('written')
