"""Generates the fixtures of the 'nuts' coefficient sampler by importing the
upstream reference (build container only; see ref_import.py).  Data only:
inputs and the reference's outputs.  Re-run with

    python tests/golden/make_nuts_golden.py

Nothing of the reference is edited: its Gibbs loop dispatches 'nuts'
(bayesbridge.py:387-389) but its option check refuses the name
(gibbs_util.py:19,46), so the chain below hands `gibbs` a SamplerOptions
object whose sampler type is set to 'nuts' after that check has run.

Files written:
  nuts_calls.npz
      Single NoUTurnSampler.generate_next_state calls with the momentum given,
      on the Cox problems of make_cox_golden.py without tied event times (the
      chain's 100 x 50 design, dense and sparse, and the 40-row data set).
      With tied events the reference's likelihood is not the model's (see
      make_cox_golden.py): the tests check those against tests/nuts_oracle.py
      on tests/cox_oracle.py instead.  Per call: the inputs, the seed of the
      global stream, the directions, the uniforms the merges consumed, the
      number after them in the stream, and the reference's result.
      A NUTS decision is a comparison (dot < 0, uniform < weight, joint >
      threshold, max H - min H > tol).  Every call is re-run with q and p
      perturbed by 1e-12 relative, several times; it is kept only if every
      decision, the tree height and the number of uniforms are unchanged, so
      the reference itself passes what the tests demand exactly.
      `min_margin` is the smallest relative decision margin seen in the kept
      calls.
  chain_cox_nuts_sparse.npz, chain_cox_nuts_dense.npz
      the seeded chain of make_cox_golden.py (seed 0, params 'all') with
      method 'nuts', 20 iterations, and every sample_by_hmc call's info.  The
      chain is accepted only if it keeps its tree heights and step counts,
      and its coefficients to the tests' tolerance, when f's gradient is
      perturbed by 1e-12 relative.
"""
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
import make_cox_golden as mcg  # noqa: E402  (imports the reference)

warnings.simplefilter('ignore')
from bayesbridge import BayesBridge, RegressionModel, RegressionCoefPrior  # noqa
from bayesbridge.gibbs_util import SamplerOptions  # noqa: E402
import bayesbridge.reg_coef_sampler.reg_coef_sampler as rcs  # noqa: E402
from bayesbridge.reg_coef_sampler.hamiltonian_monte_carlo import nuts  # noqa

NUTS_KEYS = ('stepsize', 'tree_height', 'ave_accept_prob',
             'stability_limit_est', 'stability_adjustment_factor',
             'n_hessian_matvec', 'n_grad_evals', 'instability_detected')


class DecisionLog:
    """Records every comparison a NUTS draw makes, and its margin."""

    def __init__(self):
        self.decisions = []
        self.margin = np.inf
        T = nuts._TrajectoryTree
        self._orig = (T.__init__, T._update_sample,
                      T._check_u_turn_at_front_and_rear_ends,
                      T._merge_next_tree)

    def note(self, outcome, margin):
        self.decisions.append(bool(outcome))
        if np.isfinite(margin):
            self.margin = min(self.margin, float(margin))

    def __enter__(self):
        log, T = self, nuts._TrajectoryTree
        o_init, o_upd, o_turn, o_merge = self._orig

        def init(tree, dynamics, f, dt, q, p, logp, grad, joint, init_joint,
                 thr, tol=100., u_turn_criterion='momentum'):
            o_init(tree, dynamics, f, dt, q, p, logp, grad, joint, init_joint,
                   thr, tol, u_turn_criterion)
            log.note(joint > thr, abs(joint - thr) / max(1., abs(joint)))

        def update(tree, next_tree, method):
            state = np.random.get_state()
            u = np.random.uniform()
            np.random.set_state(state)
            if method == 'uniform':
                w = next_tree.n_acceptable_state / max(
                    1, tree.n_acceptable_state + next_tree.n_acceptable_state)
            else:
                w = next_tree.n_acceptable_state / tree.n_acceptable_state
            log.note(u < w, abs(u - w))
            log.n_uniform += 1
            return o_upd(tree, next_tree, method)

        def turn(tree):
            qf, pf, _ = tree._get_states(1)
            qr, pr, _ = tree._get_states(-1)
            dq = qf - qr
            for pp in (pf, pr):
                d = np.dot(dq, pp)
                log.note(d < 0, abs(d) / max(
                    1e-300, np.linalg.norm(dq) * np.linalg.norm(pp)))
            return o_turn(tree)

        def merge(tree, next_tree, direction, sampling_method):
            out = o_merge(tree, next_tree, direction, sampling_method)
            for t in (next_tree, tree):
                fl = t.max_hamiltonian - t.min_hamiltonian
                log.note(fl > t.hamiltonian_error_tol,
                         abs(fl - t.hamiltonian_error_tol)
                         / t.hamiltonian_error_tol)
            return out
        self.n_uniform = 0
        T.__init__, T._update_sample = init, update
        T._check_u_turn_at_front_and_rear_ends, T._merge_next_tree = \
            turn, merge
        return self

    def __exit__(self, *a):
        T = nuts._TrajectoryTree
        (T.__init__, T._update_sample,
         T._check_u_turn_at_front_and_rear_ends, T._merge_next_tree) = \
            self._orig


def problems():
    out = []
    for fmt in ('dense', 'sparse'):
        outcome, X = mcg.simulate(fmt)
        out.append(('chain_' + fmt, outcome, X))
    event, cens, X = mcg.small_data(event_ties=False)
    out.append(('small', (event, cens), X))
    return out


def one_call(f, seed, dt, q, p, max_height, tol):
    np.random.seed(seed)
    sampler = nuts.NoUTurnSampler(f, warning_requested=False)
    with DecisionLog() as log:
        q_out, info = sampler.generate_next_state(
            dt, q.copy(), p=p.copy(), max_height=max_height,
            hamiltonian_error_tol=tol)
    next_number = np.random.rand()
    np.random.seed(seed)
    exponential = np.random.exponential()
    directions = 2 * (np.random.rand(max_height) < 0.5) - 1
    uniforms = np.random.rand(log.n_uniform)
    assert np.random.rand() == next_number
    return q_out, info, log, dict(exponential=exponential,
                                  directions=directions, uniforms=uniforms,
                                  next_number=next_number)


def calls_file():
    rs = np.random.RandomState(11)
    out, kinds, min_margin, k = {}, set(), np.inf, 0
    for name, outcome, X in problems():
        model = RegressionModel(outcome, X, 'cox')
        P = X.shape[1]
        Xd = X.toarray() if sparse.issparse(X) else X
        out.update({name + '_event_time': outcome[0],
                    name + '_censoring_time': outcome[1], name + '_X': Xd})
        scale = np.exp(rs.randn(P) * .3) * .3
        prior_prec = np.ones(P)
        f = rcs.SparseRegressionCoefficientSampler \
            .get_precond_logprob_and_gradient(model, scale, prior_prec)
        out.update({name + '_scale': scale, name + '_prior_prec': prior_prec})
        # (dt, max_height, tol): short and long trees, a small max_height
        # that is reached, step sizes past the stability limit
        plans = [(.02, 3, 100.), (.05, 6, 100.), (.1, 9, 100.),
                 (.2, 9, 100.), (.3, 9, 100.), (.03, 2, 100.),
                 (.6, 9, 100.), (1.5, 9, 100.), (3., 9, 100.),
                 (.25, 9, 2.)]
        for dt, mh, tol in plans:
            for rep in range(3):
                seed = 1000 * k + rep
                q = rs.randn(P) * .1
                p = rs.randn(P)
                with np.errstate(all='ignore'):
                    q_out, info, log, rec = one_call(f, seed, dt, q, p, mh,
                                                     tol)
                    stable = True
                    for trial in range(4):
                        qq = q * (1 + 1e-12 * rs.randn(P))
                        pp = p * (1 + 1e-12 * rs.randn(P))
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
    np.savez_compressed(os.path.join(HERE, 'nuts_calls.npz'), **out)
    print('nuts_calls.npz: %d calls kept, min margin %.3g' % (k, min_margin))


class Recorder:
    def __init__(self, perturb=0.):
        self.calls, self.perturb = [], perturb
        C = rcs.SparseRegressionCoefficientSampler
        self._orig = C.sample_by_hmc
        self._orig_f = C.get_precond_logprob_and_gradient

    def __enter__(self):
        rec, C = self, rcs.SparseRegressionCoefficientSampler

        def wrapped(sampler, coef, gscale, lscale, model, **kw):
            out, info = rec._orig(sampler, coef, gscale, lscale, model, **kw)
            rec.calls.append(dict(coef_out=np.array(out), **{
                k: info[k] for k in NUTS_KEYS}))
            return out, info

        def get_f(model, scale, prec, obs_prec=None):
            f = rec._orig_f(model, scale, prec, obs_prec)
            rs = np.random.RandomState(5)

            def g(q, loglik_only=False):
                logp, grad = f(q, loglik_only=loglik_only)
                if grad is not None:
                    grad = grad * (1 + rec.perturb * rs.randn(len(grad)))
                return logp, grad
            return g if rec.perturb else f
        C.sample_by_hmc = wrapped
        C.get_precond_logprob_and_gradient = staticmethod(get_f)
        return self

    def __exit__(self, *a):
        C = rcs.SparseRegressionCoefficientSampler
        C.sample_by_hmc = self._orig
        C.get_precond_logprob_and_gradient = staticmethod(self._orig_f)


def run_chain(fmt, n_iter=20, perturb=0.):
    outcome, X = mcg.simulate(fmt)
    prior = RegressionCoefPrior(sd_for_intercept=2., regularizing_slab_size=1.,
                                bridge_exponent=.25)
    model = RegressionModel(outcome, X, 'cox')
    init = {'global_scale': 0.1, 'local_scale': np.ones(X.shape[1])}
    options = SamplerOptions('hmc')         # the reference's validation ...
    options.coef_sampler_type = 'nuts'      # ... and the name it refuses
    with Recorder(perturb) as rec:
        samples, info = BayesBridge(model, prior).gibbs(
            n_iter, 0, init=init, seed=0, params_to_save='all',
            options=options)
    return outcome, X, samples, info, rec


def chain_file(fmt):
    outcome, X, samples, info, rec = run_chain(fmt)
    _, _, s2, i2, _ = run_chain(fmt, perturb=1e-12)
    si, si2 = info['_reg_coef_sampling_info'], i2['_reg_coef_sampling_info']
    for key in ('tree_height', 'n_grad_evals', 'n_hessian_matvec'):
        assert np.array_equal(si[key], si2[key]), (fmt, key)
    # the tests' tolerance on the chain: the perturbed reference keeps it
    np.testing.assert_allclose(s2['coef'], samples['coef'], rtol=1e-6,
                               atol=1e-9)
    Xd = X.toarray() if sparse.issparse(X) else X
    out = dict(event_time=outcome[0], censoring_time=outcome[1], X=Xd,
               **{'samples_' + k: v for k, v in samples.items()},
               **{'info_' + k: np.asarray(v, dtype=np.float64)
                  for k, v in si.items()})
    for key in rec.calls[0]:
        out['nuts_' + key] = np.array([c[key] for c in rec.calls])
    np.savez_compressed(
        os.path.join(HERE, 'chain_cox_nuts_%s.npz' % fmt), **out)
    print(fmt, 'tree heights', si['tree_height'])


if __name__ == '__main__':
    calls_file()
    chain_file('sparse')
    chain_file('dense')
    print('written')
