"""CPU: the host side of the negative-binomial model -- the NumPy oracle
(tests/negbin_oracle.py) against central differences, its Poisson limit and
its logit identity, the slice sampler of the dispersion (dispersion.py)
against quadrature, the Gibbs driver on the oracle model, the refusals, the
declared entry points and the register / scratch use of the kernels in
csrc/negbin.hip and csrc/negbin_predict.hip."""
import math
import os
import re
import warnings

import numpy as np
import pytest

import logit_oracle as lo
import negbin_oracle as nb
from conftest import ROOT
from test_cholesky_kernel_resources import (HIPCC, _resource_table,
                                            glm_row_occupancy)

Z_BOUND = 4.5          # the long-run tests' bound on a batch-means z score


class _Design:
    """What the Gibbs driver and the option checks read of a design."""
    use_hip = True
    is_sparse = False
    intercept_added = True

    def __init__(self, n=50, P=5):
        self.shape = (n, P)


def _problem(n, p, r, seed, exposure=True):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, p) * .5
    o = np.log(rs.uniform(.5, 2., n)) if exposure else np.zeros(n)
    truth = np.concatenate(([.8], rs.randn(p) * .4))
    D = nb.design(X)
    mu = np.exp(nb.dot(D, truth) + o)
    y = rs.poisson(mu * rs.gamma(r, 1. / r, n)).astype(np.float64)
    return D, y, o, truth


def test_oracle_gradient_hessian_and_dL_dr_match_central_differences():
    D, y, o, _ = _problem(60, 5, 2., 0)
    rs = np.random.RandomState(1)
    beta, v, r = rs.randn(6) * .3, rs.randn(6), 1.7
    _, grad = nb.loglik_grad(D, y, o, beta, r)
    h = 1e-5
    num = np.array([
        (nb.loglik_grad(D, y, o, beta + h * e, r)[0]
         - nb.loglik_grad(D, y, o, beta - h * e, r)[0]) / (2 * h)
        for e in np.eye(6)])
    # O(h^2) truncation and eps / h rounding, both ~1e-10 of the values
    np.testing.assert_allclose(grad, num, rtol=1e-7, atol=1e-7)
    hv = nb.hessian_matvec(D, y, o, beta, v, r)
    num = (nb.loglik_grad(D, y, o, beta + h * v, r)[1]
           - nb.loglik_grad(D, y, o, beta - h * v, r)[1]) / (2 * h)
    np.testing.assert_allclose(hv, num, rtol=1e-7, atol=1e-7)
    # dL/dr = sum psi(y + r) - psi(r) + log r + 1 - softplus(t) - log r ...
    # written from the definition: d/dr [G + y t - (y + r) softplus(t)] with
    # dt/dr = -1 / r and d softplus = sigma
    from scipy.special import digamma
    t = nb.dot(D, beta) + o - math.log(r)
    exact = np.sum(digamma(y + r) - digamma(r) - y / r - nb.softplus(t)
                   + (y + r) * nb.sigma(t) / r)
    num = (nb.dispersion_loglik(D, y, o, beta, r + h)
           - nb.dispersion_loglik(D, y, o, beta, r - h)) / (2 * h)
    np.testing.assert_allclose(num, exact, rtol=1e-7, atol=1e-7)
    # L is the beta-part plus sum G
    np.testing.assert_allclose(
        nb.dispersion_loglik(D, y, o, beta, r),
        nb.loglik_grad(D, y, o, beta, r)[0] + float(np.sum(nb.G(y, r))),
        rtol=1e-13)
    # G against lgamma
    from scipy.special import gammaln
    np.testing.assert_allclose(nb.G(y, r).astype(np.float64),
                               gammaln(y + r) - gammaln(r), rtol=1e-12,
                               atol=1e-13)
    # f of the preconditioned coordinates: the chain rule and the prior
    scale, pp = np.exp(rs.randn(6) * .3), np.ones(6)
    f = nb.precond_f(D, y, o, scale, pp, r)
    q = rs.randn(6) * .3
    num = np.array([(f(q + h * e)[0] - f(q - h * e)[0]) / (2 * h)
                    for e in np.eye(6)])
    np.testing.assert_allclose(f(q)[1], num, rtol=1e-7, atol=1e-7)


def test_poisson_limit_of_the_weights():
    """At r = 2^40 the oracle's w differs from the Poisson oracle's y - mu by
    mu (mu - y) / (mu + r) exactly, so by at most mu |y - mu| / r per row.
    The allowance of 1e-6 of that bound is 1e-18 of w: the oracle's formulas
    are evaluated on mpmath numbers of 50 digits (tests/negbin_oracle.py
    takes them), a long double's rounding of t = eta + o - log r alone is
    2e-18."""
    import mpmath
    D, y, o, truth = _problem(200, 4, 1.5, 2)
    r = 2. ** 40
    eta_o = nb.dot(D, truth) + o
    with mpmath.workdps(50):
        mp = np.frompyfunc(mpmath.mpf, 1, 1)
        eta_mp, y_mp = mp(eta_o), mp(y)
        w = nb.row_weights(eta_mp, y_mp, mpmath.mpf(r))
        mu = nb._fn('exp', eta_mp)
        w_poisson = y_mp - mu
        diff = np.abs(w - w_poisson)
        bound = mu * np.abs(y_mp - mu) / mpmath.mpf(r)
        ratio = max(float(d / b) for d, b in zip(diff, bound) if b > 0)
        print('largest |w - w_poisson| / bound: 1 - %.3e' % (1. - ratio))
        assert all(d <= b * (1 + mpmath.mpf('1e-6'))
                   for d, b in zip(diff, bound))
        assert ratio > .999            # the bound is the difference's size
    # and in float64 the two gradients agree to the rounding of t
    _, g = nb.loglik_grad(D, y, o, truth, r)
    import poisson_oracle as po
    _, gp = po.loglik_grad(D, y, o, truth)
    np.testing.assert_allclose(g, gp, rtol=1e-9, atol=1e-9)


def test_beta_part_is_the_logit_likelihood_with_a_moved_intercept():
    """Without exposure: y t - (y + r) softplus(t) is the binomial-logit
    log-likelihood with n_success = y, n_trial = y + r at the coefficients
    with the intercept moved by -log r."""
    D, y, o, _ = _problem(80, 4, 2., 3, exposure=False)
    rs = np.random.RandomState(4)
    for r in (.05, 1., 30., 1e4):
        beta = rs.randn(5) * .4
        moved = beta.copy()
        moved[0] -= math.log(r)
        ll, grad = nb.loglik_grad(D, y, o, beta, r)
        lll, lgrad = lo.loglik_grad(D, y, y + r, moved)
        # (the intercept's subtraction rounds eta once more: 1 ulp of eta
        # times the weights' size)
        np.testing.assert_allclose(ll, lll, rtol=1e-12)
        np.testing.assert_allclose(grad, lgrad, rtol=1e-11, atol=1e-10)
        v = rs.randn(5)
        np.testing.assert_allclose(
            nb.hessian_matvec(D, y, o, beta, v, r),
            lo.hessian_matvec(D, y, y + r, moved, v), rtol=1e-11, atol=1e-10)


# ---- the slice sampler ------------------------------------------------------

def _batch_z(x, truth, n_batch=50):
    """(mean(x) - truth) / its batch-means standard error."""
    x = np.asarray(x)
    means = x[:len(x) // n_batch * n_batch].reshape(n_batch, -1).mean(axis=1)
    return (x.mean() - truth) / (means.std(ddof=1) / math.sqrt(n_batch))


class _FastL:
    """L(r) of the oracle's definition in float64 with G = lgamma(y + r) -
    lgamma(r): 20 000 slice updates evaluate it 100 000 times."""

    def __init__(self, D, y, o, beta):
        self.y, self.eta_o = y, nb.dot(D, beta) + o

    def dispersion_loglik(self, coef, r):
        from scipy.special import gammaln
        r = np.atleast_1d(r)[:, None]
        t = self.eta_o - np.log(r)
        return np.sum(gammaln(self.y + r) - gammaln(r) + self.y * t
                      - (self.y + r) * nb.softplus(t), axis=1)


def _slice_chain(jacobian, n_update=20000):
    from bayesbridge_amd import dispersion
    D, y, o, truth = _problem(40, 3, 3., 5)
    model = _FastL(D, y, o, truth)
    prior = dispersion.check_prior(None)
    # the fast L is the oracle's
    rr = np.array([.3, 2., 40.])
    np.testing.assert_allclose(model.dispersion_loglik(None, rr),
                               nb.dispersion_loglik(D, y, o, truth, rr),
                               rtol=1e-12)
    target = dispersion.log_conditional(model, truth, prior, jacobian=True)
    f = dispersion.log_conditional(model, truth, prior, jacobian=jacobian)
    rs = np.random.RandomState(6)
    theta, draws = 0., np.empty(n_update)
    for k in range(n_update):
        theta = dispersion.slice_update(theta, f, rs.random_sample)
        draws[k] = theta
    # quadrature of exp f, f with the Jacobian, on a grid that covers it
    grid = np.linspace(-6., 12., 18001)
    dens = np.concatenate([target(grid[k:k + 8])
                           for k in range(0, len(grid), 8)])
    dens = np.exp(dens - dens.max())
    assert dens[0] < 1e-12 and dens[-1] < 1e-12
    dens /= dens.sum()
    mean = np.sum(grid * dens)
    var = np.sum((grid - mean) ** 2 * dens)
    z_mean = _batch_z(draws, mean)
    z_var = _batch_z((draws - mean) ** 2, var)
    print('jacobian', jacobian, 'theta mean %.4f (quadrature %.4f) z %.2f; '
          'variance %.4f (%.4f) z %.2f'
          % (draws.mean(), mean, z_mean, np.mean((draws - mean) ** 2), var,
             z_var))
    return z_mean, z_var


def test_slice_update_leaves_the_conditional_of_log_r_invariant():
    z_mean, z_var = _slice_chain(True)
    assert abs(z_mean) < Z_BOUND and abs(z_var) < Z_BOUND


def test_slice_update_without_the_jacobian_misses_the_same_bound():
    """The negative control: the same 20 000 updates on the density without
    the Jacobian's theta are compared with the same quadrature."""
    z_mean, z_var = _slice_chain(False)
    assert abs(z_mean) > Z_BOUND


def test_slice_update_draw_order_and_stepping_out():
    from bayesbridge_amd import dispersion
    calls = []

    def f(points):
        calls.append(np.array(points))
        return -.5 * np.asarray(points) ** 2 / 25.    # N(0, 5^2): wide

    pool = [.5, .25, .35, .99, .1, .6]
    used = []

    def uniform():
        used.append(pool.pop(0))
        return used[-1]

    x = dispersion.slice_update(1., f, uniform)
    # level = f(1) + log .5, so the slice is |x| < 5.97; L = 1 - .25,
    # R = L + 1; J = floor(10 * .35) = 3 expansions to the left, 6 to the
    # right.  The left end uses its three (-2.25 is inside); the right end
    # stops at its fifth, 6.75, the first outside.
    assert np.allclose(calls[0], [1., .75, 1.75])
    assert [list(c) for c in calls[1:4]] == [
        [-.25, 2.75], [-1.25, 3.75], [-2.25, 4.75]]
    assert [list(c) for c in calls[4:6]] == [[5.75], [6.75]]
    left, right = -2.25, 6.75
    # .99 of the way is outside the slice: the interval shrinks to it
    first = left + .99 * (right - left)
    assert np.allclose(calls[6], [first]) and first > 5.97
    assert np.allclose(calls[7], [left + .1 * (first - left)])
    assert len(calls) == 8 and np.allclose(x, calls[7][0])
    assert used == [.5, .25, .35, .99, .1]
    with pytest.raises(ValueError, match='not finite'):
        dispersion.slice_update(0., lambda p: np.full(len(p), np.nan),
                                lambda: .5)
    for bad in ({'shape': 2.}, {'shape': 0., 'rate': 1.}, 3.,
                {'shape': 2., 'rate': 1., 'scale': 1.},
                {'shape': 2., 'rate': np.inf}):
        with pytest.raises(ValueError):
            dispersion.check_prior(bad)
    assert dispersion.check_prior(None) == {'shape': 2., 'rate': .1}


# ---- the Gibbs driver on the oracle model -----------------------------------

def _oracle_chain(n_iter, n_burnin, seed, method='nuts', **model_args):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    D, y, o, truth = _problem(2000, 5, 3., 7)
    model = nb.OracleModel(D, y, o, design=_Design(2000, 6), **model_args)
    prior = RegressionCoefPrior(bridge_exponent=2.,
                                _global_scale_parametrization='raw')
    start = nb.newton_mle(D, y, o, 3.)[0]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            samples, info = BayesBridge(model, prior).gibbs(
                n_iter, n_burnin=n_burnin, seed=seed, coef_sampler_type=method,
                init={'coef': start, 'global_scale': 100.},
                params_to_save='all',
                options={'global_scale_update': None})
    return samples, info, truth, model


def test_gibbs_on_the_oracle_recovers_the_dispersion_and_the_coefficients():
    """2 000 x 5, r = 3: the simulating values against the posterior.  A
    simulating value is, to the posterior, one more draw, so it lies within
    Z_BOUND of the posterior mean in units of sqrt(posterior variance + the
    mean's batch-means variance); log r for the dispersion."""
    samples, info, truth, model = _oracle_chain(700, 100, 3)
    assert set(samples) == {'coef', 'local_scale', 'global_scale', 'logp',
                            'dispersion'}
    assert samples['dispersion'].shape == (600,)
    assert info['_markov_chain_state']['dispersion'] \
        == samples['dispersion'][-1] == model.dispersion
    assert info['_markov_chain_state_raw']['dispersion'] \
        == samples['dispersion'][-1]
    assert info['init']['dispersion'] == 1.
    assert 'obs_prec' not in info['_markov_chain_state']
    series = np.vstack((samples['coef'], np.log(samples['dispersion'])))
    want = np.concatenate((truth, [math.log(3.)]))
    for x, value in zip(series, want):
        means = x.reshape(20, -1).mean(axis=1)
        mcse2 = means.var(ddof=1) / 20
        z = (value - x.mean()) / math.sqrt(x.var(ddof=1) + mcse2)
        print('truth %.4f posterior mean %.4f sd %.4f mcse %.4f z %.2f'
              % (value, x.mean(), x.std(ddof=1), math.sqrt(mcse2), z))
        assert abs(z) < Z_BOUND
    # logp: the likelihood's beta-part at the iteration's dispersion plus the
    # priors of the coefficients and of the global scale (bridge exponent 2,
    # raw scale, flat hyper-prior, no slab); neither G - log y! nor the
    # dispersion's prior is in it
    D, y, o, _ = _problem(2000, 5, 3., 7)
    sd = info['prior_sd_for_unshrunk']
    for k in (0, 299, 599):
        coef, g = samples['coef'][:, k], samples['global_scale'][k]
        want_logp = nb.loglik_grad(D, y, o, coef, samples['dispersion'][k])[0] \
            - 5 * math.log(g) - np.sum((coef[1:] / g) ** 2) \
            - .5 * np.sum((coef[:1] / sd) ** 2) \
            - np.sum(np.log(sd[sd < np.inf])) - math.log(g)
        np.testing.assert_allclose(samples['logp'][k], want_logp, rtol=1e-12)
    # the posterior has concentrated: the check above is not vacuous
    assert np.log(samples['dispersion']).std() < .15
    assert samples['coef'].std(axis=1).max() < .1


def test_fixed_dispersion_resume_and_initial_state_on_the_oracle():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    fixed, info, _, model = _oracle_chain(6, 0, 2, method='hmc',
                                          dispersion=3.)
    assert np.all(fixed['dispersion'] == 3.) and model.dispersion == 3.
    # the same seed with a sampled dispersion started at 3: the first
    # coefficient draw is the same, the chains part at the first slice update
    D, y, o, truth = _problem(2000, 5, 3., 7)
    prior = RegressionCoefPrior(bridge_exponent=2.,
                                _global_scale_parametrization='raw')
    start = nb.newton_mle(D, y, o, 3.)[0]

    def run(n_iter, model, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with np.errstate(all='ignore'):
                return BayesBridge(model, prior).gibbs(
                    n_iter, seed=2, coef_sampler_type='hmc',
                    params_to_save='all',
                    options={'global_scale_update': None}, **kw)

    init = {'coef': start, 'global_scale': 100., 'dispersion': 3.}
    model = nb.OracleModel(D, y, o, design=_Design(2000, 6))
    sampled, sinfo = run(6, model, init=init)
    assert sinfo['init']['dispersion'] == 3.
    assert np.array_equal(sampled['coef'][:, 0], fixed['coef'][:, 0])
    assert not np.array_equal(sampled['coef'][:, 1], fixed['coef'][:, 1])
    assert len(set(sampled['dispersion'])) == 6
    # resume equals a straight run
    model = nb.OracleModel(D, y, o, design=_Design(2000, 6))
    first, finfo = run(3, model, init=init)
    bridge = BayesBridge(model, prior)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            both, binfo = bridge.gibbs_resume(finfo, 3, merge=True,
                                              prev_samples=first)
    for key in sampled:
        assert np.array_equal(both[key], sampled[key]), key
    # a fixed dispersion refuses another initial value, an invalid one is
    # refused
    with pytest.raises(ValueError, match='held fixed'):
        run(2, nb.OracleModel(D, y, o, design=_Design(2000, 6),
                              dispersion=2.), init=init)
    for bad in (0., -1., np.inf, np.nan):
        with pytest.raises(ValueError):
            run(2, nb.OracleModel(D, y, o, design=_Design(2000, 6)),
                init=dict(init, dispersion=bad))


# ---- refusals ---------------------------------------------------------------

@pytest.mark.parametrize('method', [None, 'hmc', 'nuts'])
def test_negbin_takes_the_hamiltonian_samplers_on_the_reference_rng(method):
    from bayesbridge_amd import SamplerOptions
    for options in (None, {'rng': 'reference'}):
        opt = SamplerOptions.pick_default_and_create(
            method, options, 'negbin', _Design())
        assert opt.coef_sampler_type == (method or 'hmc')
        assert opt.rng == 'reference'


@pytest.mark.parametrize('method', ['cg', 'cholesky', 'woodbury'])
def test_negbin_refuses_the_gaussian_samplers_and_the_device_rng(method):
    from bayesbridge_amd import BayesBridge, SamplerOptions
    with warnings.catch_warnings():
        warnings.simplefilter('error')       # no warn-and-switch either
        with pytest.raises(ValueError, match="negative-binomial model draws "
                                             "its coefficients with 'hmc' or "
                                             "'nuts'"):
            SamplerOptions.pick_default_and_create(method, None, 'negbin',
                                                   _Design())
        with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
            SamplerOptions.pick_default_and_create(
                None, {'coef_sampler_type': method}, 'negbin', _Design())
    for ham in (None, 'hmc', 'nuts'):
        with pytest.raises(ValueError, match="rng='reference'"):
            SamplerOptions.pick_default_and_create(
                ham, {'rng': 'device'}, 'negbin', _Design())
    D, y, o, _ = _problem(50, 4, 2., 0)
    bridge = BayesBridge(nb.OracleModel(D, y, o, design=_Design(50, 5)))
    init = {'global_scale': .1}
    with pytest.raises(ValueError, match="'hmc' or 'nuts' only"):
        bridge.gibbs(2, init=init, seed=0, options=SamplerOptions(method))
    with pytest.raises(ValueError, match="'cg'"):
        bridge.gibbs_batch([0, 1], 2, init=init)
    with pytest.raises(ValueError, match="'cg' only"):
        bridge.gibbs_multichain(2, 2, init=init)


def test_outcome_and_keyword_checks():
    from bayesbridge_amd import NegBinModel, RegressionModel
    from bayesbridge_amd.design_matrix import HipDesignMatrix

    class Design(HipDesignMatrix):       # no device: the checks come first
        shape = (6, 3)

        def __init__(self):
            self._h = None

    d = Design()
    y = np.array([0, 1, 2, 0, 7, 3])
    e = np.array([1., .5, 2., 1., 3., .25])
    m = NegBinModel(y, e, d)
    assert m.name == 'negbin' and m._ham_prefix == 'bbx_negbin_'
    assert m.y.dtype == np.float64 and np.array_equal(m.y, y)
    assert np.array_equal(m.log_exposure, np.log(e))
    assert m.calc_intercept_mle() == pytest.approx(np.log(13 / 7.75))
    assert not m._negbin                  # the handle is made on first use
    assert m.dispersion == 1. and not m.dispersion_fixed
    assert m.dispersion_prior == {'shape': 2., 'rate': .1}
    m.dispersion = 2.5                    # no handle yet: kept for create
    assert m.dispersion == 2.5
    m = RegressionModel((y, e), d, 'negbin', dispersion=3.)
    assert m.dispersion == 3. and m.dispersion_fixed
    assert np.array_equal(m.exposure, e)
    m = RegressionModel(y, d, 'negbin',
                        dispersion_prior={'shape': 1., 'rate': 2.})
    assert np.array_equal(m.exposure, np.ones(6))
    assert m.dispersion_prior == {'shape': 1., 'rate': 2.}
    for bad_y in (y[:5], np.where(np.arange(6) == 2, -1, y),
                  np.where(np.arange(6) == 2, 1.5, y),
                  np.where(np.arange(6) == 2, np.nan, y), y.reshape(2, 3)):
        with pytest.raises(ValueError):
            NegBinModel(bad_y, None, d)
    for bad_e in (e[:5], np.where(np.arange(6) == 4, 0., e),
                  np.where(np.arange(6) == 4, np.inf, e)):
        with pytest.raises(ValueError):
            NegBinModel(y, bad_e, d)
    for bad_r in (0., -2., np.inf, np.nan, 'a'):
        with pytest.raises(ValueError):
            NegBinModel(y, e, d, dispersion=bad_r)
        with pytest.raises(ValueError):
            m.dispersion = bad_r
    with pytest.raises(ValueError):
        NegBinModel(y, e, d, dispersion_prior={'shape': -1., 'rate': 1.})
    with pytest.raises(ValueError, match='held fixed'):
        NegBinModel(y, e, d, dispersion=2.,
                    dispersion_prior={'shape': 1., 'rate': 1.})
    # strata are refused; the keywords belong to this family
    with pytest.raises(ValueError, match='strata are not supported'):
        RegressionModel((y, e, np.array([0, 0, 0, 1, 1, 1])), d, 'negbin')
    for family, outcome in (('linear', y * 1.), ('logit', (y > 0) * 1.),
                            ('poisson', y)):
        with pytest.raises(ValueError, match="dispersion is an argument of "
                                             "family='negbin' only"):
            RegressionModel(outcome, d, family, dispersion=2.)
        with pytest.raises(ValueError, match="dispersion_prior is an argument "
                                             "of family='negbin' only"):
            RegressionModel(outcome, d, family,
                            dispersion_prior={'shape': 1., 'rate': 1.})
    with pytest.raises(ValueError, match="entry_time is an argument"):
        RegressionModel(y, d, 'negbin', entry_time=np.zeros(6))


def test_simulated_outcome_has_the_mean_and_the_variance():
    from bayesbridge_amd import NegBinModel, simulate
    rs = np.random.RandomState(0)
    n = 200000
    X = rs.randn(n, 2) * .3
    beta, r = np.array([.4, -.2]), 2.5
    e = rs.uniform(.5, 2., n)
    y = NegBinModel.simulate_outcome(X, beta, r, exposure=e, seed=3)
    assert np.array_equal(
        y, NegBinModel.simulate_outcome(X, beta, r, exposure=e, seed=3))
    assert y.min() >= 0 and np.issubdtype(y.dtype, np.integer)
    mu = e * np.exp(X.dot(beta))
    var = mu + mu ** 2 / r
    # the mean of n counts: sd = sqrt(sum var) / n
    assert abs(y.mean() - mu.mean()) < 5 * np.sqrt(var.sum()) / n
    # sum (y - mu)^2 has mean sum var; its sd from the negative binomial's
    # fourth central moment, bounded here by the sample's own
    sq = (y - mu) ** 2
    assert abs(sq.mean() - var.mean()) < 5 * sq.std() / math.sqrt(n)
    # overdispersed: the Poisson variance is far off
    assert sq.mean() > 1.3 * mu.mean()
    y1 = simulate.simulate_outcome(X, beta, 'negbin', intercept=.2,
                                   dispersion=r, exposure=e, seed=3)
    assert abs(y1.mean() - math.exp(.2) * mu.mean()) \
        < 5 * np.sqrt((math.exp(.2) * mu + math.exp(.4) * mu ** 2 / r).sum()) / n


def test_negbin_entry_points_are_declared_bound_and_documented():
    from bayesbridge_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_negbin_\w+)\s*\(', header))
    shared = {'bbx_negbin_destroy', 'bbx_negbin_loglik_grad',
              'bbx_negbin_loglik_grad_dev', 'bbx_negbin_set_location',
              'bbx_negbin_hessian_matvec', 'bbx_negbin_hessian_matvec_dev',
              'bbx_negbin_hmc_trajectory', 'bbx_negbin_nuts_begin',
              'bbx_negbin_nuts_doubling', 'bbx_negbin_nuts_sample'}
    own = {'bbx_negbin_create', 'bbx_negbin_set_dispersion',
           'bbx_negbin_dispersion_loglik'}
    assert declared == shared | own
    predict = 'bbx_design_predictive_summary_negbin'
    assert re.search(r'\b%s\s*\(' % predict, header)
    lib = _lib.load()
    assert declared | {predict} <= set(_lib.EXPORTED_SYMBOLS)
    sigs = _lib._declare(lib)
    for name in shared:
        assert sigs[name] == sigs[name.replace('bbx_negbin_', 'bbx_logit_')]
    hp = sigs['bbx_design_destroy'][0][0]
    assert sigs['bbx_negbin_create'][0][0] is hp
    assert len(sigs['bbx_negbin_create'][0]) == 5
    assert len(sigs['bbx_negbin_dispersion_loglik'][0]) == 5
    # the family's summary: the shared one's list without family and n_trial
    shared_list = sigs['bbx_design_predictive_summary'][0]
    assert sigs[predict][0] == shared_list[:1] + shared_list[2:7] \
        + shared_list[8:]
    # new symbols and nothing else: the ABI number stays
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() == 113
    assert 'bbx_negbin_*' in header[:header.index('#define BBX_VERSION')]
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in declared | {predict}:
        assert name in doc, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '10k' in design and 'negbin.hip' in design
    # without a device the calls fail with a status, not a crash
    null = None
    assert lib.bbx_negbin_set_dispersion(null, 1.) < 0
    assert 'NULL negbin handle' in _lib.last_error()
    assert lib.bbx_negbin_dispersion_loglik(null, None, 1, None, None) < 0
    assert lib.bbx_negbin_destroy(null) == 0
    assert lib.bbx_design_predictive_summary_negbin(
        null, 1, None, None, None, None, None, 0, None, None, None, None,
        None, None) < 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_negbin_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "bayes-bridge_amd", "csrc")
    table = _resource_table(os.path.join(src, "negbin.hip"), tmp_path)
    # the three modes of the row kernel, the dispersion kernel and the
    # shared trajectory kernels
    assert sum("glm_row_kernel" in k for k in table) == 3
    assert sum("glm_cand_kernel" in k for k in table) == 1
    # no fewer waves per SIMD than negbin_row_kernel<GRAD / LOC / HESS> (114 /
    # 78 / 50 VGPRs) and negbin_disp_kernel (104 VGPRs, 16 416 B of LDS) had
    # before the folds onto glm_rows.hpp
    occupancy = glm_row_occupancy(table) + tuple(
        res["Occupancy [waves/SIMD]"] for k, res in table.items()
        if "glm_cand_kernel" in k)
    assert all(got >= was
               for got, was in zip(occupancy, (4, 6, 8, 4))), occupancy
    for k in ("cox_step1_kernel", "cox_post_a_kernel", "cox_post_b_kernel",
              "cox_finish_kernel", "cox_nuts_leaf_kernel",
              "cox_nuts_merge_a_kernel", "cox_nuts_merge_b_kernel"):
        assert any(k in name for name in table), (k, sorted(table))
    predict = _resource_table(os.path.join(src, "negbin_predict.hip"),
                              tmp_path)
    # the family's summary kernel with an outcome and without
    assert len(predict) == 2
    assert all("predict_summary_kernel" in k for k in predict)
    table.update(predict)
    for name, res in table.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= 64 * 1024, (name, res)
