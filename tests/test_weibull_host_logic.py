"""CPU: the host side of the Weibull model -- the NumPy oracle
(tests/weibull_oracle.py) against central differences and against mpmath, its
exponential (Poisson) identity, the slice update of the shape
(weibull_shape.py) against quadrature, the Gibbs driver on the oracle model,
the refusals, the simulated outcome, the declared entry points and the
register / scratch use of the kernels in csrc/weibull.hip and
csrc/weibull_predict.hip."""
import inspect
import math
import os
import re
import warnings

import numpy as np
import pytest

import poisson_oracle as po
import weibull_oracle as wb
from conftest import ROOT
from test_cholesky_kernel_resources import (HIPCC, _resource_table,
                                            glm_row_occupancy)

Z_BOUND = 4.5          # the slice tests' bound on a batch-means z score
LD = np.longdouble


class _Design:
    """What the Gibbs driver and the option checks read of a design."""
    use_hip = True
    is_sparse = False
    intercept_added = True

    def __init__(self, n=50, P=5):
        self.shape = (n, P)


def _problem(n, p, k, seed, censoring_frac=.4):
    from bayesbridge_amd import WeibullModel
    rs = np.random.RandomState(seed)
    X = rs.randn(n, p) * .5
    truth = np.concatenate(([-.3], rs.randn(p) * .4))
    D = wb.design(X)
    eta = wb.dot(D, truth)
    et, ct = WeibullModel._simulate_from_eta(eta, k, censoring_frac,
                                             seed + 1000)
    d = np.isfinite(et).astype(np.float64)
    lt = np.log(np.minimum(et, ct))
    return D, d, lt, truth


def test_oracle_gradient_hessian_and_dL_dk_match_central_differences():
    D, d, lt, _ = _problem(60, 5, 1.6, 0)
    rs = np.random.RandomState(1)
    beta, v, k = rs.randn(6) * .3, rs.randn(6), 1.7
    _, grad = wb.loglik_grad(D, d, lt, beta, k)
    h = 1e-5
    num = np.array([
        (wb.loglik_grad(D, d, lt, beta + h * e, k)[0]
         - wb.loglik_grad(D, d, lt, beta - h * e, k)[0]) / (2 * h)
        for e in np.eye(6)])
    # O(h^2) truncation and eps / h rounding, both ~1e-10 of the values
    np.testing.assert_allclose(grad, num, rtol=1e-7, atol=1e-7)
    hv = wb.hessian_matvec(D, d, lt, beta, v, k)
    num = (wb.loglik_grad(D, d, lt, beta + h * v, k)[1]
           - wb.loglik_grad(D, d, lt, beta - h * v, k)[1]) / (2 * h)
    np.testing.assert_allclose(hv, num, rtol=1e-7, atol=1e-7)
    # dL/dk = sum d (1 / k + lt) - lt exp(eta + k lt)
    eta = wb.dot(D, beta)
    exact = np.sum(d * (1. / k + lt) - lt * np.exp(eta + k * lt))
    num = (wb.shape_loglik(D, d, lt, beta, k + h)
           - wb.shape_loglik(D, d, lt, beta, k - h)) / (2 * h)
    np.testing.assert_allclose(num, exact, rtol=1e-7, atol=1e-7)
    # L is the beta-part plus sum d (log k + (k - 1) lt)
    np.testing.assert_allclose(
        wb.shape_loglik(D, d, lt, beta, k),
        wb.loglik_grad(D, d, lt, beta, k)[0]
        + float(np.sum(d * (math.log(k) + (k - 1.) * lt))), rtol=1e-13)
    # f of the preconditioned coordinates: the chain rule and the prior
    scale, pp = np.exp(rs.randn(6) * .3), np.ones(6)
    f = wb.precond_f(D, d, lt, scale, pp, k)
    q = rs.randn(6) * .3
    num = np.array([(f(q + h * e)[0] - f(q - h * e)[0]) / (2 * h)
                    for e in np.eye(6)])
    np.testing.assert_allclose(f(q)[1], num, rtol=1e-7, atol=1e-7)
    # the density integrates to one and has the median the oracle states:
    # S(t) = exp(-t^k exp(eta)), so S(median) = 1 / 2
    for eta0 in (-1.3, .4):
        med = float(wb.median(np.array([eta0]), k)[0])
        assert math.exp(-med ** k * math.exp(eta0)) == pytest.approx(.5,
                                                                     rel=1e-14)
        t = np.exp(np.linspace(-40., 12., 400001))
        dens = np.exp(wb.row_full(eta0, 1., np.log(t), k))   # the density
        mass = np.sum(.5 * (dens[1:] + dens[:-1]) * np.diff(t))
        assert mass == pytest.approx(1., rel=1e-6)
        # a censored row's term is log S(t)
        assert wb.row_full(eta0, 0., math.log(2.), k) \
            == pytest.approx(-2. ** k * math.exp(eta0), rel=1e-14)


def test_long_double_oracle_against_mpmath_on_a_handful_of_rows():
    """The reference of the device tolerances is itself checked: the
    long-double rows against mpmath at 50 digits, on times spanning 1e-6 ..
    1e6 and the three shapes of the device tests.  A long double carries 64
    bits: the allowance is 8 ulps of the largest term of the sum."""
    import mpmath
    rs = np.random.RandomState(2)
    eta = rs.randn(8) * 2.
    lt = np.log(10.) * np.linspace(-6., 6., 8)
    d = (np.arange(8) % 2).astype(np.float64)
    eps = float(np.finfo(LD).eps)
    worst = 0.
    with mpmath.workdps(50):
        for k in (.3, 1., 4.):
            got_full = wb.row_full(eta, d, lt, k, LD)
            got_ll, got_w = wb.row_beta_part(eta, d, lt, k, LD)
            got_med = wb.median(eta, k, LD)
            for i in range(8):
                x, t, dd, kk = (mpmath.mpf(float(a))
                                for a in (eta[i], lt[i], d[i], k))
                m = mpmath.exp(x + kk * t)
                if m > mpmath.mpf(10) ** 4000:
                    continue
                full = dd * (mpmath.log(kk) + (kk - 1) * t + x) - m
                size = max(abs(full), m, abs((kk - 1) * t), abs(x), 1)
                for got, want in ((got_full[i], full), (got_ll[i], dd * x - m),
                                  (got_w[i], dd - m)):
                    if not np.isfinite(got):
                        assert m > mpmath.mpf(10) ** 300
                        continue
                    err = abs(mpmath.mpf(float(got))
                              + mpmath.mpf(float(got - LD(float(got))))
                              - want)
                    worst = max(worst, float(err / size) / eps)
                    assert err <= 8 * eps * size, (k, i)
                med = mpmath.exp((mpmath.log(mpmath.log(2)) - x) / kk)
                err = abs(mpmath.mpf(float(got_med[i]))
                          + mpmath.mpf(float(got_med[i]
                                             - LD(float(got_med[i])))) - med)
                # exp magnifies its argument's rounding by the argument
                arg = max(1., abs(float((mpmath.log(mpmath.log(2)) - x) / kk)))
                assert err <= 8 * eps * arg * med, (k, i)
    print('largest long-double error: %.2f long-double ulps of the largest '
          'term' % worst)


def test_the_exponential_model_is_the_poisson_model_bit_for_bit():
    """k = 1: k * lt is lt, so every float64 value of the oracle is the
    Poisson oracle's on y = d, log_exposure = lt."""
    D, d, lt, truth = _problem(200, 4, 1., 3)
    ll, g = wb.loglik_grad(D, d, lt, truth, 1.)
    pll, pg = po.loglik_grad(D, d, lt, truth)
    assert ll == pll and np.array_equal(g, pg)
    v = np.random.RandomState(4).randn(5)
    assert np.array_equal(wb.hessian_matvec(D, d, lt, truth, v, 1.),
                          po.hessian_matvec(D, d, lt, truth, v))


# ---- the slice update of the shape -------------------------------------------

def _batch_z(x, truth, n_batch=50):
    """(mean(x) - truth) / its batch-means standard error."""
    x = np.asarray(x)
    means = x[:len(x) // n_batch * n_batch].reshape(n_batch, -1).mean(axis=1)
    return (x.mean() - truth) / (means.std(ddof=1) / math.sqrt(n_batch))


class _FastL:
    """L(k) of the oracle's definition for several k at once: 20 000 slice
    updates evaluate it 100 000 times."""

    def __init__(self, D, d, lt, beta):
        self.d, self.lt, self.eta = d, lt, wb.dot(D, beta)

    def shape_loglik(self, coef, k):
        k = np.atleast_1d(k)[:, None]
        with np.errstate(over='ignore'):
            return np.sum(
                self.d * ((np.log(k) + (k - 1.) * self.lt) + self.eta)
                - np.exp(self.eta + k * self.lt), axis=1)


def _slice_chain(jacobian, n_update=20000):
    from bayesbridge_amd import weibull_shape
    from bayesbridge_amd.dispersion import slice_update
    assert weibull_shape.slice_update is slice_update     # imported, no copy
    D, d, lt, truth = _problem(40, 3, 1.5, 5)
    model = _FastL(D, d, lt, truth)
    prior = weibull_shape.check_prior(None)
    # the fast L is the oracle's
    kk = np.array([.3, 1.5, 6.])
    np.testing.assert_allclose(model.shape_loglik(None, kk),
                               wb.shape_loglik(D, d, lt, truth, kk),
                               rtol=1e-12)
    target = weibull_shape.log_conditional(model, truth, prior, jacobian=True)
    f = weibull_shape.log_conditional(model, truth, prior, jacobian=jacobian)
    rs = np.random.RandomState(6)
    theta, draws = 0., np.empty(n_update)
    for j in range(n_update):
        theta = slice_update(theta, f, rs.random_sample)
        draws[j] = theta
    # quadrature of exp f, f with the Jacobian, on a grid that covers it
    grid = np.linspace(-6., 4., 20001)
    dens = np.concatenate([target(grid[j:j + 8])
                           for j in range(0, len(grid), 8)])
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


def test_update_shape_leaves_the_conditional_of_log_k_invariant():
    z_mean, z_var = _slice_chain(True)
    assert abs(z_mean) < Z_BOUND and abs(z_var) < Z_BOUND


def test_update_without_the_jacobian_misses_the_same_bound():
    """The negative control: the same 20 000 updates on the density without
    the Jacobian's theta are compared with the same quadrature."""
    z_mean, z_var = _slice_chain(False)
    assert abs(z_mean) > Z_BOUND


def test_update_shape_is_one_slice_update_on_log_k_and_the_prior_checks():
    from bayesbridge_amd import weibull_shape
    from bayesbridge_amd.dispersion import slice_update
    D, d, lt, truth = _problem(40, 3, 1.5, 5)
    model = wb.OracleModel(D, d, lt)
    prior = weibull_shape.check_prior({'shape': 3., 'rate': 2.})
    rs = np.random.RandomState(0)
    got = weibull_shape.update_shape(model, truth, 1.3, prior,
                                     rs.random_sample)
    rs = np.random.RandomState(0)
    want = math.exp(slice_update(
        math.log(1.3), weibull_shape.log_conditional(model, truth, prior),
        rs.random_sample))
    assert got == want and got != 1.3
    # f = L + shape theta - rate k
    f = weibull_shape.log_conditional(model, truth, prior)
    th = np.array([-.2, .5])
    np.testing.assert_allclose(
        f(th), wb.shape_loglik(D, d, lt, truth, np.exp(th)) + 3. * th
        - 2. * np.exp(th), rtol=1e-14)
    assert np.all(f(np.array([800., -800.])) == -np.inf)
    for bad in ({'shape': 2.}, {'shape': 0., 'rate': 1.}, 3.,
                {'shape': 2., 'rate': 1., 'scale': 1.},
                {'shape': 2., 'rate': np.inf}):
        with pytest.raises(ValueError):
            weibull_shape.check_prior(bad)
    assert weibull_shape.check_prior(None) == {'shape': 2., 'rate': 1.}


# ---- the Gibbs driver on the oracle model -----------------------------------

TRUE_K = 1.5


def _oracle_chain(n_iter, n_burnin, seed, method='nuts', **model_args):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    D, d, lt, truth = _problem(2000, 5, TRUE_K, 7)
    model = wb.OracleModel(D, d, lt, design=_Design(2000, 6), **model_args)
    prior = RegressionCoefPrior(bridge_exponent=2.,
                                _global_scale_parametrization='raw')
    start = wb.newton_mle(D, d, lt, TRUE_K)[0]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            samples, info = BayesBridge(model, prior).gibbs(
                n_iter, n_burnin=n_burnin, seed=seed, coef_sampler_type=method,
                init={'coef': start, 'global_scale': 100.},
                params_to_save='all',
                options={'global_scale_update': None})
    return samples, info, truth, model


def test_gibbs_on_the_oracle_recovers_the_shape_and_the_coefficients():
    """2 000 x 5, k = 1.5: every simulating value lies within 4 posterior
    standard deviations of the posterior mean (log k for the shape)."""
    samples, info, truth, model = _oracle_chain(700, 100, 3)
    assert set(samples) == {'coef', 'local_scale', 'global_scale', 'logp',
                            'weibull_shape'}
    assert samples['weibull_shape'].shape == (600,)
    assert info['_markov_chain_state']['weibull_shape'] \
        == samples['weibull_shape'][-1] == model.shape
    assert info['_markov_chain_state_raw']['weibull_shape'] \
        == samples['weibull_shape'][-1]
    assert info['init']['weibull_shape'] == 1.
    assert 'obs_prec' not in info['_markov_chain_state']
    series = np.vstack((samples['coef'], np.log(samples['weibull_shape'])))
    want = np.concatenate((truth, [math.log(TRUE_K)]))
    for x, value in zip(series, want):
        z = (value - x.mean()) / x.std(ddof=1)
        print('truth %.4f posterior mean %.4f sd %.4f z %.2f'
              % (value, x.mean(), x.std(ddof=1), z))
        assert abs(z) < 4.
    # logp: the likelihood's beta-part at the iteration's shape plus the
    # priors of the coefficients and of the global scale (bridge exponent 2,
    # raw scale, flat hyper-prior, no slab); neither d (log k + (k - 1) lt)
    # nor the shape's prior is in it
    D, d, lt, _ = _problem(2000, 5, TRUE_K, 7)
    sd = info['prior_sd_for_unshrunk']
    for j in (0, 299, 599):
        coef, g = samples['coef'][:, j], samples['global_scale'][j]
        want_logp = wb.loglik_grad(D, d, lt, coef,
                                   samples['weibull_shape'][j])[0] \
            - 5 * math.log(g) - np.sum((coef[1:] / g) ** 2) \
            - .5 * np.sum((coef[:1] / sd) ** 2) \
            - np.sum(np.log(sd[sd < np.inf])) - math.log(g)
        np.testing.assert_allclose(samples['logp'][j], want_logp, rtol=1e-12)
    # the posterior has concentrated: the check above is not vacuous
    assert np.log(samples['weibull_shape']).std() < .1
    assert samples['coef'].std(axis=1).max() < .15


def test_fixed_shape_resume_and_initial_state_on_the_oracle():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    D, d, lt, truth = _problem(2000, 5, TRUE_K, 7)
    prior = RegressionCoefPrior(bridge_exponent=2.,
                                _global_scale_parametrization='raw')
    start = wb.newton_mle(D, d, lt, TRUE_K)[0]

    def run(n_iter, model, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with np.errstate(all='ignore'):
                return BayesBridge(model, prior).gibbs(
                    n_iter, seed=2, coef_sampler_type='hmc',
                    params_to_save='all',
                    options={'global_scale_update': None}, **kw)

    init = {'coef': start, 'global_scale': 100., 'weibull_shape': 1.5}
    fixed_model = wb.OracleModel(D, d, lt, design=_Design(2000, 6), shape=1.5)
    calls = []
    fixed_model.shape_loglik = lambda *a: calls.append(a)
    fixed, info = run(6, fixed_model,
                      init={'coef': start, 'global_scale': 100.})
    assert np.all(fixed['weibull_shape'] == 1.5) and fixed_model.shape == 1.5
    assert not calls           # a fixed shape: no conditional, no uniforms ...
    # ... the whole chain at a fixed k = 1 is the Poisson model's on y = d,
    # log_exposure = lt, whose likelihood is the same bit for bit and whose
    # chain has no such update: one uniform more would part them
    one = wb.OracleModel(D, d, lt, design=_Design(2000, 6), shape=1.)
    exp_chain, _ = run(6, one, init={'coef': start, 'global_scale': 100.})
    poisson, _ = run(6, po.OracleModel(D, d, lt, design=_Design(2000, 6)),
                     init={'coef': start, 'global_scale': 100.})
    for key in poisson:
        assert np.array_equal(exp_chain[key], poisson[key]), key
    # ... so the same seed with a sampled shape started at 1.5 has the same
    # first coefficient draw, and the chains part at the first slice update
    model = wb.OracleModel(D, d, lt, design=_Design(2000, 6))
    sampled, sinfo = run(6, model, init=init)
    assert sinfo['init']['weibull_shape'] == 1.5
    assert np.array_equal(sampled['coef'][:, 0], fixed['coef'][:, 0])
    assert not np.array_equal(sampled['coef'][:, 1], fixed['coef'][:, 1])
    assert len(set(sampled['weibull_shape'])) == 6
    # a fixed shape leaves the stream where a chain without the update would:
    # two fixed-shape chains of 3 + 3 iterations equal the one of 6
    first, finfo = run(3, fixed_model,
                       init={'coef': start, 'global_scale': 100.})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            both, _ = BayesBridge(fixed_model, prior).gibbs_resume(
                finfo, 3, merge=True, prev_samples=first)
    for key in fixed:
        assert np.array_equal(both[key], fixed[key]), key
    # resume equals a straight run
    model = wb.OracleModel(D, d, lt, design=_Design(2000, 6))
    first, finfo = run(3, model, init=init)
    assert finfo['_markov_chain_state']['weibull_shape'] \
        == first['weibull_shape'][-1]
    bridge = BayesBridge(model, prior)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            both, binfo = bridge.gibbs_resume(finfo, 3, merge=True,
                                              prev_samples=first)
    for key in sampled:
        assert np.array_equal(both[key], sampled[key]), key
    # without init['weibull_shape'] the chain starts at 1
    _, dinfo = run(1, wb.OracleModel(D, d, lt, design=_Design(2000, 6)),
                   init={'coef': start, 'global_scale': 100.})
    assert dinfo['init']['weibull_shape'] == 1.
    # a fixed shape refuses another initial value, an invalid one is refused
    with pytest.raises(ValueError, match='held fixed'):
        run(2, wb.OracleModel(D, d, lt, design=_Design(2000, 6), shape=2.),
            init=init)
    for bad in (0., -1., np.inf, np.nan):
        with pytest.raises(ValueError):
            run(2, wb.OracleModel(D, d, lt, design=_Design(2000, 6)),
                init=dict(init, weibull_shape=bad))


# ---- refusals ---------------------------------------------------------------

@pytest.mark.parametrize('method', [None, 'hmc', 'nuts'])
def test_weibull_takes_the_hamiltonian_samplers_on_the_reference_rng(method):
    from bayesbridge_amd import SamplerOptions
    for options in (None, {'rng': 'reference'}):
        opt = SamplerOptions.pick_default_and_create(
            method, options, 'weibull', _Design())
        assert opt.coef_sampler_type == (method or 'hmc')
        assert opt.rng == 'reference'


@pytest.mark.parametrize('method', ['cg', 'cholesky', 'woodbury'])
def test_weibull_refuses_the_gaussian_samplers_and_the_device_rng(method):
    from bayesbridge_amd import BayesBridge, SamplerOptions
    with warnings.catch_warnings():
        warnings.simplefilter('error')       # no warn-and-switch either
        with pytest.raises(ValueError, match="Weibull model draws its "
                                             "coefficients with 'hmc' or "
                                             "'nuts'"):
            SamplerOptions.pick_default_and_create(method, None, 'weibull',
                                                   _Design())
        with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
            SamplerOptions.pick_default_and_create(
                None, {'coef_sampler_type': method}, 'weibull', _Design())
    for ham in (None, 'hmc', 'nuts'):
        with pytest.raises(ValueError, match="rng='reference'"):
            SamplerOptions.pick_default_and_create(
                ham, {'rng': 'device'}, 'weibull', _Design())
    D, d, lt, _ = _problem(50, 4, 1.5, 0)
    bridge = BayesBridge(wb.OracleModel(D, d, lt, design=_Design(50, 5)))
    init = {'global_scale': .1}
    with pytest.raises(ValueError, match="'hmc' or 'nuts' only"):
        bridge.gibbs(2, init=init, seed=0, options=SamplerOptions(method))
    with pytest.raises(ValueError, match="'cg'"):
        bridge.gibbs_batch([0, 1], 2, init=init)
    with pytest.raises(ValueError, match="'cg' only"):
        bridge.gibbs_multichain(2, 2, init=init)


def test_outcome_and_keyword_checks():
    from bayesbridge_amd import RegressionModel, WeibullModel
    from bayesbridge_amd.design_matrix import HipDesignMatrix

    class Design(HipDesignMatrix):       # no device: the checks come first
        shape = (6, 3)
        intercept_added = True
        centered = False

        def __init__(self):
            self._h = None

    inf = np.inf
    d = Design()
    et = np.array([1.5, inf, .2, inf, 7., 3.])
    ct = np.array([inf, 2., inf, .5, inf, inf])
    m = WeibullModel(et, ct, d)
    assert m.name == 'weibull' and m._ham_prefix == 'bbx_weibull_'
    assert np.array_equal(m.event, [1, 0, 1, 0, 1, 1])
    assert np.array_equal(m.time, [1.5, 2., .2, .5, 7., 3.])
    assert np.array_equal(m.log_time, np.log(m.time))
    assert m.calc_intercept_mle() == pytest.approx(math.log(4 / 14.2))
    assert not m._weibull                 # the handle is made on first use
    assert m.shape == 1. and not m.shape_fixed
    assert m.shape_prior == {'shape': 2., 'rate': 1.}
    m.shape = 2.5                         # no handle yet: kept for create
    assert m.shape == 2.5
    assert m.calc_intercept_mle() == pytest.approx(
        math.log(4 / np.sum(m.time ** 2.5)))
    m = RegressionModel((et, ct), d, 'weibull', weibull_shape=3.)
    assert isinstance(m, WeibullModel) and m.shape == 3. and m.shape_fixed
    m = RegressionModel((et, ct), d, 'weibull',
                        weibull_shape_prior={'shape': 1., 'rate': 2.})
    assert m.shape_prior == {'shape': 1., 'rate': 2.}
    # times that are not positive, rows where not exactly one time is finite,
    # a wrong length
    for bad_et, bad_ct in (
            (np.where(np.arange(6) == 0, 0., et), ct),
            (np.where(np.arange(6) == 0, -1., et), ct),
            (et, np.where(np.arange(6) == 1, 0., ct)),
            (et, np.where(np.arange(6) == 0, 2., ct)),       # both finite
            (np.where(np.arange(6) == 0, inf, et), ct),      # neither
            (np.where(np.arange(6) == 0, np.nan, et), ct),
            (et[:5], ct[:5]), (et, ct[:5]), (et.reshape(2, 3), ct)):
        with pytest.raises(ValueError):
            WeibullModel(bad_et, bad_ct, d)
    for bad_k in (0., -2., inf, np.nan, 'a'):
        with pytest.raises(ValueError):
            WeibullModel(et, ct, d, shape=bad_k)
        with pytest.raises(ValueError):
            m.shape = bad_k
    with pytest.raises(ValueError):
        WeibullModel(et, ct, d, shape_prior={'shape': -1., 'rate': 1.})
    with pytest.raises(ValueError, match='held fixed'):
        WeibullModel(et, ct, d, shape=2.,
                     shape_prior={'shape': 1., 'rate': 1.})
    # a design without HIP is refused where the device is first needed

    class NoHip:
        shape = (6, 3)
        use_hip = False
        intercept_added = True

    with pytest.raises(TypeError, match='HipDesignMatrix'):
        WeibullModel(et, ct, NoHip()).handle
    # strata are refused; the keywords belong to this family
    with pytest.raises(ValueError, match='strata are not supported'):
        RegressionModel((et, ct, np.array([0, 0, 0, 1, 1, 1])), d, 'weibull')
    with pytest.raises(ValueError, match='strata are not supported'):
        RegressionModel(et, d, 'weibull')
    y = np.array([0, 1, 2, 0, 7, 3])
    for family, outcome in (('linear', y * 1.), ('logit', (y > 0) * 1.),
                            ('poisson', y), ('negbin', y)):
        with pytest.raises(ValueError, match="weibull_shape is an argument "
                                             "of family='weibull' only"):
            RegressionModel(outcome, d, family, weibull_shape=2.)
        with pytest.raises(ValueError, match="weibull_shape_prior is an "
                                             "argument of family='weibull' "
                                             "only"):
            RegressionModel(outcome, d, family,
                            weibull_shape_prior={'shape': 1., 'rate': 1.})
    # the Cox keywords keep their refusals, word for word
    for kw, text in (
            ({'entry_time': np.zeros(6)},
             "entry_time is an argument of family='cox' only."),
            ({'ties': 'efron'}, "ties is an argument of family='cox' only."),
            ({'weights': np.ones(6)},
             "weights is an argument of family='cox' only."),
            ({'competing_time': np.full(6, inf)},
             "competing_time is an argument of family='cox' only.")):
        with pytest.raises(ValueError, match=re.escape(text)):
            RegressionModel((et, ct), d, 'weibull', **kw)
    names = list(inspect.signature(RegressionModel).parameters)
    assert names[-3:] == ['weibull_shape', 'weibull_shape_prior',
                          'competing_time']
    # predict's own checks come before the device
    m = WeibullModel(et, ct, d)
    coef = np.zeros((3, 4))
    with pytest.raises(ValueError, match='one value per draw'):
        m.predict(coef, np.ones(3))
    with pytest.raises(ValueError, match='strictly positive'):
        m.predict(coef, np.array([1., 2., 0., 1.]))
    with pytest.raises(ValueError, match='new rows only'):
        m.predict(coef, 1., event_time_new=et)
    with pytest.raises(ValueError, match='together'):
        m.predict(coef, 1., X_new=np.zeros((2, 2)),
                  event_time_new=np.array([1., inf]))
    with pytest.raises(ValueError, match='increasing'):
        m.predict_survival(coef, 1., times=[2., 1.])
    with pytest.raises(ValueError, match='increasing'):
        m.predict_survival(coef, 1., times=[0., 1.])


def test_simulated_outcome_has_the_censoring_fraction_and_the_median():
    from bayesbridge_amd import WeibullModel, simulate
    rs = np.random.RandomState(0)
    n = 200000
    X = rs.randn(n, 2) * .3
    beta, k = np.array([.4, -.2]), 1.8
    for frac in (.5, .2):
        et, ct = WeibullModel.simulate_outcome(X, beta, k, frac, seed=3)
        again = WeibullModel.simulate_outcome(X, beta, k, frac, seed=3)
        assert np.array_equal(et, again[0]) and np.array_equal(ct, again[1])
        assert np.all(np.isfinite(et) != np.isfinite(ct))
        assert np.minimum(et, ct).min() > 0
        # a binomial fraction of n rows: 5 sd
        got = np.mean(np.isfinite(ct))
        assert abs(got - frac) < 5 * math.sqrt(frac * (1 - frac) / n)
    # without censoring every time is an event time, and half of the rows
    # lie below their own median (log 2 / exp(eta))^(1 / k)
    et, ct = WeibullModel.simulate_outcome(X, beta, k, 0., seed=4)
    assert np.all(np.isinf(ct))
    med = wb.median(X.dot(beta), k)
    assert abs(np.mean(et < med) - .5) < 5 * .5 / math.sqrt(n)
    # and t^k exp(eta) is a standard exponential: mean 1, variance 1
    e = et ** k * np.exp(X.dot(beta))
    assert abs(e.mean() - 1.) < 5 / math.sqrt(n)
    assert abs(e.var() - 1.) < 5 * math.sqrt(8. / n)
    # the package-level entry adds the intercept
    et1, ct1 = simulate.simulate_outcome(X, beta, 'weibull', intercept=.7,
                                         weibull_shape=k, censoring_frac=0.,
                                         seed=4)
    assert np.all(np.isinf(ct1))
    np.testing.assert_allclose(et1, et * math.exp(-.7 / k), rtol=1e-13)
    assert WeibullModel.simulate_outcome(X[:5], beta, k)[0].shape == (5,)
    with pytest.raises(ValueError):
        WeibullModel.simulate_outcome(X[:5], beta, k, censoring_frac=1.)


# ---- bindings and kernel resources -------------------------------------------

def test_weibull_entry_points_are_declared_bound_and_documented():
    from bayesbridge_amd import _lib
    import bayesbridge_amd
    assert 'WeibullModel' in bayesbridge_amd.__all__
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_weibull_\w+)\s*\(', header))
    shared = {'bbx_weibull_destroy', 'bbx_weibull_loglik_grad',
              'bbx_weibull_loglik_grad_dev', 'bbx_weibull_set_location',
              'bbx_weibull_hessian_matvec', 'bbx_weibull_hessian_matvec_dev',
              'bbx_weibull_hmc_trajectory', 'bbx_weibull_nuts_begin',
              'bbx_weibull_nuts_doubling', 'bbx_weibull_nuts_sample'}
    own = {'bbx_weibull_create', 'bbx_weibull_set_shape',
           'bbx_weibull_shape_loglik'}
    assert declared == shared | own
    predict = 'bbx_design_predictive_summary_weibull'
    assert re.search(r'\b%s\s*\(' % predict, header)
    lib = _lib.load()
    assert declared | {predict} <= set(_lib.EXPORTED_SYMBOLS)
    sigs = _lib._declare(lib)
    for name in shared:
        assert sigs[name] == sigs[name.replace('bbx_weibull_', 'bbx_logit_')]
    hp = sigs['bbx_design_destroy'][0][0]
    assert sigs['bbx_weibull_create'][0][0] is hp
    assert len(sigs['bbx_weibull_create'][0]) == 5
    assert len(sigs['bbx_weibull_shape_loglik'][0]) == 5
    # the family's summary has the negative-binomial one's argument list
    assert sigs[predict] == sigs['bbx_design_predictive_summary_negbin']
    # new symbols and nothing else: the ABI number stays
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() == 113
    assert 'bbx_weibull_*' in header[:header.index('#define BBX_VERSION')]
    # the family code is not one of the header's
    assert not re.search(r'#define BBX_PRED_\w+ 4\b', header)
    summary = open(os.path.join(ROOT, 'bayes-bridge_amd', 'csrc',
                                'predict_summary.hpp')).read()
    assert re.search(r'constexpr int PRED_WEIBULL = 4;', summary)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in declared | {predict}:
        assert name in doc, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '10m' in design and 'weibull.hip' in design
    makefile = open(os.path.join(ROOT, 'bayes-bridge_amd', 'csrc',
                                 'Makefile')).read()
    srcs = re.search(r'SRCS := (.*)', makefile).group(1)
    assert 'weibull.hip' in srcs and 'weibull_predict.hip' in srcs
    # without a device the calls fail with a status, not a crash
    null = None
    assert lib.bbx_weibull_set_shape(null, 1.) < 0
    assert 'NULL weibull handle' in _lib.last_error()
    assert lib.bbx_weibull_shape_loglik(null, None, 1, None, None) < 0
    assert lib.bbx_weibull_destroy(null) == 0
    assert lib.bbx_weibull_create(null, None, None, 1., None) < 0
    assert lib.bbx_design_predictive_summary_weibull(
        null, 2, None, None, None, None, None, 0, None, None, None, None,
        None, None) < 0
    assert predict + ': the design is NULL or destroyed' in _lib.last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_weibull_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "bayes-bridge_amd", "csrc")
    table = _resource_table(os.path.join(src, "weibull.hip"), tmp_path)
    # the three modes of the row kernel, the shape kernel and the shared
    # trajectory kernels: weibull.hip adds no row kernel of its own
    assert sum("glm_row_kernel" in k for k in table) == 3
    assert sum("glm_cand_kernel" in k for k in table) == 1
    assert not any("weibull" in k and "row" in k and "glm_row_kernel" not in k
                   for k in table)
    # the row kernel does the Poisson kernel's work plus one multiply per
    # row: no fewer waves per SIMD than the negative-binomial modes, which
    # hold more (tests/test_negbin_host_logic.py: 4 / 6 / 8)
    # ... and the shape kernel no fewer than weibull_shape_kernel had before
    # the fold onto glm_rows.hpp (64 VGPRs: 8)
    occupancy = glm_row_occupancy(table) + tuple(
        res["Occupancy [waves/SIMD]"] for k, res in table.items()
        if "glm_cand_kernel" in k)
    assert len(occupancy) == 4
    assert all(got >= was
               for got, was in zip(occupancy, (4, 6, 8, 8))), occupancy
    for k in ("cox_step1_kernel", "cox_post_a_kernel", "cox_post_b_kernel",
              "cox_finish_kernel", "cox_nuts_leaf_kernel",
              "cox_nuts_merge_a_kernel", "cox_nuts_merge_b_kernel"):
        assert any(k in name for name in table), (k, sorted(table))
    predict = _resource_table(os.path.join(src, "weibull_predict.hip"),
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
