"""CPU: the host side of the ordinal model -- the NumPy oracle
(tests/ordinal_oracle.py) against its own normalisation, against mpmath at 400
digits and against central differences, the cutpoint update (cutpoints.py)
against a grid quadrature with a negative control, the Gibbs driver on the
oracle model, the refusals, the declared entry points and the register /
scratch use of the kernels in csrc/ordinal.hip and csrc/ordinal_predict.hip."""
import math
import os
import re
import warnings

import numpy as np
import pytest

import ordinal_oracle as oo
from conftest import ROOT
from test_cholesky_kernel_resources import (HIPCC, _resource_table,
                                            glm_row_occupancy)

LD = np.longdouble
Z_BOUND = 4.5          # the long-run tests' bound on a batch-means z score

# cutpoint vectors of the oracle's own checks: K = 2, 3, 7, 16, one gap of
# 1e-8 and one of 80
CUTS = (np.array([.3]), np.array([-1., 1.5]),
        np.array([-3., -1., -1. + 1e-8, .5, 2., 82.]),
        np.linspace(-6., 6., 15))


class _Design:
    """What the Gibbs driver and the option checks read of a design."""
    use_hip = True
    is_sparse = False
    intercept_added = False

    def __init__(self, n=50, P=5):
        self.shape = (n, P)


def _problem(n, p, cuts, seed, offset=True):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, p) * .7
    o = rs.randn(n) * .3 if offset else np.zeros(n)
    truth = rs.randn(p) * .8
    D = oo.design(X, True, False)
    y = oo.simulate(rs, oo.dot(D, truth) + o, cuts)
    return D, y, o, truth


# ---- the oracle's own checks ------------------------------------------------
# Measured here (long double, x87 80-bit): the largest |sum_k exp(ll_k) - 1|
# over the eta grid below and the four cutpoint vectors is 2.17e-19 (K = 16;
# 1.08e-19 for K = 2, 3, 7), 2 ulp of a long double's 1: the K exp's round
# once each.  The test's bound is 4 times that residual.
NORMALISATION_RESIDUAL = 2.17e-19
NORMALISATION_TOL = 4 * NORMALISATION_RESIDUAL


def test_oracle_probabilities_sum_to_one():
    eta = np.linspace(-60., 60., 2401)
    worst = 0.
    for cuts in CUTS:
        K = len(cuts) + 1
        total = sum(np.exp(oo.category_loglik(eta, k, cuts))
                    for k in range(K))
        resid = float(np.max(np.abs(total - 1)))
        print('K = %2d  max |sum_k exp(ll_k) - 1| = %.2e' % (K, resid))
        worst = max(worst, resid)
    if np.finfo(LD).eps > 1e-18:
        pytest.skip("long double is a double here: the bound is the 80-bit "
                    "residual")
    assert worst <= NORMALISATION_TOL, worst


def test_oracle_agrees_with_400_digits_to_eta_300():
    """The product form in long double against log(sigma(a) - sigma(b))
    formed as a difference at 400 digits, |eta| up to 300: relative error
    (floor 1) within 8 long-double ulp -- the two softplus and g round once
    each, and eta +- c once."""
    mpmath = pytest.importorskip('mpmath')
    tol = 8 * float(np.finfo(LD).eps)
    worst = 0.
    for cuts in CUTS:
        K = len(cuts) + 1
        for eta in (-300., -135., -50., -37.5, -3., 0., .7, 40., 82., 135.,
                    300.):
            for k in range(K):
                got = oo.category_loglik(np.array([eta]), k, cuts)[0]
                want = oo.category_loglik_mp(eta, k, cuts, dps=400)
                with mpmath.workdps(400):
                    # (a long double as the exact sum of two doubles)
                    head = float(got)
                    err = abs(mpmath.mpf(head) + mpmath.mpf(
                        float(got - LD(head))) - want) / max(1, abs(want))
                worst = max(worst, float(err))
                assert err <= tol, (cuts, eta, k, float(err))
    print('largest relative error (floor 1) %.2e, bound %.2e' % (worst, tol))


def test_a_difference_of_sigmas_is_wrong_past_40():
    """What the oracle must not be: the naive form has lost everything at
    eta = -45 (both sigmas round to 1) where the product form is exact."""
    cuts = CUTS[1]
    eta = np.array([-45.])
    with np.errstate(divide='ignore'):
        naive = np.log(oo.sigma(cuts[1] - eta) - oo.sigma(cuts[0] - eta))
    good = float(oo.category_loglik(eta, 1, cuts, np.float64)[0])
    want = float(oo.category_loglik_mp(-45., 1, cuts))
    assert abs(good - want) < 1e-13 * abs(want)
    assert not abs(naive[0] - want) < 1e-3 * abs(want)


def test_oracle_w_and_d_match_central_differences_of_ll():
    h = LD(1e-6)
    for cuts in CUTS:
        K = len(cuts) + 1
        eta = np.linspace(-8., 8., 41).astype(LD)
        for k in range(K):
            y = np.full(eta.shape, k)
            ll, w, d = oo.row_terms(eta, y, cuts, LD)
            up = oo.row_terms(eta + h, y, cuts, LD)
            dn = oo.row_terms(eta - h, y, cuts, LD)
            # d ll / d eta = w, d w / d eta = -d; O(h^2) truncation ~1e-12
            np.testing.assert_allclose(
                ((up[0] - dn[0]) / (2 * h)).astype(np.float64),
                w.astype(np.float64), rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(
                ((up[1] - dn[1]) / (2 * h)).astype(np.float64),
                -d.astype(np.float64), rtol=1e-9, atol=1e-10)
    # the model's gradient and Hessian product: the chain rule through the
    # design, in float64
    D, y, o, truth = _problem(60, 5, CUTS[1], 0)
    rs = np.random.RandomState(1)
    beta, v, hh = rs.randn(5) * .3, rs.randn(5), 1e-5
    _, grad = oo.loglik_grad(D, y, o, beta, CUTS[1])
    num = np.array([(oo.loglik_grad(D, y, o, beta + hh * e, CUTS[1])[0]
                     - oo.loglik_grad(D, y, o, beta - hh * e, CUTS[1])[0])
                    / (2 * hh) for e in np.eye(5)])
    np.testing.assert_allclose(grad, num, rtol=1e-7, atol=1e-7)
    hv = oo.hessian_matvec(D, y, o, beta, v, CUTS[1])
    num = (oo.loglik_grad(D, y, o, beta + hh * v, CUTS[1])[1]
           - oo.loglik_grad(D, y, o, beta - hh * v, CUTS[1])[1]) / (2 * hh)
    np.testing.assert_allclose(hv, num, rtol=1e-7, atol=1e-7)
    # the long-double forms are the float64 ones
    ll64, g64 = oo.loglik_grad(D, y, o, beta, CUTS[1])
    llx, gx = oo.loglik_grad(D, y, o, beta, CUTS[1], LD)
    np.testing.assert_allclose(ll64, float(llx), rtol=1e-14)
    np.testing.assert_allclose(g64, gx.astype(np.float64), rtol=1e-12,
                               atol=1e-13)
    np.testing.assert_allclose(
        hv, oo.hessian_matvec(D, y, o, beta, v, CUTS[1], LD).astype(
            np.float64), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(
        oo.cutpoint_loglik(D, y, o, beta, CUTS[1]), ll64, rtol=1e-14)


def test_end_categories_at_infinite_eta_and_k2_is_the_logit_model():
    """The convention of csrc/ordinal.hip: the end category on the side of an
    infinite eta gives ll = 0, w = 0, d = 0; every other category there
    -inf.  K = 2 with cutpoint 0 is the logit model of y >= 1."""
    import logit_oracle as lo
    cuts = CUTS[1]
    for eta, end in ((np.inf, 2), (-np.inf, 0)):
        for k in range(3):
            ll, w, d = oo.row_terms(np.array([eta]), np.array([k]), cuts)
            if k == end:
                assert ll[0] == 0. and w[0] == 0. and d[0] == 0.
            else:
                assert ll[0] == -np.inf and abs(w[0]) == 1. and d[0] == 0.
    assert np.isnan(oo.row_terms(np.array([np.nan]), np.array([1]), cuts)[0])
    D, y, o, truth = _problem(80, 4, np.array([0.]), 3, offset=False)
    beta = truth * .7
    ll, grad = oo.loglik_grad(D, y, o, beta, np.array([0.]))
    lll, lgrad = lo.loglik_grad(D, (y >= 1) * 1., np.ones(80), beta)
    np.testing.assert_allclose(ll, lll, rtol=1e-13)
    np.testing.assert_allclose(grad, lgrad, rtol=1e-12, atol=1e-13)


# ---- the cutpoint update ----------------------------------------------------

def _batch_z(x, truth, n_batch=50):
    """(mean(x) - truth) / its batch-means standard error."""
    x = np.asarray(x)
    means = x[:len(x) // n_batch * n_batch].reshape(n_batch, -1).mean(axis=1)
    return (x.mean() - truth) / (means.std(ddof=1) / math.sqrt(n_batch))


class _FastL:
    """L(c) of the oracle's definition in float64: 4 000 sweeps evaluate it
    50 000 times."""

    def __init__(self, D, y, o, beta):
        self.y, self.xo = y, oo.dot(D, beta) + o

    def cutpoint_loglik(self, coef, cuts, gap_term=True):
        return np.array([np.sum(oo.row_terms(self.xo, self.y, c, np.float64,
                                             gap_term)[0])
                         for c in np.atleast_2d(cuts)])


def _quadrature(model, sd):
    """Means and variances of (c_1, c_2) under exp(L(c) - |c|^2 / (2 sd^2)) on
    c_1 < c_2, K = 3, by the rectangle rule on a grid of step 0.01.  L is
    separable but for the gap term: L = A(c_1) + B(c_2) + n_1 g(c_2 - c_1)."""
    grid = np.arange(-4., 4., .01)
    xo, y = model.xo, model.y
    A = np.array([-np.sum(oo.softplus(xo[y == 0] - c))
                  - np.sum(oo.softplus(c - xo[y == 1])) for c in grid])
    B = np.array([-np.sum(oo.softplus(xo[y == 1] - c))
                  - np.sum(oo.softplus(c - xo[y == 2])) for c in grid])
    gap = grid[None, :] - grid[:, None]             # c_2 - c_1
    with np.errstate(all='ignore'):
        g = np.where(gap > 0, np.log(-np.expm1(-np.abs(gap))), -np.inf)
    logf = A[:, None] + B[None, :] + np.sum(y == 1) * g \
        - .5 * (grid[:, None] ** 2 + grid[None, :] ** 2) / sd ** 2
    # the separable form is the oracle's L
    for i, j in ((350, 420), (380, 500), (300, 301)):
        np.testing.assert_allclose(
            A[i] + B[j] + np.sum(y == 1) * g[i, j],
            model.cutpoint_loglik(None, np.array([grid[i], grid[j]]))[0],
            rtol=1e-11)
    f = np.exp(logf - logf.max())
    edge = max(f[0].max(), f[-1].max(), f[:, 0].max(), f[:, -1].max())
    assert edge < 1e-12
    f /= f.sum()
    m1, m2 = np.sum(f.sum(axis=1) * grid), np.sum(f.sum(axis=0) * grid)
    v1 = np.sum(f.sum(axis=1) * (grid - m1) ** 2)
    v2 = np.sum(f.sum(axis=0) * (grid - m2) ** 2)
    return (m1, m2), (v1, v2)


CUT_SWEEPS = 4000
# Checked on the oracle alone before the seed was fixed: seeds 0 ... 7 of the
# sampler's uniforms all pass with the gap term (largest |z| of the four
# statistics 0.4 to 2.4) and all fail without it (largest |z| 48 to 72).
CUT_SEED = 6


def _cutpoint_chain(gap_term, seed=CUT_SEED):
    from bayesbridge_amd import cutpoints
    true_cuts = np.array([-.4, .9])
    D, y, o, truth = _problem(200, 3, true_cuts, 5)
    assert set(y) == {0., 1., 2.}
    model = _FastL(D, y, o, truth)
    prior = cutpoints.check_prior({'sd': 10.})
    np.testing.assert_allclose(
        model.cutpoint_loglik(None, true_cuts)[0],
        oo.cutpoint_loglik(D, y, o, truth, true_cuts), rtol=1e-12)
    rs = np.random.RandomState(seed)
    cuts, draws = oo.initial_cutpoints(y, 3), np.empty((CUT_SWEEPS, 2))
    for k in range(CUT_SWEEPS):
        cuts = cutpoints.update_cutpoints(model, truth, cuts, prior,
                                          rs.random_sample, gap_term=gap_term)
        assert cuts[0] < cuts[1]
        draws[k] = cuts
    mean, var = _quadrature(model, prior['sd'])
    z = []
    for j in range(2):
        z.append(_batch_z(draws[:, j], mean[j]))
        z.append(_batch_z((draws[:, j] - mean[j]) ** 2, var[j]))
        print('gap term %s c_%d: mean %.4f (quadrature %.4f) z %.2f; '
              'variance %.5f (%.5f) z %.2f'
              % (gap_term, j + 1, draws[:, j].mean(), mean[j], z[-2],
                 np.mean((draws[:, j] - mean[j]) ** 2), var[j], z[-1]))
    return np.abs(z)


def test_cutpoint_sweeps_leave_the_conditional_invariant():
    assert _cutpoint_chain(True).max() < Z_BOUND


def test_cutpoint_sweeps_without_the_gap_term_miss_the_same_bound():
    """The negative control: the same sweeps with g_k dropped from L are
    compared with the same quadrature."""
    assert _cutpoint_chain(False).max() > Z_BOUND


def test_update_order_brackets_and_uniform_count():
    from bayesbridge_amd import cutpoints
    calls = []

    class Model:
        def cutpoint_loglik(self, coef, cuts):
            calls.append((coef, np.array(cuts)))
            return -.5 * np.sum((np.asarray(cuts) - [0., 1., 2.]) ** 2, axis=1)

    n_uniform = [0]
    rs = np.random.RandomState(0)

    def uniform():
        n_uniform[0] += 1
        return rs.random_sample()

    start = np.array([-.5, 1., 2.5])
    new = cutpoints.update_cutpoints(Model(), 'beta', start,
                                     {'sd': 10.}, uniform)
    assert np.all(np.diff(new) > 0) and not np.array_equal(new, start)
    # only the sweep's first launch forms the linear predictor
    assert calls[0][0] == 'beta' and all(c[0] is None for c in calls[1:])
    # every candidate is a whole ordered vector that differs from the current
    # state in one entry, k = 0, 1, 2 in that order
    state, k = start.copy(), 0
    for _, cand in calls:
        for c in cand:
            assert np.all(np.diff(c) > 0)
            moved = np.flatnonzero(c != state)
            if list(moved) not in ([], [k]):
                # the next cutpoint's turn: the previous one is final
                state[k] = new[k]
                k += 1
                moved = np.flatnonzero(c != state)
            assert list(moved) in ([], [k]), (c, state, k)
    assert k == 2
    # at least 4 uniforms per cutpoint: level, position, split, one proposal
    assert n_uniform[0] >= 12
    # outside the bracket: -inf without a call
    f = cutpoints.log_conditional(Model(), None, start, 1, {'sd': 10.})
    n_calls = len(calls)
    assert np.all(f(np.array([-.5, -1., 2.5, 3.])) == -np.inf)
    assert len(calls) == n_calls
    assert np.isfinite(f(np.array([0., -1.]))[0]) and len(calls) == n_calls + 1
    assert calls[-1][1].shape == (1, 3)
    for bad in ({'sd': 0.}, {'sd': -1.}, {'sd': np.inf}, {'scale': 1.}, 3.,
                {'sd': 1., 'mean': 0.}):
        with pytest.raises(ValueError):
            cutpoints.check_prior(bad)
    assert cutpoints.check_prior(None) == {'sd': 10.}
    for bad in ([1., 1.], [2., 1.], [0., np.inf], [0.], [0., 1., 2.], 'ab'):
        with pytest.raises(ValueError):
            cutpoints.check_cutpoints(bad, 3)


# ---- the Gibbs driver on the oracle model -----------------------------------

def _oracle_chain(n_iter, seed, method='nuts', init_extra=None, resume=None,
                  **model_args):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    true_cuts = np.array([-1., 0., 1.2])
    D, y, o, truth = _problem(400, 4, true_cuts, 7)
    model = oo.OracleModel(D, y, o, design=_Design(400, 4), **model_args)
    prior = RegressionCoefPrior(bridge_exponent=2.,
                                _global_scale_parametrization='raw')
    init = {'coef': oo.newton_mle(D, y, o, true_cuts), 'global_scale': 100.}
    init.update(init_extra or {})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            bridge = BayesBridge(model, prior)
            samples, info = bridge.gibbs(
                n_iter, seed=seed, coef_sampler_type=method, init=init,
                params_to_save='all', options={'global_scale_update': None})
            if resume:
                samples, info = bridge.gibbs_resume(
                    info, resume, merge=True, prev_samples=samples)
    return samples, info, model, (D, y, o)


def test_gibbs_on_the_oracle_samples_resumes_and_keeps_fixed_cutpoints(
        monkeypatch):
    from bayesbridge_amd import bayesbridge
    samples, info, model, (D, y, o) = _oracle_chain(8, 3)
    assert set(samples) == {'coef', 'local_scale', 'global_scale', 'logp',
                            'cutpoints'}
    assert samples['cutpoints'].shape == (3, 8)
    assert np.all(np.diff(samples['cutpoints'], axis=0) > 0)
    assert len(set(samples['cutpoints'][1])) == 8
    for state in ('_markov_chain_state', '_markov_chain_state_raw'):
        assert np.array_equal(info[state]['cutpoints'],
                              samples['cutpoints'][:, -1])
    assert np.array_equal(model.cutpoints, samples['cutpoints'][:, -1])
    np.testing.assert_array_equal(info['init']['cutpoints'],
                                  oo.initial_cutpoints(y, 4))
    assert 'obs_prec' not in info['_markov_chain_state']
    # logp: the whole likelihood at the iteration's cutpoints plus the priors
    # of the coefficients and of the global scale (bridge exponent 2, raw
    # scale, flat hyper-prior, no slab, no unshrunk coefficient); the
    # cutpoints' prior is not in it
    for k in (0, 7):
        coef, g = samples['coef'][:, k], samples['global_scale'][k]
        want = oo.loglik_grad(D, y, o, coef, samples['cutpoints'][:, k])[0] \
            - 4 * math.log(g) - np.sum((coef / g) ** 2) - math.log(g)
        np.testing.assert_allclose(samples['logp'][k], want, rtol=1e-12)
    # a resumed chain continues bit for bit
    both, binfo, _, _ = _oracle_chain(5, 3, resume=3)
    for key in samples:
        assert np.array_equal(both[key], samples[key]), key
    # init['cutpoints'] is the start; an invalid one is refused
    start = np.array([-.8, .1, 1.])
    _, sinfo, _, _ = _oracle_chain(2, 3, init_extra={'cutpoints': start})
    assert np.array_equal(sinfo['init']['cutpoints'], start)
    for bad in ([0., 1.], [1., 0., 2.], [0., 1., np.inf]):
        with pytest.raises(ValueError, match='invalid initial state'):
            _oracle_chain(2, 3, init_extra={'cutpoints': bad})
    # fixed cutpoints: constant samples, no update, no uniform for them
    count = [0]
    real = bayesbridge.update_cutpoints

    def counting(*args, **kw):
        count[0] += 1
        return real(*args, **kw)

    monkeypatch.setattr(bayesbridge, 'update_cutpoints', counting)
    fixed, finfo, fmodel, _ = _oracle_chain(4, 3, cutpoints=start)
    assert count[0] == 0
    assert np.all(fixed['cutpoints'] == start[:, None])
    _oracle_chain(4, 3)
    assert count[0] == 4
    with pytest.raises(ValueError, match='held fixed'):
        _oracle_chain(2, 3, cutpoints=start,
                      init_extra={'cutpoints': start + .1})


# ---- refusals ---------------------------------------------------------------

@pytest.mark.parametrize('method', [None, 'hmc', 'nuts'])
def test_ordinal_takes_the_hamiltonian_samplers_on_the_reference_rng(method):
    from bayesbridge_amd import SamplerOptions
    for options in (None, {'rng': 'reference'}):
        opt = SamplerOptions.pick_default_and_create(
            method, options, 'ordinal', _Design())
        assert opt.coef_sampler_type == (method or 'hmc')
        assert opt.rng == 'reference'


@pytest.mark.parametrize('method', ['cg', 'cholesky', 'woodbury'])
def test_ordinal_refuses_the_gaussian_samplers_and_the_device_rng(method):
    from bayesbridge_amd import BayesBridge, SamplerOptions
    with warnings.catch_warnings():
        warnings.simplefilter('error')       # no warn-and-switch either
        with pytest.raises(ValueError, match="ordinal model draws its "
                                             "coefficients with 'hmc' or "
                                             "'nuts'"):
            SamplerOptions.pick_default_and_create(method, None, 'ordinal',
                                                   _Design())
        with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
            SamplerOptions.pick_default_and_create(
                None, {'coef_sampler_type': method}, 'ordinal', _Design())
    for ham in (None, 'hmc', 'nuts'):
        with pytest.raises(ValueError, match="rng='reference'"):
            SamplerOptions.pick_default_and_create(
                ham, {'rng': 'device'}, 'ordinal', _Design())
    D, y, o, _ = _problem(50, 4, CUTS[1], 0)
    bridge = BayesBridge(oo.OracleModel(D, y, o, design=_Design(50, 4)))
    init = {'global_scale': .1}
    with pytest.raises(ValueError, match="'hmc' or 'nuts' only"):
        bridge.gibbs(2, init=init, seed=0, options=SamplerOptions(method))
    with pytest.raises(ValueError, match="'cg'"):
        bridge.gibbs_batch([0, 1], 2, init=init)
    with pytest.raises(ValueError, match="'cg' only"):
        bridge.gibbs_multichain(2, 2, init=init)


def test_outcome_and_keyword_checks():
    from bayesbridge_amd import OrdinalModel, RegressionModel
    from bayesbridge_amd.design_matrix import HipDesignMatrix

    class Design(HipDesignMatrix):       # no device: the checks come first
        shape = (6, 3)
        intercept_added = False

        def __init__(self):
            self._h = None

    d = Design()
    y = np.array([0, 1, 2, 0, 2, 1])
    o = np.array([0., .5, -2., 1., 3., .25])
    m = OrdinalModel(y, d)
    assert m.name == 'ordinal' and m._ham_prefix == 'bbx_ordinal_'
    assert m.y.dtype == np.float64 and np.array_equal(m.y, y)
    assert m.n_category == 3 and not m.cutpoints_fixed
    assert np.array_equal(m.offset, np.zeros(6))
    assert not m._ordinal                 # the handle is made on first use
    # the empirical logits of 1/3 and 2/3
    np.testing.assert_allclose(m.cutpoints, [-math.log(2.), math.log(2.)])
    assert m.cutpoint_prior == {'sd': 10.}
    m.cutpoints = [-1., 2.]               # no handle yet: kept for create
    assert np.array_equal(m.cutpoints, [-1., 2.])
    m = RegressionModel((y, o), d, 'ordinal', cutpoints=[0., 1.])
    assert m.cutpoints_fixed and np.array_equal(m.cutpoints, [0., 1.])
    assert np.array_equal(m.offset, o)
    m = RegressionModel(y, d, 'ordinal', cutpoint_prior={'sd': 2.})
    assert m.cutpoint_prior == {'sd': 2.} and not m.intercept_added
    # an empty category is named
    with pytest.raises(ValueError, match='Category 1 of 0 ... 2 has no row'):
        OrdinalModel(np.array([0, 2, 2, 0, 2, 0]), d)
    for bad_y in (y[:5], np.where(np.arange(6) == 2, -1, y),
                  np.where(np.arange(6) == 2, 1.5, y),
                  np.where(np.arange(6) == 2, np.nan, y), y.reshape(2, 3),
                  np.zeros(6), np.where(np.arange(6) == 2, 16, y)):
        with pytest.raises(ValueError):
            OrdinalModel(bad_y, d)
    for bad_o in (o[:5], np.where(np.arange(6) == 4, np.inf, o),
                  np.where(np.arange(6) == 4, np.nan, o)):
        with pytest.raises(ValueError):
            OrdinalModel(y, d, offset=bad_o)
    for bad_c in ([0.], [0., 1., 2.], [1., 0.], [0., 0.], [0., np.inf],
                  [np.nan, 1.], 'ab'):
        with pytest.raises(ValueError):
            OrdinalModel(y, d, cutpoints=bad_c)
        with pytest.raises(ValueError):
            m.cutpoints = bad_c
    with pytest.raises(ValueError):
        OrdinalModel(y, d, cutpoint_prior={'sd': -1.})
    with pytest.raises(ValueError, match='held fixed'):
        OrdinalModel(y, d, cutpoints=[0., 1.], cutpoint_prior={'sd': 1.})
    with pytest.raises(ValueError, match='strata are not supported'):
        RegressionModel((y, o, np.zeros(6)), d, 'ordinal')
    # an intercept: asked for, it is dropped with a warning; on a prebuilt
    # design it is refused
    with pytest.warns(UserWarning, match="won't be added"):
        m = RegressionModel(y, d, 'ordinal', add_intercept=True)
    assert m.name == 'ordinal'

    class WithIntercept(Design):
        intercept_added = True

    with pytest.raises(ValueError, match='without an intercept'):
        RegressionModel(y, WithIntercept(), 'ordinal')
    with pytest.raises(ValueError, match='without an intercept'):
        OrdinalModel(y, WithIntercept())
    # the keywords belong to this family
    for family, outcome in (('linear', y * 1.), ('logit', (y > 0) * 1.),
                            ('poisson', y), ('negbin', y)):
        with pytest.raises(ValueError, match="cutpoints is an argument of "
                                             "family='ordinal' only"):
            RegressionModel(outcome, d, family, cutpoints=[0., 1.])
        with pytest.raises(ValueError, match="cutpoint_prior is an argument "
                                             "of family='ordinal' only"):
            RegressionModel(outcome, d, family, cutpoint_prior={'sd': 1.})
    with pytest.raises(ValueError, match="dispersion is an argument"):
        RegressionModel(y, d, 'ordinal', dispersion=2.)
    with pytest.raises(ValueError, match="entry_time is an argument"):
        RegressionModel(y, d, 'ordinal', entry_time=np.zeros(6))


def test_simulated_outcome_has_the_cumulative_probabilities():
    from bayesbridge_amd import OrdinalModel
    rs = np.random.RandomState(0)
    n = 200000
    X = rs.randn(n, 2) * .5
    beta, cuts = np.array([.8, -.4]), np.array([-1., .2, 1.5])
    o = rs.randn(n) * .2
    y = OrdinalModel.simulate_outcome(X, beta, cuts, offset=o, seed=3)
    assert np.array_equal(
        y, OrdinalModel.simulate_outcome(X, beta, cuts, offset=o, seed=3))
    assert set(y) == {0, 1, 2, 3}
    eta = X.dot(beta) + o
    for k, c in enumerate(cuts):
        p = oo.sigma(c - eta)
        # the mean of n Bernoulli indicators: sd = sqrt(sum p (1 - p)) / n
        assert abs(np.mean(y <= k) - p.mean()) \
            < 5 * math.sqrt(np.sum(p * (1 - p))) / n


def test_ordinal_entry_points_are_declared_bound_and_documented():
    from bayesbridge_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_ordinal_\w+)\s*\(', header))
    shared = {'bbx_ordinal_' + e for e in (
        'destroy', 'loglik_grad', 'loglik_grad_dev', 'set_location',
        'hessian_matvec', 'hessian_matvec_dev', 'hmc_trajectory',
        'nuts_begin', 'nuts_doubling', 'nuts_sample')}
    own = {'bbx_ordinal_create', 'bbx_ordinal_set_cutpoints',
           'bbx_ordinal_cutpoint_loglik'}
    assert declared == shared | own
    predict = 'bbx_design_predictive_summary_ordinal'
    assert re.search(r'\b%s\s*\(' % predict, header)
    lib = _lib.load()
    assert declared | {predict} <= set(_lib.EXPORTED_SYMBOLS)
    sigs = _lib._declare(lib)
    for name in shared:
        assert sigs[name] == sigs[name.replace('bbx_ordinal_', 'bbx_logit_')]
    hp = sigs['bbx_design_destroy'][0][0]
    assert sigs['bbx_ordinal_create'][0][0] is hp
    assert len(sigs['bbx_ordinal_create'][0]) == 6
    assert len(sigs['bbx_ordinal_set_cutpoints'][0]) == 2
    assert len(sigs['bbx_ordinal_cutpoint_loglik'][0]) == 5
    assert len(sigs[predict][0]) == 13
    # new symbols and nothing else: the ABI number stays
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() == 113
    assert 'bbx_ordinal_*' in header[:header.index('#define BBX_VERSION')]
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in declared | {predict}:
        assert name in doc, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '10l' in design and 'ordinal.hip' in design
    # without a device the calls fail with a status, not a crash
    null = None
    assert lib.bbx_ordinal_set_cutpoints(null, None) < 0
    assert 'NULL ordinal handle' in _lib.last_error()
    assert lib.bbx_ordinal_cutpoint_loglik(null, None, 1, None, None) < 0
    assert lib.bbx_ordinal_destroy(null) == 0
    assert lib.bbx_design_predictive_summary_ordinal(
        null, 1, 3, None, None, None, None, 0, None, None, None, None,
        None) < 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ordinal_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "bayes-bridge_amd", "csrc")
    table = _resource_table(os.path.join(src, "ordinal.hip"), tmp_path)
    # the three modes of the row kernel and the cutpoint kernel
    assert sum("glm_row_kernel" in k for k in table) == 3
    assert sum("glm_cand_kernel" in k for k in table) == 1
    # the gradient mode holds two exp and two log1p per row, the logit row
    # kernel's count: no fewer waves per SIMD than the negative-binomial row
    # kernels, whose budget it shares
    occupancy = glm_row_occupancy(table) + tuple(
        res["Occupancy [waves/SIMD]"] for k, res in table.items()
        if "glm_cand_kernel" in k)
    assert all(got >= was
               for got, was in zip(occupancy, (4, 6, 8, 4))), occupancy
    predict = _resource_table(os.path.join(src, "ordinal_predict.hip"),
                              tmp_path)
    assert len(predict) == 1
    assert all("ordinal_summary_kernel" in k for k in predict)
    table.update(predict)
    for name, res in table.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= 64 * 1024, (name, res)
