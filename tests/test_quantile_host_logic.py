"""CPU: the host side of the quantile model (family='quantile') -- the outcome
and level checks, the sampler and rng dispatch of BayesBridge.gibbs, the
refusals of batches, predict's argument checks, the symbols and constants of
the C ABI and the measurement behind the prediction test's tolerances.  No
GPU."""
import math
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest

from conftest import ROOT

import quantile_oracle as O

CSRC = os.path.join(ROOT, 'bayes-bridge_amd', 'csrc')


class _Design():
    """What the checks before any device call look at."""
    use_hip, is_sparse, centered, intercept_added = True, False, True, True
    column_offset = np.zeros(3)

    def __init__(self, n=6, p=4):
        self.shape = (n, p)


Y = (0.3, -1.2, 2.5, 0., 40., -.7)


def _model(y=Y, q=.25):
    from bayesbridge_amd import QuantileModel
    return QuantileModel(np.asarray(y), _Design(len(y)), q)


# ---- the outcome and the level

def test_outcome_and_level_are_checked():
    from bayesbridge_amd import QuantileModel, RegressionModel
    model = _model()
    assert model.name == 'quantile' and model.quantile == .25
    assert model.n_obs == 6 and model.n_pred == 4
    assert QuantileModel(np.asarray(Y), _Design()).quantile == .5   # default
    for bad, where in (([0., np.nan, 2., 0., 1., 0.], r'y\[1\]'),
                       ([0., 1., 1., np.inf, 1., 0.], r'y\[3\]'),
                       ([-np.inf, 1., 1., 0., 1., 0.], r'y\[0\]')):
        with pytest.raises(ValueError, match=where):
            QuantileModel(np.array(bad), _Design())
    with pytest.raises(ValueError, match='incompatible|Incompatible'):
        QuantileModel(np.zeros(5), _Design())
    with pytest.raises(ValueError, match='quantile model.*tuple'):
        QuantileModel((np.zeros(6), np.ones(6)), _Design())
    for q in (0., 1., -.1, 1.5, np.nan, np.inf, 'median', None):
        with pytest.raises(ValueError, match='quantile'):
            QuantileModel(np.asarray(Y), _Design(), q)
    # the factory refuses before it builds a design
    X = np.zeros((6, 3))
    with pytest.raises(ValueError, match=r'y\[1\]'):
        RegressionModel(np.array([0., np.nan, 2., 0., 1., 0.]), X, 'quantile')
    with pytest.raises(ValueError, match='tuple'):
        RegressionModel((np.zeros(6), np.ones(6)), X, 'quantile')
    for q in (0., 1., 2.):
        with pytest.raises(ValueError, match='quantile'):
            RegressionModel(np.asarray(Y), X, 'quantile', quantile=q)
    for family in ('linear', 'logit', 'probit', 'student_t'):
        with pytest.raises(ValueError, match="family='quantile' only"):
            RegressionModel(np.ones(6), X, family, quantile=.5)
    with pytest.raises(ValueError, match="family='student_t' only"):
        RegressionModel(np.ones(6), X, 'quantile', df=4.)


def test_intercept_start_is_the_sample_quantile():
    for q in (.1, .5, .9):
        assert _model(q=q).calc_intercept_mle() == float(np.quantile(Y, q))


def test_simulated_outcome_has_its_quantile_at_the_predictor():
    from bayesbridge_amd import QuantileModel, simulate
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40000, 3))
    beta = np.array([1., -.5, 0.])
    for q in (.1, .5, .8):
        y = simulate.simulate_outcome(X, beta, 'quantile', intercept=.2,
                                      seed=3, quantile=q)
        assert y.shape == (40000,) and y.dtype == np.float64
        assert np.array_equal(y, simulate.simulate_outcome(
            X, beta, 'quantile', intercept=.2, seed=3, quantile=q))
        e = y - .2 - X @ beta
        # P(e < 0) = q, and E rho_q(e) = 1 / tau = 1
        assert abs(np.mean(e < 0.) - q) < 4.5 * math.sqrt(q * (1 - q) / 4e4)
        assert abs(np.mean(O.check_loss(e, q)) - 1.) < .03
    e = QuantileModel.simulate_outcome(X, beta, .8, noise_scale=3., seed=1) \
        - X @ beta
    assert abs(np.mean(O.check_loss(e, .8)) - 3.) < .09
    with pytest.raises(ValueError, match='quantile'):
        QuantileModel.simulate_outcome(X, beta, quantile=1.)


# ---- the dispatch of BayesBridge.gibbs

def _bridge():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    bridge = BayesBridge.__new__(BayesBridge)
    bridge.model, bridge.prior = _model(), RegressionCoefPrior()
    bridge._chain = None
    return bridge


def test_sampler_and_rng_dispatch():
    from bayesbridge_amd import SamplerOptions
    from bayesbridge_amd.bayesbridge import (LATENT, NO_OBS_PREC,
                                             SCALAR_OBS_PREC)
    assert 'quantile' not in NO_OBS_PREC          # tau is its obs_prec
    assert 'quantile' in SCALAR_OBS_PREC and 'quantile' in LATENT
    pick = SamplerOptions.pick_default_and_create
    dense = _Design()
    opt = pick(None, None, 'quantile', dense)
    assert opt.coef_sampler_type == 'cg' and opt.rng == 'device'
    for kind in ('cholesky', 'woodbury'):
        assert pick(kind, None, 'quantile', dense).coef_sampler_type == kind

    class _Sparse(_Design):
        is_sparse = True
    for kind in ('cholesky', 'woodbury'):
        with pytest.raises(ValueError):
            pick(kind, None, 'quantile', _Sparse())
    assert pick('cg', None, 'quantile', _Sparse()).coef_sampler_type == 'cg'
    for kind in ('hmc', 'nuts'):
        for options in (None, {'rng': 'reference'}):
            with pytest.raises(ValueError,
                               match="quantile model.*'%s' sampler" % kind):
                pick(kind, options, 'quantile', dense)
    with pytest.raises(ValueError, match="quantile model.*rng='reference'"):
        pick(None, {'rng': 'reference'}, 'quantile', dense)
    # a SamplerOptions instance states its own choices: gibbs checks them
    bridge = _bridge()
    for options in (SamplerOptions('hmc'), SamplerOptions('nuts')):
        with pytest.raises(ValueError, match='quantile.*sampler'):
            bridge.gibbs(2, options=options)
    with pytest.raises(ValueError, match="quantile.*rng='reference'"):
        bridge.gibbs(2, options=SamplerOptions('cg', rng='reference'))


def test_batches_and_multichain_are_refused():
    bridge = _bridge()
    with pytest.raises(ValueError, match='gibbs_batch.*quantile'):
        bridge.gibbs_batch([1, 2], 10)
    with pytest.raises(ValueError, match='gibbs_multichain.*quantile'):
        bridge.gibbs_multichain(2, 10)
    assert bridge.batch_width(4) == 0
    from bayesbridge_amd.device_chain import HipGibbsChain
    with pytest.raises(ValueError, match="'quantile'"):
        HipGibbsChain(_Design(), 'cox', np.zeros(6))
    with pytest.raises(ValueError, match='quantile'):
        HipGibbsChain(_Design(), 'linear', np.zeros(6), quantile=.5)
    for q in (0., 1., float('nan')):
        with pytest.raises(ValueError, match='quantile'):
            HipGibbsChain(_Design(), 'quantile', np.zeros(6), quantile=q)


def test_sample_layout_and_initial_precision():
    """obs_prec is one tau per kept sample; the weights only when asked for;
    the chain starts at the asymmetric-Laplace law's ML scale."""
    bridge = _bridge()
    bridge.n_obs, bridge.n_pred, bridge.n_unshrunk = 6, 4, 1
    samples, _ = bridge._pre_allocate(
        10, 2, ('coef', 'obs_prec', 'mixing_weight', 'logp'))
    assert samples['obs_prec'].shape == (5,)
    assert samples['mixing_weight'].shape == (6, 5)
    samples, _ = bridge._pre_allocate(10, 2, ('coef', 'obs_prec'))
    assert 'mixing_weight' not in samples
    bridge.model.design.dot = lambda coef: np.full(6, coef[0])
    tau = bridge._initial_obs_prec({}, np.array([.1, 0., 0., 0.]))
    want = 1. / np.mean(O.check_loss(np.asarray(Y) - .1, .25))
    assert abs(tau - want) <= 1e-15 * want
    assert bridge._initial_obs_prec({'obs_prec': 2.5}, np.zeros(4)) == 2.5


# ---- predict's argument checks (all before the device)

def test_predict_argument_checks():
    model = _model()
    coef = np.zeros((4, 3))
    tau = np.ones(3)
    with pytest.raises(ValueError):
        model.predict(np.zeros((5, 3)), tau)                     # P
    with pytest.raises(ValueError, match='y_new'):
        model.predict(coef, tau, y_new=np.zeros(6))              # training rows
    with pytest.raises(ValueError, match='columns'):
        model.predict(coef, tau, X_new=np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r'y\[1\]'):
        model.predict(coef, tau, X_new=np.zeros((2, 3)), y_new=[0., np.nan])
    with pytest.raises(ValueError, match='sizes'):
        model.predict(coef, tau, X_new=np.zeros((2, 3)), y_new=[0., 1., 1.])
    with pytest.raises(ValueError, match='obs_prec'):
        model.predict(coef)
    with pytest.raises(ValueError, match='one value per draw'):
        model.predict(coef, np.ones(2))
    with pytest.raises(ValueError, match='positive'):
        model.predict(coef, [1., 0., 1.])
    with pytest.raises(ValueError, match='at least 2 draws'):
        model.predict(np.zeros(4), [1.])
    entry, integers, arrays = model._pred_call(3, 'draws', 'tau', 'off', 'y',
                                               None, 'c')
    assert entry == 'bbx_design_predictive_summary_quantile'
    assert integers == (3, .25) and arrays == ('draws', 'tau', 'off', 'y', 'c')


def test_loglik_and_gradient_on_a_host_design():
    """QuantileModel.compute_loglik_and_gradient (the initial mode search)
    against the long-double oracle and finite differences (no residual is
    within the step of a kink), with an outlier."""
    class _Dense(_Design):
        def __init__(self, X):
            self.X, self.shape = X, X.shape

        def dot(self, v):
            return self.X @ v

        def Tdot(self, w):
            return self.X.T @ w
    rng = np.random.default_rng(1)
    X = rng.standard_normal((50, 4))
    beta = np.array([1.2, -.3, .5, 0.])
    y = X @ beta + rng.standard_t(4., 50)
    y[0] += 1e4
    assert np.abs(y - X @ beta).min() > 1e-4
    from bayesbridge_amd import QuantileModel
    for q, tau in ((.5, 1.), (.05, 2.5), (.9, .3)):
        model = QuantileModel(y, _Dense(X), q)
        ll, grad = model.compute_loglik_and_gradient(beta, tau)
        want = O.loglik(X @ beta, y, tau, q)
        assert abs(ll - want) <= 1e-13 * abs(want)
        assert np.all(np.isfinite(grad))
        for j in range(4):
            h = np.zeros(4)
            h[j] = 1e-7
            fd = (model.compute_loglik_and_gradient(beta + h, tau, True)[0]
                  - model.compute_loglik_and_gradient(beta - h, tau, True)[0]) \
                / 2e-7
            assert abs(fd - grad[j]) <= 1e-5 * max(1., abs(grad[j]))
    # the mode search hands the model its precision, as it does the linear
    # one: every evaluation it makes gets the obs_prec it was given
    from bayesbridge_amd.reg_coef_sampler import \
        HipRegressionCoefficientSampler

    class _Counted(_Dense):
        n_matvec = 0

        def memoize_dot(self, flag):
            pass

        def reset_matvec_count(self):
            pass
    model = QuantileModel(y[1:], _Counted(X[1:]), .9)
    seen = []
    inner = model.compute_loglik_and_gradient

    def recording(beta, obs_prec=1., loglik_only=False):
        seen.append(obs_prec)
        return inner(beta, obs_prec, loglik_only=loglik_only)
    model.compute_loglik_and_gradient = recording
    sampler = HipRegressionCoefficientSampler(4, np.array([2.]), 'cg', 2.)
    mode, info = sampler.search_mode(np.zeros(4), np.ones(3), .5, 2.5, model)
    assert len(seen) > 2 and set(seen) == {2.5}
    assert inner(mode, 2.5, True)[0] > inner(np.zeros(4), 2.5, True)[0]


# ---- the C ABI

NEW_SYMBOLS = ('bbx_chain_set_quantile', 'bbx_chain_get_quantile',
               'bbx_device_inverse_gaussian',
               'bbx_design_predictive_summary_quantile')


def test_entry_points_are_declared_exported_and_documented():
    from bayesbridge_amd import _lib, hostrng, replay
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert name in doc, name
    assert re.search(r'\bbbx_replay_inverse_gaussian\s*\(', header)
    assert hasattr(hostrng.load(), 'bbx_replay_inverse_gaussian')
    assert re.search(r'#define BBX_MODEL_QUANTILE 5\b', header)
    assert 'BBX_MODEL_QUANTILE' in doc
    assert _lib.MODEL_QUANTILE == 5
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version()
    philox = open(os.path.join(CSRC, 'philox.hpp')).read()
    assert re.search(r'STREAM_QMIX = 9\b', philox)
    assert re.search(r'STREAM_MIX = 8\b', philox)        # stays Student-t's
    assert replay.STREAM_QMIX == 9
    summary = open(os.path.join(CSRC, 'predict_summary.hpp')).read()
    assert re.search(r'constexpr int PRED_QUANTILE = 9;', summary)
    srcs = re.search(r'^SRCS := (.*)$', open(os.path.join(CSRC, 'Makefile'))
                     .read(), re.M).group(1).split()
    assert 'quantile.hip' in srcs and 'quantile_predict.hip' in srcs


def test_c_calls_refuse_without_a_device():
    """What is checked before anything touches a device."""
    from ctypes import byref, c_double
    from bayesbridge_amd import _lib
    lib = _lib.load()
    a = np.ones(4)
    p = a.ctypes.data_as(c_void_p)
    q = c_double()
    assert lib.bbx_chain_set_quantile(None, .5) == -1
    assert lib.bbx_chain_get_quantile(None, byref(q)) == -1
    fn = lib.bbx_design_predictive_summary_quantile
    for handle in (None, p):
        assert fn(handle, 2, .5, p, p, None, None, None, 0, p, p, None, None,
                  None, None) == -1
        assert 'the design is NULL or destroyed' in _lib.last_error()
    ig = lib.bbx_device_inverse_gaussian
    assert ig(0, 1, -1, p, 1., p) == -1
    assert ig(0, 1, 4, None, 1., p) == -1
    assert ig(0, 1, 4, p, 0., p) == -1 and 'lambda' in _lib.last_error()
    neg = np.array([1., 2., -3., 1.])
    assert ig(0, 1, 4, neg.ctypes.data_as(c_void_p), 1., p) == -1
    assert 'm[2]' in _lib.last_error()


# ---- the tolerances of the GPU prediction test

def test_prediction_tolerances_are_the_measured_ones():
    """The float64 recurrence against the long-double explicit form over the
    cases of the GPU test: PRED_MEASURED, and 16 x that rounded up to a power
    of ten is what the device is held to.  (The oracle alone: no library code
    runs here.)"""
    worst = dict.fromkeys(O.PRED_KEYS, 0.)
    for X, coef, tau, y in O.predict_cases().values():
        want = O.predict_explicit(X, coef, tau, y, O.PRED_Q)
        rec = O.predict_recurrence(X, coef, tau, y, O.PRED_Q)
        for key in O.PRED_KEYS:
            assert np.all(np.isfinite(np.asarray(want[key], dtype=float)))
            worst[key] = max(worst[key], O.rel_err(rec[key], want[key]))
    print(worst)
    for key in O.PRED_KEYS:
        assert .5 * O.PRED_MEASURED[key] <= worst[key] <= O.PRED_MEASURED[key]
