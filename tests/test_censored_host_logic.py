"""CPU: the host side of the censored-outcome models (family='tobit',
family='lognormal') -- the outcome checks, the mapping from (event_time,
censoring_time), the sampler and rng dispatch of BayesBridge.gibbs, the
refusals, predict's argument checks, the likelihood's gradient, the symbols and
constants of the C ABI and the measurement behind the prediction test's
tolerances.  No GPU."""
import math
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest

from conftest import ROOT

import censored_oracle as O

CSRC = os.path.join(ROOT, 'bayes-bridge_amd', 'csrc')
FAMILIES = ('tobit', 'lognormal')


class _Design():
    """What the checks before any device call look at."""
    use_hip, is_sparse, centered, intercept_added = True, False, True, True
    column_offset = np.zeros(3)

    def __init__(self, n=6, p=4):
        self.shape = (n, p)


Y = np.array([0.3, -1.2, 2.5, 0., 40., -.7])
STATUS = np.array([0, 1, 2, 0, 1, 0])
EVENT = np.array([1.5, np.inf, 2., .25, np.inf, 7.])
CENSORING = np.array([np.inf, 3., np.inf, np.inf, .5, np.inf])


def _model(family='tobit'):
    from bayesbridge_amd import CensoredNormalModel, LogNormalAFTModel
    if family == 'tobit':
        return CensoredNormalModel(Y, STATUS, _Design())
    return LogNormalAFTModel(EVENT, CENSORING, _Design())


# ---- the outcomes

def test_tobit_outcome_is_checked():
    from bayesbridge_amd import CensoredNormalModel, RegressionModel
    model = _model()
    assert model.name == 'tobit' and model.n_obs == 6 and model.n_pred == 4
    assert model.status.dtype == np.uint8 and model.y.dtype == np.float64
    assert np.array_equal(model.status, STATUS)
    for bad, where in (([0., np.nan, 2., 0., 1., 0.], r'y\[1\]'),
                       ([0., 1., 1., np.inf, 1., 0.], r'y\[3\]')):
        with pytest.raises(ValueError, match=where):
            CensoredNormalModel(np.array(bad), STATUS, _Design())
    for bad, where in (([0, 1, 3, 0, 1, 0], r'status\[2\]'),
                       ([0, 1, 2, 0, 1, -1], r'status\[5\]'),
                       ([.5, 1, 2, 0, 1, 0], r'status\[0\]')):
        with pytest.raises(ValueError, match=where):
            CensoredNormalModel(Y, np.array(bad), _Design())
    with pytest.raises(ValueError, match='sizes'):
        CensoredNormalModel(Y[:5], STATUS, _Design())
    with pytest.raises(ValueError, match='sizes'):
        CensoredNormalModel(Y, STATUS[:5], _Design())
    # the factory refuses before it builds a design
    X = np.zeros((6, 3))
    with pytest.raises(ValueError, match=r'\(y, status\)'):
        RegressionModel(Y, X, 'tobit')
    with pytest.raises(ValueError, match=r'status\[2\]'):
        RegressionModel((Y, [0, 1, 3, 0, 1, 0]), X, 'tobit')
    with pytest.raises(ValueError, match=r'y\[1\]'):
        RegressionModel(([0., np.nan, 2., 0., 1., 0.], STATUS), X, 'tobit')
    for family in FAMILIES:
        with pytest.raises(ValueError, match="family='student_t' only"):
            RegressionModel((Y, STATUS), X, family, df=4.)


def test_lognormal_maps_times_to_log_times_and_right_censoring():
    from bayesbridge_amd import LogNormalAFTModel, RegressionModel
    model = _model('lognormal')
    assert model.name == 'lognormal'
    assert np.array_equal(model.status, [0, 1, 0, 0, 1, 0])
    assert np.array_equal(model.y, np.log([1.5, 3., 2., .25, .5, 7.]))
    assert np.array_equal(model.event, [1., 0., 1., 1., 0., 1.])
    assert np.array_equal(model.time, [1.5, 3., 2., .25, .5, 7.])
    assert model.log_time is model.y
    # the Weibull model's outcome, checked by _survival_outcome
    both = CENSORING.copy()
    both[0] = 2.
    with pytest.raises(ValueError, match='Exactly one'):
        LogNormalAFTModel(EVENT, both, _Design())
    zero = EVENT.copy()
    zero[0] = 0.
    with pytest.raises(ValueError, match='strictly positive'):
        LogNormalAFTModel(zero, CENSORING, _Design())
    with pytest.raises(ValueError, match='sizes'):
        LogNormalAFTModel(EVENT[:5], CENSORING[:5], _Design())
    X = np.zeros((6, 3))
    with pytest.raises(ValueError, match='event_time, censoring_time'):
        RegressionModel(EVENT, X, 'lognormal')
    with pytest.raises(ValueError, match='event_time, censoring_time'):
        RegressionModel((EVENT, CENSORING, np.zeros(6)), X, 'lognormal')
    with pytest.raises(ValueError, match='Exactly one'):
        RegressionModel((EVENT, both), X, 'lognormal')
    # the docstring says which way the coefficients point
    assert 'TIME ratios' in LogNormalAFTModel.__doc__
    assert 'opposite sign' in LogNormalAFTModel.__doc__


def test_intercept_start():
    assert _model().calc_intercept_mle() == float(np.mean(Y))
    assert _model('lognormal').calc_intercept_mle() == \
        float(np.mean(np.log([1.5, 3., 2., .25, .5, 7.])))


def test_simulated_outcomes():
    from bayesbridge_amd import (CensoredNormalModel, LogNormalAFTModel,
                                 simulate)
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40000, 3))
    beta = np.array([1., -.5, 0.])
    y, status = CensoredNormalModel.simulate_outcome(X, beta, 2., lower=-1.,
                                                     upper=1.5, seed=3)
    assert status.dtype == np.uint8 and set(status) == {0, 1, 2}
    assert np.all(y[status == 2] == -1.) and np.all(y[status == 1] == 1.5)
    assert np.all((y[status == 0] > -1.) & (y[status == 0] <= 1.5))
    from scipy.stats import norm
    eta = X @ beta
    for code, share in ((2, norm.cdf((-1. - eta) / 2.).mean()),
                        (1, norm.sf((1.5 - eta) / 2.).mean())):
        assert abs((status == code).mean() - share) < .01
    again = CensoredNormalModel.simulate_outcome(X, beta, 2., lower=-1.,
                                                 upper=1.5, seed=3)
    assert np.array_equal(y, again[0]) and np.array_equal(status, again[1])
    for frac in (0., .3, .6):
        et, ct = LogNormalAFTModel.simulate_outcome(X, beta, 1.5, frac, seed=4)
        assert np.all(np.isfinite(et) != np.isfinite(ct))
        assert np.all(np.minimum(et, ct) > 0.)
        assert abs(np.isinf(et).mean() - frac) < .01
        e = (np.log(et) - X @ beta)[np.isfinite(et)]
        if frac == 0.:
            assert abs(e.std() - 1.5) < .03 and abs(e.mean()) < .03
    with pytest.raises(ValueError, match='censoring_frac'):
        LogNormalAFTModel.simulate_outcome(X, beta, censoring_frac=1.)
    # through simulate.simulate_outcome, with an intercept
    et, ct = simulate.simulate_outcome(X, beta, 'lognormal', intercept=.2,
                                       censoring_frac=.5, seed=5)
    assert abs(np.isinf(et).mean() - .5) < .01
    e = np.log(et[np.isfinite(et)]) - (.2 + X @ beta)[np.isfinite(et)]
    assert e.mean() < 0.          # the longer times are the censored ones
    y, status = simulate.simulate_outcome(X, beta, 'tobit', intercept=.2,
                                          seed=5)
    assert set(status) == {0, 2} and np.all(y[status == 2] == 0.)
    assert np.all(y[status == 0] > 0.)


# ---- the dispatch of BayesBridge.gibbs

def _bridge(family):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    bridge = BayesBridge.__new__(BayesBridge)
    bridge.model, bridge.prior = _model(family), RegressionCoefPrior()
    bridge._chain = None
    return bridge


@pytest.mark.parametrize("family", FAMILIES)
def test_sampler_and_rng_dispatch(family):
    from bayesbridge_amd import SamplerOptions
    from bayesbridge_amd.bayesbridge import (CENSORED, NO_OBS_PREC,
                                             SCALAR_OBS_PREC)
    assert family in CENSORED and family in SCALAR_OBS_PREC
    assert family not in NO_OBS_PREC               # tau is its obs_prec
    pick = SamplerOptions.pick_default_and_create
    dense = _Design()
    opt = pick(None, None, family, dense)
    assert opt.coef_sampler_type == 'cg' and opt.rng == 'device'
    for kind in ('cholesky', 'woodbury'):
        assert pick(kind, None, family, dense).coef_sampler_type == kind

    class _Sparse(_Design):
        is_sparse = True
    for kind in ('cholesky', 'woodbury'):
        with pytest.raises(ValueError):
            pick(kind, None, family, _Sparse())
    assert pick('cg', None, family, _Sparse()).coef_sampler_type == 'cg'
    for kind in ('hmc', 'nuts'):
        for options in (None, {'rng': 'reference'}):
            with pytest.raises(ValueError,
                               match="%s.*'%s' sampler" % (family, kind)):
                pick(kind, options, family, dense)
    with pytest.raises(ValueError, match="%s.*rng='reference'" % family):
        pick(None, {'rng': 'reference'}, family, dense)
    # a SamplerOptions instance states its own choices: gibbs checks them
    bridge = _bridge(family)
    for options in (SamplerOptions('hmc'), SamplerOptions('nuts')):
        with pytest.raises(ValueError, match='%s.*sampler' % family):
            bridge.gibbs(2, options=options)
    with pytest.raises(ValueError, match="%s.*rng='reference'" % family):
        bridge.gibbs(2, options=SamplerOptions('cg', rng='reference'))


@pytest.mark.parametrize("family", FAMILIES)
def test_batches_and_multichain_are_refused(family):
    bridge = _bridge(family)
    with pytest.raises(ValueError, match='gibbs_batch.*%s' % family):
        bridge.gibbs_batch([1, 2], 10)
    with pytest.raises(ValueError, match='gibbs_multichain.*%s' % family):
        bridge.gibbs_multichain(2, 10)
    assert bridge.batch_width(4) == 0


def test_the_chain_wrapper_checks_the_status():
    from bayesbridge_amd.device_chain import HipGibbsChain
    with pytest.raises(ValueError, match="'censored'"):
        HipGibbsChain(_Design(), 'cox', np.zeros(6))
    with pytest.raises(ValueError, match='status'):
        HipGibbsChain(_Design(), 'censored', np.zeros(6))
    with pytest.raises(ValueError, match='status'):
        HipGibbsChain(_Design(), 'linear', np.zeros(6), status=STATUS)


@pytest.mark.parametrize("family", FAMILIES)
def test_sample_layout_and_initial_precision(family):
    """obs_prec is one tau per kept sample; the latents only when asked for;
    an initial obs_prec is one number, as for the linear model."""
    bridge = _bridge(family)
    bridge.n_obs, bridge.n_pred, bridge.n_unshrunk = 6, 4, 1
    samples, _ = bridge._pre_allocate(
        10, 2, ('coef', 'obs_prec', 'latent', 'logp'))
    assert samples['obs_prec'].shape == (5,)
    assert samples['latent'].shape == (6, 5)
    samples, _ = bridge._pre_allocate(10, 2, ('coef', 'obs_prec'))
    assert 'latent' not in samples
    assert bridge._initial_obs_prec({'obs_prec': 2.5}, np.zeros(4)) == 2.5
    with pytest.raises(ValueError, match='invalid initial state'):
        bridge._initial_obs_prec({'obs_prec': np.ones(6)}, np.zeros(4))


# ---- predict's argument checks (all before the device)

def test_predict_argument_checks():
    model = _model()
    coef = np.zeros((4, 3))
    tau = np.ones(3)
    with pytest.raises(ValueError):
        model.predict(np.zeros((5, 3)), tau)                     # P
    with pytest.raises(ValueError, match='y_new'):
        model.predict(coef, tau, y_new=np.zeros(6))              # training rows
    with pytest.raises(ValueError, match='status_new'):
        model.predict(coef, tau, status_new=np.zeros(6))
    with pytest.raises(ValueError, match='columns'):
        model.predict(coef, tau, X_new=np.zeros((2, 5)))
    with pytest.raises(ValueError, match='together'):
        model.predict(coef, tau, X_new=np.zeros((2, 3)), y_new=[0., 1.])
    with pytest.raises(ValueError, match=r'y\[1\]'):
        model.predict(coef, tau, X_new=np.zeros((2, 3)), y_new=[0., np.nan],
                      status_new=[0, 1])
    with pytest.raises(ValueError, match=r'status\[0\]'):
        model.predict(coef, tau, X_new=np.zeros((2, 3)), y_new=[0., 1.],
                      status_new=[5, 1])
    with pytest.raises(ValueError, match='obs_prec'):
        model.predict(coef)
    with pytest.raises(ValueError, match='one value per draw'):
        model.predict(coef, np.ones(2))
    with pytest.raises(ValueError, match='positive'):
        model.predict(coef, [1., 0., 1.])
    with pytest.raises(ValueError, match='at least 2 draws'):
        model.predict(np.zeros(4), [1.])
    entry, integers, arrays = model._pred_call(
        3, 'draws', 'tau', 'off', 'y', np.array([0., 1., 2.]), 'c')
    assert entry == 'bbx_design_predictive_summary_censored'
    assert integers == (3, 0)
    assert arrays[:4] == ('draws', 'tau', 'off', 'y') and arrays[5] == 'c'
    assert arrays[4].dtype == np.uint8 and list(arrays[4]) == [0, 1, 2]
    aft = _model('lognormal')
    assert aft._pred_call(3, 'd', 't', None, None, None, None)[1] == (3, 1)
    with pytest.raises(ValueError, match='together'):
        aft.predict(coef, tau, X_new=np.zeros((2, 3)),
                    event_time_new=[1., 2.])
    with pytest.raises(ValueError, match='event_time_new'):
        aft.predict(coef, tau, event_time_new=EVENT,
                    censoring_time_new=CENSORING)
    with pytest.raises(ValueError, match='Exactly one'):
        aft.predict(coef, tau, X_new=np.zeros((2, 3)),
                    event_time_new=[1., 2.], censoring_time_new=[1., np.inf])
    for times in ([], [0., 1.], [2., 1.], [1., np.inf], [[1., 2.]]):
        with pytest.raises(ValueError, match='times'):
            aft.predict_survival(coef, tau, times=times)
    with pytest.raises(ValueError, match='obs_prec'):
        aft.predict_survival(coef, None, times=[1.])


# ---- the likelihood the mode search climbs

class _Dense(_Design):
    def __init__(self, X):
        self.X, self.shape = X, X.shape

    def dot(self, v):
        return self.X @ v

    def Tdot(self, w):
        return self.X.T @ w


def test_loglik_and_gradient_on_a_host_design():
    """compute_loglik_and_gradient against the long-double oracle and central
    differences, with bounds far in both tails."""
    from bayesbridge_amd import CensoredNormalModel, LogNormalAFTModel
    rng = np.random.default_rng(1)
    X = rng.standard_normal((60, 4))
    beta = np.array([1.2, -.3, .5, 0.])
    y = X @ beta + rng.standard_normal(60)
    status = rng.integers(0, 3, 60)
    y[:4] += [8., -8., 8., -8.]
    status[:4] = [1, 1, 2, 2]
    for tau in (1., 2.5, .3):
        model = CensoredNormalModel(y, status, _Dense(X))
        ll, grad = model.compute_loglik_and_gradient(beta, tau)
        want = O.loglik(X @ beta, y, status, tau)
        assert abs(ll - want) <= 1e-13 * abs(want)
        assert np.all(np.isfinite(grad))
        assert model.compute_loglik_and_gradient(beta, tau, True)[1] is None
        for j in range(4):
            h = np.zeros(4)
            h[j] = 1e-6
            fd = (model.compute_loglik_and_gradient(beta + h, tau, True)[0]
                  - model.compute_loglik_and_gradient(beta - h, tau, True)[0]) \
                / 2e-6
            assert abs(fd - grad[j]) <= 1e-6 * max(1., abs(grad[j]))
    # the AFT model is the same likelihood on the log times
    et = np.where(status == 0, np.exp(y), np.inf)
    ct = np.where(status == 0, np.inf, np.exp(y))
    aft = LogNormalAFTModel(et, ct, _Dense(X))
    same = CensoredNormalModel(aft.y, aft.status, _Dense(X))
    got, want = (m.compute_loglik_and_gradient(beta, 1.7) for m in (aft, same))
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    # the mode search hands the models their precision, as it does the linear
    # one
    from bayesbridge_amd.reg_coef_sampler import \
        HipRegressionCoefficientSampler
    src = open(HipRegressionCoefficientSampler.search_mode.__code__
               .co_filename).read()
    assert "model.name in ('tobit', 'lognormal')" in src


# ---- the C ABI

NEW_SYMBOLS = ('bbx_chain_create_censored', 'bbx_device_censored_normal',
               'bbx_design_predictive_summary_censored')


def test_entry_points_are_declared_exported_and_documented():
    from bayesbridge_amd import _lib, replay
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert name in doc, name
    assert re.search(r'#define BBX_MODEL_CENSORED 4\b', header)
    assert 'BBX_MODEL_CENSORED' in doc
    assert _lib.MODEL_CENSORED == 4
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version()
    assert replay.STREAM_LATENT == 7 and hasattr(replay, 'censored_normal')
    summary = open(os.path.join(CSRC, 'predict_summary.hpp')).read()
    assert re.search(r'constexpr int PRED_CENSORED = 7;', summary)
    srcs = re.search(r'^SRCS := (.*)$', open(os.path.join(CSRC, 'Makefile'))
                     .read(), re.M).group(1).split()
    assert 'censored.hip' in srcs and 'censored_predict.hip' in srcs
    import bayesbridge_amd
    for name in ('CensoredNormalModel', 'LogNormalAFTModel'):
        assert name in bayesbridge_amd.__all__


def test_c_calls_refuse_without_a_device():
    """What is checked before anything touches a device."""
    from ctypes import byref
    from bayesbridge_amd import _lib
    lib = _lib.load()
    a = np.ones(4)
    p = a.ctypes.data_as(c_void_p)
    st = np.zeros(4, dtype=np.uint8).ctypes.data_as(c_void_p)
    c = c_void_p()
    fn = lib.bbx_chain_create_censored
    assert fn(None, 4, p, st, 0, None, .5, 2., 0., 0., 1, byref(c)) == -1
    assert fn(p, 4, p, st, 0, None, .5, 2., 0., 0., 1, None) == -1
    assert fn(p, 0, p, st, 0, None, .5, 2., 0., 0., 1, byref(c)) == -1
    assert 'BBX_MODEL_CENSORED' in _lib.last_error()
    assert fn(p, 4, p, None, 0, None, .5, 2., 0., 0., 1, byref(c)) == -1
    draw = lib.bbx_device_censored_normal
    assert draw(0, 1, -1, p, p, st, 1., p) == -1
    assert 'n_draw' in _lib.last_error()
    assert draw(0, 1, 4, None, p, st, 1., p) == -1
    assert draw(0, 1, 4, p, p, st, 0., p) == -1
    assert 'tau' in _lib.last_error()
    bad = np.array([0, 1, 9, 0], dtype=np.uint8)
    assert draw(0, 1, 4, p, p, bad.ctypes.data_as(c_void_p), 1., p) == -1
    assert 'status[2]' in _lib.last_error()
    fn = lib.bbx_design_predictive_summary_censored
    for handle in (None, p):
        assert fn(handle, 2, 0, p, p, None, None, None, None, 0, p, p, None,
                  None, None, None, 0, None, None, None) == -1
        assert 'the design is NULL or destroyed' in _lib.last_error()


# ---- the tolerances of the GPU prediction test

def test_prediction_tolerances_are_the_measured_ones():
    """The float64 recurrence against the long-double explicit form over the
    cases of the GPU test, both models' forms: PRED_MEASURED, and 16 x that
    rounded up to a power of ten is what the device is held to."""
    keys = O.PRED_KEYS + O.SURV_KEYS
    worst = dict.fromkeys(keys, 0.)
    for X, coef, tau, y, status in O.predict_cases().values():
        points = O.survival_points(y)
        assert np.all(np.diff(points) > 0.)
        assert points[1] < y.min() and points[-2] > y.max()
        for exp_mean in (False, True):
            c = np.where(status == 0, -y, 0.) if exp_mean else None
            want = O.predict_explicit(X, coef, tau, y, status, exp_mean, c,
                                      points)
            rec = O.predict_recurrence(X, coef, tau, y, status, exp_mean, c,
                                       points)
            for key in keys:
                assert np.all(np.isfinite(np.asarray(want[key], dtype=float)))
                worst[key] = max(worst[key], O.rel_err(rec[key], want[key]))
    print(worst)
    for key in keys:
        assert .5 * O.PRED_MEASURED[key] <= worst[key] <= O.PRED_MEASURED[key]
        assert O.pred_tolerance(O.PRED_MEASURED[key]) == \
            (1e-14 if key in ('loglik_mean',) + O.SURV_KEYS else 1e-13)
    # the survival function at the far points, and scipy's as a second opinion
    from scipy.stats import norm
    X, coef, tau, y, status = O.predict_cases()[257, 2]
    res = O.predict_explicit(X, coef, tau, y, status, points=O.survival_points(y))
    assert np.all(res['surv_mean'][:, 0] == 1.)
    assert np.all(res['surv_mean'][:, -1] == 0.)
    eta = X @ coef
    direct = norm.sf((y.mean() - eta) * np.sqrt(tau)).mean(axis=1)
    got = O.predict_explicit(X, coef, tau, y, status,
                             points=[y.mean()])['surv_mean'][:, 0]
    assert np.abs(got.astype(float) - direct).max() <= 1e-14
