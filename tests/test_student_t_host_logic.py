"""CPU: the host side of the Student-t model (family='student_t') -- the outcome
and df checks, the sampler and rng dispatch of BayesBridge.gibbs, the refusals
of batches, predict's argument checks, the symbols and constants of the C ABI
and the measurement behind the prediction test's tolerances.  No GPU."""
import math
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest

from conftest import ROOT

import student_t_oracle as O

CSRC = os.path.join(ROOT, 'bayes-bridge_amd', 'csrc')


class _Design():
    """What the checks before any device call look at."""
    use_hip, is_sparse, centered, intercept_added = True, False, True, True
    column_offset = np.zeros(3)

    def __init__(self, n=6, p=4):
        self.shape = (n, p)


Y = (0.3, -1.2, 2.5, 0., 40., -.7)


def _model(y=Y, df=4.):
    from bayesbridge_amd import StudentTModel
    return StudentTModel(np.asarray(y), _Design(len(y)), df)


# ---- the outcome and the degrees of freedom

def test_outcome_and_df_are_checked():
    from bayesbridge_amd import RegressionModel, StudentTModel
    model = _model()
    assert model.name == 'student_t' and model.df == 4.
    assert model.n_obs == 6 and model.n_pred == 4
    assert StudentTModel(np.asarray(Y), _Design()).df == 4.     # the default
    for bad, where in (([0., np.nan, 2., 0., 1., 0.], r'y\[1\]'),
                       ([0., 1., 1., np.inf, 1., 0.], r'y\[3\]'),
                       ([-np.inf, 1., 1., 0., 1., 0.], r'y\[0\]')):
        with pytest.raises(ValueError, match=where):
            StudentTModel(np.array(bad), _Design())
    with pytest.raises(ValueError, match='incompatible|Incompatible'):
        StudentTModel(np.zeros(5), _Design())
    with pytest.raises(ValueError, match='tuple'):
        StudentTModel((np.zeros(6), np.ones(6)), _Design())
    for df in (0., -1., np.nan, np.inf, 'four', None):
        with pytest.raises(ValueError, match='df'):
            StudentTModel(np.asarray(Y), _Design(), df)
    # the factory refuses before it builds a design
    X = np.zeros((6, 3))
    with pytest.raises(ValueError, match=r'y\[1\]'):
        RegressionModel(np.array([0., np.nan, 2., 0., 1., 0.]), X, 'student_t')
    with pytest.raises(ValueError, match='df'):
        RegressionModel(np.asarray(Y), X, 'student_t', df=0.)
    for family in ('linear', 'logit', 'probit'):
        with pytest.raises(ValueError, match="family='student_t' only"):
            RegressionModel(np.ones(6), X, family, df=4.)


def test_intercept_start_is_the_median():
    assert _model().calc_intercept_mle() == float(np.median(Y))


def test_simulated_outcome_has_t_noise():
    from bayesbridge_amd import StudentTModel, simulate
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40000, 3))
    beta = np.array([1., -.5, 0.])
    y = simulate.simulate_outcome(X, beta, 'student_t', intercept=.2, seed=3)
    assert y.shape == (40000,) and y.dtype == np.float64
    assert np.array_equal(y, simulate.simulate_outcome(
        X, beta, 'student_t', intercept=.2, seed=3))
    e = y - .2 - X @ beta
    # a t_4 variate: median 0, P(|e| > 2.776) = 0.05, and far heavier tails than
    # a normal's (P(|e| > 6) = 3.9e-3 against 2e-9)
    assert abs(np.median(e)) < .03
    assert abs(np.mean(np.abs(e) > 2.776) - .05) < 4.5 * math.sqrt(.05 * .95 / 4e4)
    assert 60 < np.sum(np.abs(e) > 6.) < 260
    e = StudentTModel.simulate_outcome(X, beta, df=4., noise_scale=3., seed=1) \
        - X @ beta
    assert abs(np.mean(np.abs(e) > 3. * 2.776) - .05) < .006
    with pytest.raises(ValueError, match='df'):
        StudentTModel.simulate_outcome(X, beta, df=-1.)


# ---- the dispatch of BayesBridge.gibbs

def _bridge():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    bridge = BayesBridge.__new__(BayesBridge)
    bridge.model, bridge.prior = _model(), RegressionCoefPrior()
    bridge._chain = None
    return bridge


def test_sampler_and_rng_dispatch():
    from bayesbridge_amd import SamplerOptions
    from bayesbridge_amd.bayesbridge import NO_OBS_PREC
    assert 'student_t' not in NO_OBS_PREC          # tau is its obs_prec
    pick = SamplerOptions.pick_default_and_create
    dense = _Design()
    opt = pick(None, None, 'student_t', dense)
    assert opt.coef_sampler_type == 'cg' and opt.rng == 'device'
    for kind in ('cholesky', 'woodbury'):
        assert pick(kind, None, 'student_t', dense).coef_sampler_type == kind

    class _Sparse(_Design):
        is_sparse = True
    for kind in ('cholesky', 'woodbury'):
        with pytest.raises(ValueError):
            pick(kind, None, 'student_t', _Sparse())
    assert pick('cg', None, 'student_t', _Sparse()).coef_sampler_type == 'cg'
    for kind in ('hmc', 'nuts'):
        for options in (None, {'rng': 'reference'}):
            with pytest.raises(ValueError, match="'%s' sampler" % kind):
                pick(kind, options, 'student_t', dense)
    with pytest.raises(ValueError, match="rng='reference'"):
        pick(None, {'rng': 'reference'}, 'student_t', dense)
    # a SamplerOptions instance states its own choices: gibbs checks them
    bridge = _bridge()
    for options in (SamplerOptions('hmc'), SamplerOptions('nuts')):
        with pytest.raises(ValueError, match='student_t.*sampler'):
            bridge.gibbs(2, options=options)
    with pytest.raises(ValueError, match="student_t.*rng='reference'"):
        bridge.gibbs(2, options=SamplerOptions('cg', rng='reference'))


def test_batches_and_multichain_are_refused():
    bridge = _bridge()
    with pytest.raises(ValueError, match='gibbs_batch.*student_t'):
        bridge.gibbs_batch([1, 2], 10)
    with pytest.raises(ValueError, match='gibbs_multichain.*student_t'):
        bridge.gibbs_multichain(2, 10)
    assert bridge.batch_width(4) == 0
    from bayesbridge_amd.device_chain import HipGibbsChain
    with pytest.raises(ValueError, match="'student_t'"):
        HipGibbsChain(_Design(), 'cox', np.zeros(6))
    with pytest.raises(ValueError, match='df'):
        HipGibbsChain(_Design(), 'linear', np.zeros(6), df=4.)


def test_sample_layout():
    """obs_prec is one tau per kept sample; the weights only when asked for."""
    bridge = _bridge()
    bridge.n_obs, bridge.n_pred, bridge.n_unshrunk = 6, 4, 1
    samples, _ = bridge._pre_allocate(
        10, 2, ('coef', 'obs_prec', 'mixing_weight', 'logp'))
    assert samples['obs_prec'].shape == (5,)
    assert samples['mixing_weight'].shape == (6, 5)
    samples, _ = bridge._pre_allocate(10, 2, ('coef', 'obs_prec'))
    assert 'mixing_weight' not in samples


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
    assert entry == 'bbx_design_predictive_summary_student_t'
    assert integers == (3, 4.) and arrays == ('draws', 'tau', 'off', 'y', 'c')


def test_loglik_and_gradient_on_a_host_design():
    """StudentTModel.compute_loglik_and_gradient (the initial mode search)
    against the long-double oracle and finite differences, with an outlier."""
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
    from bayesbridge_amd import StudentTModel
    for nu, tau in ((4., 1.), (.5, 2.5), (30., .3)):
        model = StudentTModel(y, _Dense(X), nu)
        ll, grad = model.compute_loglik_and_gradient(beta, tau)
        want = O.loglik(X @ beta, y, tau, nu)
        assert abs(ll - want) <= 1e-13 * abs(want)
        assert np.all(np.isfinite(grad))
        for j in range(4):
            h = np.zeros(4)
            h[j] = 1e-6
            fd = (model.compute_loglik_and_gradient(beta + h, tau, True)[0]
                  - model.compute_loglik_and_gradient(beta - h, tau, True)[0]) \
                / 2e-6
            assert abs(fd - grad[j]) <= 1e-6 * max(1., abs(grad[j]))
    # the mode search hands the model its precision, as it does the linear one
    from bayesbridge_amd.reg_coef_sampler import \
        HipRegressionCoefficientSampler
    src = open(HipRegressionCoefficientSampler.search_mode.__code__
               .co_filename).read()
    assert "model.name in ('linear', 'student_t')" in src


# ---- the C ABI

NEW_SYMBOLS = ('bbx_chain_set_df', 'bbx_chain_get_df',
               'bbx_design_predictive_summary_student_t')


def test_entry_points_are_declared_exported_and_documented():
    from bayesbridge_amd import _lib, replay
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert name in doc, name
    assert re.search(r'#define BBX_MODEL_STUDENT_T 3\b', header)
    assert 'BBX_MODEL_STUDENT_T' in doc
    assert _lib.MODEL_STUDENT_T == 3
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version()
    philox = open(os.path.join(CSRC, 'philox.hpp')).read()
    assert re.search(r'STREAM_MIX = 8\b', philox)
    assert replay.STREAM_MIX == 8
    summary = open(os.path.join(CSRC, 'predict_summary.hpp')).read()
    assert re.search(r'constexpr int PRED_STUDENT_T = 6;', summary)
    srcs = re.search(r'^SRCS := (.*)$', open(os.path.join(CSRC, 'Makefile'))
                     .read(), re.M).group(1).split()
    assert 'student_t.hip' in srcs and 'student_t_predict.hip' in srcs


def test_c_calls_refuse_without_a_device():
    """What is checked before anything touches a device."""
    from ctypes import byref, c_double
    from bayesbridge_amd import _lib
    lib = _lib.load()
    a = np.ones(4)
    p = a.ctypes.data_as(c_void_p)
    df = c_double()
    assert lib.bbx_chain_set_df(None, 4.) == -1
    assert lib.bbx_chain_get_df(None, byref(df)) == -1
    fn = lib.bbx_design_predictive_summary_student_t
    for handle in (None, p):
        assert fn(handle, 2, 4., p, p, None, None, None, 0, p, p, None, None,
                  None, None) == -1
        assert 'the design is NULL or destroyed' in _lib.last_error()


# ---- the tolerances of the GPU prediction test

def test_prediction_tolerances_are_the_measured_ones():
    """The float64 recurrence against the long-double explicit form over the
    cases of the GPU test: PRED_MEASURED, and 16 x that rounded up to a power
    of ten is what the device is held to."""
    worst = dict.fromkeys(O.PRED_KEYS, 0.)
    for X, coef, tau, y in O.predict_cases().values():
        want = O.predict_explicit(X, coef, tau, y)
        rec = O.predict_recurrence(X, coef, tau, y)
        for key in O.PRED_KEYS:
            assert np.all(np.isfinite(np.asarray(want[key], dtype=float)))
            worst[key] = max(worst[key], O.rel_err(rec[key], want[key]))
    print(worst)
    for key in O.PRED_KEYS:
        assert .5 * O.PRED_MEASURED[key] <= worst[key] <= O.PRED_MEASURED[key]
        assert O.pred_tolerance(O.PRED_MEASURED[key]) == \
            (1e-13 if key in ('mean', 'loglik_var') else 1e-14)
