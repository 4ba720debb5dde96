"""CPU: the host side of the probit model (family='probit') -- the outcome
checks, the sampler and rng dispatch of BayesBridge.gibbs, the refusals of
batches, predict's argument checks, the symbols and constants of the C ABI and
the measurement behind the prediction test's tolerances.  No GPU."""
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest

from conftest import ROOT

import probit_oracle as O

CSRC = os.path.join(ROOT, 'bayes-bridge_amd', 'csrc')


class _Design():
    """What the checks before any device call look at."""
    use_hip, is_sparse, centered, intercept_added = True, False, True, True
    column_offset = np.zeros(3)

    def __init__(self, n=6, p=4):
        self.shape = (n, p)


def _model(y=(0., 1., 1., 0., 1., 0.)):
    from bayesbridge_amd import ProbitModel
    return ProbitModel(np.asarray(y), _Design(len(y)))


# ---- the outcome

def test_outcome_is_checked_as_binary():
    from bayesbridge_amd import ProbitModel, RegressionModel
    model = _model()
    assert model.name == 'probit' and model.n_obs == 6 and model.n_pred == 4
    for bad, where in (([0., 1., 2., 0., 1., 0.], r'y\[2\]'),
                       ([0., 1., 1., .5, 1., 0.], r'y\[3\]'),
                       ([np.nan, 1., 1., 0., 1., 0.], r'y\[0\]')):
        with pytest.raises(ValueError, match=where):
            ProbitModel(np.array(bad), _Design())
    with pytest.raises(ValueError, match='incompatible|Incompatible'):
        ProbitModel(np.zeros(5), _Design())
    # the factory refuses before it builds a design
    X = np.zeros((6, 3))
    with pytest.raises(ValueError, match=r'y\[2\]'):
        RegressionModel(np.array([0., 1., 2., 0., 1., 0.]), X, 'probit')
    with pytest.raises(ValueError, match="family='logit'"):
        RegressionModel((np.ones(6), np.ones(6)), X, 'probit')


def test_simulated_outcome_is_binary_with_the_probit_rate():
    from scipy.special import ndtr
    from bayesbridge_amd import ProbitModel, simulate
    rng = np.random.default_rng(0)
    X = rng.standard_normal((40000, 3))
    beta = np.array([1., -.5, 0.])
    y = simulate.simulate_outcome(X, beta, 'probit', intercept=.2, seed=3)
    assert set(np.unique(y)) == {0., 1.} and y.dtype == np.float64
    assert np.array_equal(
        y, simulate.simulate_outcome(X, beta, 'probit', intercept=.2, seed=3))
    p = ndtr(.2 + X @ beta)
    z = (y.mean() - p.mean()) / np.sqrt(np.mean(p * (1 - p)) / len(y))
    assert abs(z) < 4.5
    assert set(np.unique(ProbitModel.simulate_outcome(X, beta, seed=1))) \
        == {0., 1.}


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
    assert 'probit' in NO_OBS_PREC
    pick = SamplerOptions.pick_default_and_create
    dense = _Design()
    opt = pick(None, None, 'probit', dense)
    assert opt.coef_sampler_type == 'cg' and opt.rng == 'device'
    for kind in ('cholesky', 'woodbury'):
        assert pick(kind, None, 'probit', dense).coef_sampler_type == kind

    class _Sparse(_Design):
        is_sparse = True
    for kind in ('cholesky', 'woodbury'):
        with pytest.raises(ValueError):
            pick(kind, None, 'probit', _Sparse())
    assert pick('cg', None, 'probit', _Sparse()).coef_sampler_type == 'cg'
    for kind in ('hmc', 'nuts'):
        for options in (None, {'rng': 'reference'}):
            with pytest.raises(ValueError, match="'%s' sampler" % kind):
                pick(kind, options, 'probit', dense)
    with pytest.raises(ValueError, match="rng='reference'"):
        pick(None, {'rng': 'reference'}, 'probit', dense)
    # a SamplerOptions instance states its own choices: gibbs checks them
    bridge = _bridge()
    for options in (SamplerOptions('hmc'), SamplerOptions('nuts')):
        with pytest.raises(ValueError, match='sampler'):
            bridge.gibbs(2, options=options)
    with pytest.raises(ValueError, match="rng='reference'"):
        bridge.gibbs(2, options=SamplerOptions('cg', rng='reference'))
    with pytest.raises(ValueError, match='obs_prec'):
        bridge.gibbs(2, init={'global_scale': .1, 'obs_prec': np.ones(6)})


def test_batches_and_multichain_are_refused():
    bridge = _bridge()
    with pytest.raises(ValueError, match='gibbs_batch'):
        bridge.gibbs_batch([1, 2], 10)
    with pytest.raises(ValueError, match='gibbs_multichain'):
        bridge.gibbs_multichain(2, 10)
    assert bridge.batch_width(4) == 0
    from bayesbridge_amd.device_chain import HipGibbsChain
    with pytest.raises(ValueError, match="'probit'"):
        HipGibbsChain(_Design(), 'cox', np.zeros(6))


# ---- predict's argument checks (all before the device)

def test_predict_argument_checks():
    model = _model()
    coef = np.zeros((4, 3))
    with pytest.raises(ValueError):
        model.predict(np.zeros((5, 3)))                     # P
    with pytest.raises(ValueError, match='y_new'):
        model.predict(coef, y_new=np.zeros(6))              # training rows
    with pytest.raises(ValueError, match='columns'):
        model.predict(coef, X_new=np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r'y\[1\]'):
        model.predict(coef, X_new=np.zeros((2, 3)), y_new=[0., 3.])
    with pytest.raises(ValueError, match='sizes'):
        model.predict(coef, X_new=np.zeros((2, 3)), y_new=[0., 1., 1.])
    with pytest.raises(ValueError, match='at least 2 draws'):
        model.predict(np.zeros(4))
    entry, integers, arrays = model._pred_call(3, 'draws', None, 'off', 'y',
                                               None, 'c')
    assert entry == 'bbx_design_predictive_summary_probit'
    assert integers == (3,) and arrays == ('draws', 'off', 'y', 'c')


def test_loglik_and_gradient_on_a_host_design():
    """ProbitModel.compute_loglik_and_gradient (the initial mode search)
    against finite differences, far tails included."""
    from scipy.special import log_ndtr

    class _Dense(_Design):
        def __init__(self, X):
            self.X, self.shape = X, X.shape

        def dot(self, v):
            return self.X @ v

        def Tdot(self, w):
            return self.X.T @ w
    rng = np.random.default_rng(1)
    X = rng.standard_normal((50, 4))
    X[0], X[1] = [30., 0., 0., 0.], [-30., 0., 0., 0.]
    y = (rng.random(50) < .5).astype(float)
    y[:2] = 1.
    from bayesbridge_amd import ProbitModel
    model = ProbitModel(y, _Dense(X))
    beta = np.array([1.2, -.3, .5, 0.])
    ll, grad = model.compute_loglik_and_gradient(beta)
    assert ll == float(np.sum(log_ndtr((2 * y - 1) * (X @ beta))))
    assert np.all(np.isfinite(grad))
    for j in range(4):
        h = np.zeros(4)
        h[j] = 1e-6
        fd = (model.compute_loglik_and_gradient(beta + h, True)[0]
              - model.compute_loglik_and_gradient(beta - h, True)[0]) / 2e-6
        assert abs(fd - grad[j]) <= 1e-6 * max(1., abs(grad[j]))


# ---- the C ABI

NEW_SYMBOLS = ('bbx_device_truncated_normal', 'bbx_chain_get_latent',
               'bbx_chain_get_zbase', 'bbx_design_predictive_summary_probit')


def test_entry_points_are_declared_exported_and_documented():
    from bayesbridge_amd import _lib, hostrng, replay
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert name in doc, name
    for name in ('bbx_replay_truncated_normal', 'bbx_host_log_norm_cdf'):
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert hasattr(hostrng.load(), name)
    assert re.search(r'#define BBX_MODEL_PROBIT 2\b', header)
    assert _lib.MODEL_PROBIT == 2
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version()
    philox = open(os.path.join(CSRC, 'philox.hpp')).read()
    assert re.search(r'STREAM_LATENT = 7\b', philox)
    assert replay.STREAM_LATENT == 7
    summary = open(os.path.join(CSRC, 'predict_summary.hpp')).read()
    assert re.search(r'constexpr int PRED_PROBIT = 5;', summary)
    srcs = re.search(r'^SRCS := (.*)$', open(os.path.join(CSRC, 'Makefile'))
                     .read(), re.M).group(1).split()
    assert 'probit.hip' in srcs and 'probit_predict.hip' in srcs


def test_c_calls_refuse_without_a_device():
    """What is checked before anything touches a device."""
    from bayesbridge_amd import _lib
    lib = _lib.load()
    a = np.zeros(4)
    p = a.ctypes.data_as(c_void_p)
    flags = np.ones(4, dtype=np.uint8).ctypes.data_as(c_void_p)
    assert lib.bbx_device_truncated_normal(0, 1, -1, p, flags, p) == -1
    assert 'n_draw' in _lib.last_error()
    for args in ((None, flags, p), (p, None, p), (p, flags, None)):
        assert lib.bbx_device_truncated_normal(0, 1, 4, *args) == -1
        assert 'NULL' in _lib.last_error()
    assert lib.bbx_chain_get_latent(None, p) == -1
    assert lib.bbx_chain_get_zbase(None, p) == -1
    for handle in (None, p):
        assert lib.bbx_design_predictive_summary_probit(
            handle, 2, p, None, None, None, 0, p, p, None, None, None,
            None) == -1
        assert 'the design is NULL or destroyed' in _lib.last_error()


# ---- the tolerances of the GPU prediction test

def test_prediction_tolerances_are_the_measured_ones():
    """The float64 recurrence against the long-double explicit form over the
    cases of the GPU test: PRED_MEASURED, and 16 x that rounded up to a power
    of ten is what the device is held to."""
    worst = dict.fromkeys(O.PRED_KEYS, 0.)
    for X, coef, y in O.predict_cases().values():
        want = O.predict_explicit(X, coef, y)
        rec = O.predict_recurrence(X, coef, y)
        for key in O.PRED_KEYS:
            assert np.all(np.isfinite(np.asarray(want[key], dtype=float)))
            worst[key] = max(worst[key], O.rel_err(rec[key], want[key]))
    print(worst)
    for key in O.PRED_KEYS:
        assert .5 * O.PRED_MEASURED[key] <= worst[key] <= O.PRED_MEASURED[key]
        assert O.pred_tolerance(O.PRED_MEASURED[key]) == 1e-14
