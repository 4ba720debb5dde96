"""CPU: the host side of posterior prediction (model.predict on
bbx_design_predictive_summary) -- the oracle against closed forms, its two
forms against each other (the measurement the GPU tests' tolerances come
from), every Python refusal on a fake design and a fake library, the C ABI's
declarations, the refusals of the C call that need no device, and the
summary kernel's register use."""
import math
import os
import re
import warnings
from ctypes import c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import predict_cases as pc
import predict_oracle as po
from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table

ENTRY = 'bbx_design_predictive_summary'
LOG_2PI = math.log(2. * math.pi)


# ---- the oracle against closed forms ----------------------------------------

@pytest.mark.parametrize('form', [po.explicit, po.recurrence])
def test_one_draw_has_no_spread_and_lpd_is_its_loglik(form):
    for family in po.FAMILIES:
        case = pc.problem(family, 'dense64', 50, 3, 1, 1)
        res = pc.oracle(case, form)
        assert np.all(res['sd'] == 0.)
        assert np.array_equal(res['mean'], res['mu'][:, 0])
        assert np.allclose(np.asarray(res['lpd'], float), res['ll'][:, 0],
                           rtol=1e-15, atol=0)
        assert np.array_equal(res['loglik_mean'], res['ll'][:, 0])
        assert np.isnan(np.asarray(res['loglik_var'], float)).all()


@pytest.mark.parametrize('form', [po.explicit, po.recurrence])
def test_two_draws_by_hand(form):
    """One row x = 1 without intercept, coefficients a and b."""
    Xt = np.ones((1, 1))
    a, b = .5, -1.25
    coef = np.array([[a, b]])

    def close(x, y):
        return abs(float(x) - y) <= 1e-14 * max(abs(y), 1.)

    # linear: y = 2, precisions 1 and 4
    res = form('linear', Xt, coef, y=[2.], obs_prec=[1., 4.],
               const=po.ll_const('linear', [2.]))
    l1 = -.5 * (2 - a) ** 2 - .5 * LOG_2PI
    l2 = .5 * math.log(4.) - 2. * (2 - b) ** 2 - .5 * LOG_2PI
    assert close(res['mean'][0], (a + b) / 2)
    assert close(res['sd'][0], abs(a - b) / 2)
    assert close(res['lpd'][0], math.log((math.exp(l1) + math.exp(l2)) / 2))
    assert close(res['loglik_mean'][0], (l1 + l2) / 2)
    assert close(res['loglik_var'][0], (l1 - l2) ** 2 / 2)
    # logit: 2 successes in 3 trials
    res = form('logit', Xt, coef, y=[2.], n_trial=[3.],
               const=po.ll_const('logit', [2.], [3.]))
    p1, p2 = 1 / (1 + math.exp(-a)), 1 / (1 + math.exp(-b))
    l1, l2 = (math.log(3 * p ** 2 * (1 - p)) for p in (p1, p2))
    assert close(res['mean'][0], (p1 + p2) / 2)
    assert close(res['sd'][0], abs(p1 - p2) / 2)
    assert close(res['lpd'][0], math.log((math.exp(l1) + math.exp(l2)) / 2))
    assert close(res['loglik_var'][0], (l1 - l2) ** 2 / 2)
    # Poisson: y = 3 at exposure 2
    res = form('poisson', Xt, coef, y=[3.], offset=[math.log(2.)],
               const=po.ll_const('poisson', [3.]))
    m1, m2 = 2 * math.exp(a), 2 * math.exp(b)
    l1, l2 = (3 * math.log(m) - m - math.log(6.) for m in (m1, m2))
    assert close(res['mean'][0], (m1 + m2) / 2)
    assert close(res['sd'][0], abs(m1 - m2) / 2)
    assert close(res['lpd'][0], math.log((math.exp(l1) + math.exp(l2)) / 2))
    assert close(res['loglik_mean'][0], (l1 + l2) / 2)


@pytest.mark.parametrize('form', [po.explicit, po.recurrence])
def test_a_constant_predictor(form):
    """Every draw the same: no spread, lpd = ll, no variance of ll."""
    case = pc.problem('logit', 'dense64', 40, 3, 1, 2)
    case['coef'] = np.repeat(case['coef'], 9, axis=1)
    res = pc.oracle(case, form)
    one = pc.oracle(dict(case, coef=case['coef'][:, :1]), form)
    tiny = 4e-16
    assert np.abs(np.asarray(res['sd'], float)).max() <= tiny
    assert np.abs(np.asarray(res['loglik_var'], float)).max() <= tiny
    assert po.within(res['mean'], one['mean'], tiny)
    assert po.within(res['lpd'], one['ll'][:, 0], tiny)


def test_infinite_draws_in_the_recurrence():
    """-inf adds exactly 0 to lpd, all -inf gives -inf (not NaN), an
    infinite mean stays, a NaN stays a NaN."""
    Xt = np.ones((1, 1))
    coef = np.array([[.1, 12000., .2]])   # (past long double's range too)
    kw = {'y': [1.], 'const': po.ll_const('poisson', [1.])}
    res = po.recurrence('poisson', Xt, coef, **kw)
    ext = po.explicit('poisson', Xt, coef, **kw)
    assert res['mean'][0] == np.inf == ext['mean'][0]
    assert res['loglik_mean'][0] == -np.inf == ext['loglik_mean'][0]
    assert np.isfinite(res['lpd'][0])
    assert po.within(res['lpd'], ext['lpd'], 1e-15)
    two = po.recurrence('poisson', Xt, coef[:, [0, 2]], **kw)
    assert abs(res['lpd'][0] - (two['lpd'][0] + math.log(2 / 3))) < 1e-14
    res = po.recurrence('poisson', Xt, np.full((1, 3), 12000.), **kw)
    ext = po.explicit('poisson', Xt, np.full((1, 3), 12000.), **kw)
    assert res['lpd'][0] == -np.inf == ext['lpd'][0]
    assert res['mean'][0] == np.inf and res['loglik_mean'][0] == -np.inf
    res = po.recurrence('poisson', Xt, np.array([[.1, np.nan, .2]]), **kw)
    assert all(np.isnan(res[key][0]) for key in po.KEYS)


# ---- the two forms against each other: where the tolerances come from -------

def test_tolerances_are_sixteen_times_the_measured_error():
    """Over every input of the GPU tests 1, 2, 3, 6 and 7 the float64
    recurrence form against the long-double explicit form, relative to the
    largest magnitude of each vector: the GPU tests' tolerance is 16 x the
    largest error, rounded up to a power of ten."""
    import test_hip_predict as thp
    worst = dict.fromkeys(po.KEYS, 0.)
    for case, outcome in pc.measured_cases():
        ext = pc.oracle(case, po.explicit, outcome)
        rec = pc.oracle(case, po.recurrence, outcome)
        for key in po.KEYS if outcome else po.KEYS[:2]:
            worst[key] = max(worst[key], po.rel_err(rec[key], ext[key]))
    print({key: '%.2e' % v for key, v in worst.items()})
    for key in po.KEYS:
        assert worst[key] > 0.
        # the figure written down is the one measured (libm's last bits may
        # move it a little between machines)
        assert .5 <= worst[key] / thp.MEASURED[key] <= 2., key
        rule = 10. ** math.ceil(math.log10(16 * thp.MEASURED[key]))
        assert math.isclose(thp.TOL[key], rule, rel_tol=1e-12), key
        assert 16 * worst[key] <= thp.TOL[key], key


# ---- the Python refusals: fake design, fake library -------------------------

class _FakeDesign():
    use_hip = True
    handle = c_void_p(1)
    centered = True

    def __init__(self, n, P, intercept=True):
        self.shape = (n, P)
        self.intercept_added = intercept
        self.column_offset = np.zeros(P - int(intercept))


class _FakeLib():
    """Refuses to be called: every refusal comes before the device."""

    def __getattr__(self, name):
        raise AssertionError('the library was reached: ' + name)


N, P, S = 12, 4, 5


def _fake_models(monkeypatch):
    from bayesbridge_amd import _lib, model
    monkeypatch.setattr(_lib, 'load', lambda: _FakeLib())
    monkeypatch.setattr(model, '_new_design', lambda *a: pytest.fail(
        'a design was built before the checks were done'))
    rs = np.random.RandomState(0)
    design = _FakeDesign(N, P)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return {
            'linear': model.LinearModel(rs.randn(N), design),
            'logit': model.LogisticModel(np.ones(N), 2 * np.ones(N), design),
            'poisson': model.PoissonModel(np.ones(N), None, design)}


def test_predict_refusals_come_before_any_device_call(monkeypatch):
    models = _fake_models(monkeypatch)
    coef = np.zeros((P, S))
    X = np.zeros((3, P - 1))
    tau = np.ones(S)
    for name, m in models.items():
        kw = {'obs_prec': tau} if name == 'linear' else {}
        for bad in (np.zeros((P + 1, S)), np.zeros(P - 1),
                    np.zeros((P, S, 2)), np.zeros((P, 0))):
            with pytest.raises(ValueError, match='coef must have shape'):
                m.predict(bad, **kw)
        for bad in (np.zeros((3, P)), np.zeros((0, P - 1)), np.zeros(P - 1),
                    sparse.csr_matrix((3, P))):
            with pytest.raises(ValueError, match='X_new must have at least '
                                                 'one row and the model'):
                m.predict(coef, X_new=bad, **kw)
        with pytest.raises(ValueError, match='y_new is an argument of new '
                                             'rows only'):
            m.predict(coef, y_new=np.ones(N), **kw)
        with pytest.raises(ValueError, match='at least 2 draws'):
            m.predict(coef[:, 0], **({'obs_prec': tau[:1]} if kw else {}))
        with pytest.raises(ValueError, match='at least 2 draws'):
            m.predict(coef[:, :1], **({'obs_prec': tau[:1]} if kw else {}))
    lin, logit, pois = (models[f] for f in po.FAMILIES)
    # the linear model
    with pytest.raises(ValueError, match='obs_prec .* is required'):
        lin.predict(coef)
    for bad in (np.ones(S + 1), np.ones(1)):
        with pytest.raises(ValueError, match='one value per draw'):
            lin.predict(coef, obs_prec=bad)
    for value in (0., -1., np.nan, np.inf):
        bad = tau.copy()
        bad[2] = value
        with pytest.raises(ValueError, match='strictly positive and finite'):
            lin.predict(coef, obs_prec=bad)
    with pytest.raises(ValueError, match='Incompatible sizes of the outcome'):
        lin.predict(coef, X_new=X, y_new=np.ones(4), obs_prec=tau)
    for m in (logit, pois):
        with pytest.raises(TypeError, match='obs_prec'):
            m.predict(coef, obs_prec=tau)
    # the logit model: the constructor's rules
    with pytest.raises(ValueError, match='incompatible sizes'):
        logit.predict(coef, X_new=X, y_new=np.ones(4))
    with pytest.raises(ValueError, match='incompatible sizes'):
        logit.predict(coef, X_new=X, y_new=np.ones(3), n_trial_new=np.ones(2))
    with pytest.raises(ValueError, match='n_trial is required'):
        logit.predict(coef, X_new=X, y_new=[0., 2., 1.])
    with pytest.raises(ValueError, match='strictly positive'):
        logit.predict(coef, X_new=X, y_new=np.zeros(3),
                      n_trial_new=[1., 0., 1.])
    with pytest.raises(ValueError, match='n_success exceeds n_trial'):
        logit.predict(coef, X_new=X, y_new=[0., 3., 1.],
                      n_trial_new=[1., 2., 1.])
    with pytest.raises(ValueError, match='finite and non-negative'):
        logit.predict(coef, X_new=X, y_new=[0., -1., 1.],
                      n_trial_new=np.ones(3))
    with pytest.raises(ValueError, match='n_trial_new is an argument of '
                                         'scoring only'):
        logit.predict(coef, X_new=X, n_trial_new=np.ones(3))
    with pytest.raises(ValueError, match='n_trial_new is an argument of new '
                                         'rows only'):
        logit.predict(coef, n_trial_new=np.ones(N))
    # the Poisson model: the constructor's rules
    with pytest.raises(ValueError, match='incompatible sizes'):
        pois.predict(coef, X_new=X, y_new=np.ones(4))
    with pytest.raises(ValueError, match='incompatible sizes'):
        pois.predict(coef, X_new=X, exposure_new=np.ones(4))
    for bad in ([1., -1., 0.], [1., .5, 0.], [1., np.nan, 0.]):
        with pytest.raises(ValueError, match='non-negative integer'):
            pois.predict(coef, X_new=X, y_new=bad)
    for bad in ([1., 0., 1.], [1., -2., 1.], [1., np.inf, 1.]):
        with pytest.raises(ValueError, match='strictly positive and finite'):
            pois.predict(coef, X_new=X, exposure_new=bad)
    with pytest.raises(ValueError, match='exposure_new is an argument of '
                                         'new rows only'):
        pois.predict(coef, exposure_new=np.ones(N))


def test_conditional_poisson_and_adopted_designs_refuse(monkeypatch):
    from bayesbridge_amd import _lib, model
    monkeypatch.setattr(_lib, 'load', lambda: _FakeLib())
    design = _FakeDesign(N, P - 1, intercept=False)
    y = np.ones(N)
    strata = np.repeat(np.arange(3), 4)
    m = model.PoissonModel(y, None, design, strata=strata)
    with pytest.raises(ValueError, match='conditioned away'):
        m.predict(np.zeros((P - 1, S)))
    # a training design adopted from device pointers keeps no offsets
    adopted = _FakeDesign(N, P)
    adopted.column_offset = None
    m = model.PoissonModel(y, None, adopted)
    with pytest.raises(TypeError, match='adopted from device pointers'):
        m.predict(np.zeros((P, S)), X_new=np.zeros((3, P - 1)))


def test_what_predict_hands_to_the_library(monkeypatch):
    """The training rows of a logit model: the family code, the draws
    draw-major, the model's own outcome, the binomial coefficient, and the
    sums of the dict."""
    from ctypes import c_double
    from scipy.special import comb
    from bayesbridge_amd import _lib, model
    seen = {}

    class Lib():
        def bbx_design_predictive_summary(self, h, family, n_draw, coef, tau,
                                          offset, y, m, const, K, mean, sd,
                                          lpd, ll_mean, ll_var, draws):
            def arr(p, length):
                return np.ctypeslib.as_array(
                    (c_double * length).from_address(p.value))
            seen.update(h=h, family=family, n_draw=n_draw, tau=tau,
                        offset=offset, K=K, draws=draws,
                        coef=arr(coef, S * P).copy(), y=arr(y, N).copy(),
                        m=arr(m, N).copy(), const=arr(const, N).copy())
            for k, p in enumerate((mean, sd, lpd, ll_mean, ll_var)):
                arr(p, N)[:] = k + 1.
            return 0

    monkeypatch.setattr(_lib, 'load', lambda: Lib())
    rs = np.random.RandomState(3)
    design = _FakeDesign(N, P)
    trials = rs.randint(1, 5, N).astype(float)
    succ = np.floor(trials * rs.rand(N))
    m = model.LogisticModel(succ, trials, design)
    coef = rs.randn(P, S)
    res = m.predict(coef)
    assert seen['h'] is design.handle and seen['family'] == 1
    assert seen['n_draw'] == S and seen['K'] == 0
    assert seen['tau'] is None and seen['offset'] is None
    assert seen['draws'] is None
    assert np.array_equal(seen['coef'].reshape(S, P), coef.T)
    assert np.array_equal(seen['y'], succ)
    assert np.array_equal(seen['m'], trials)
    assert np.allclose(seen['const'], np.log(comb(trials, succ)), rtol=1e-13)
    assert set(res) == {'mean', 'sd', 'lpd', 'loglik_mean', 'loglik_var',
                        'lppd', 'p_waic', 'waic'}
    assert res['lppd'] == 3. * N and res['p_waic'] == 5. * N
    assert res['waic'] == -2. * (3. * N - 5. * N)


def test_cox_new_design_is_the_shared_helper(monkeypatch):
    """CoxModel._new_design hands the shared helper what it built itself:
    the training design, the rows, no intercept column."""
    from bayesbridge_amd import model
    seen = []
    monkeypatch.setattr(model, '_new_design',
                        lambda *a, **kw: seen.append((a, kw)) or 'design')
    cox = model.CoxModel.__new__(model.CoxModel)
    cox.design = object()
    X = np.zeros((2, 3))
    assert model.CoxModel._new_design(cox, X) == 'design'
    (args, kw), = seen
    assert len(args) == 2 and args[0] is cox.design and args[1] is X
    assert kw == {'add_intercept': False}
    cox._cox = c_void_p()        # (nothing for __del__ to release)


# ---- the C ABI --------------------------------------------------------------

def test_entry_point_is_declared_exported_and_documented():
    from bayesbridge_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    assert re.search(r'\b%s\s*\(' % ENTRY, header)
    for k, name in enumerate(('LINEAR', 'LOGIT', 'POISSON')):
        assert re.search(r'#define BBX_PRED_%s %d\b' % (name, k), header)
        assert getattr(_lib, 'PRED_' + name) == k
    assert ENTRY in _lib.EXPORTED_SYMBOLS
    assert len(_lib._declare(lib)[ENTRY][0]) == 16
    assert getattr(lib, ENTRY).restype is not None
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() == 113
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert ENTRY in doc and 'draws_per_pass' in doc
    makefile = open(os.path.join(ROOT, 'bayes-bridge_amd', 'csrc',
                                 'Makefile')).read()
    assert re.search(r'^SRCS := .*\bpredict\.hip\b', makefile, re.M)


def test_c_call_refuses_a_design_that_is_not_one_without_a_device():
    from bayesbridge_amd import _lib
    lib = _lib.load()
    a = np.zeros(4)
    p = a.ctypes.data_as(c_void_p)
    # a NULL handle, and an address that is no live design's (never read)
    for handle in (None, p):
        assert lib.bbx_design_predictive_summary(
            handle, 1, 1, p, None, None, None, None, None, 0, p, p, None,
            None, None, None) == -1
        assert ENTRY + ': the design is NULL or destroyed' \
            in _lib.last_error()


# ---- the summary kernel's registers -----------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_summary_kernel_does_not_spill(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, 'bayes-bridge_amd', 'csrc', 'predict.hip'),
        tmp_path)
    kernels = [k for k in table if 'predict_summary_kernel' in k]
    # three families, with an outcome and without
    assert len(kernels) == 6 and len(table) == 6, sorted(table)
    for name in kernels:
        res = table[name]
        assert res['VGPRs Spill'] == 0, (name, res)
        assert res['SGPRs Spill'] == 0, (name, res)
        assert res['ScratchSize [bytes/lane]'] == 0, (name, res)
