"""CPU: the host side of case weights in the Cox model -- the oracle's two
forms against each other and against central differences, unit weights and
integer weights against the plain oracle, the ValueErrors, what
RegressionModel hands to the library on shuffled rows, and the C ABI's
declarations and host-side refusals."""
import os
import re
import warnings
from ctypes import byref, c_double, c_int32, c_void_p

import numpy as np
import pytest

import cox_oracle as co
import cox_weighted_oracle as cwo
from conftest import ROOT

# the tolerances tests/test_hip_cox.py holds the device to against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10
INF = float('inf')


def _sorted_problem(n, p, seed, weights='lognormal', **kw):
    """Rows in the model's order, with their weights."""
    from bayesbridge_amd.model import cox_preprocess
    rs = np.random.RandomState(seed + 1000)
    X = rs.randn(n, p)
    if weights == 'lognormal':
        a = np.exp(rs.randn(n))
    elif weights == 'integer':
        a = rs.randint(1, 4, n).astype(np.float64)
    else:
        a = np.ones(n)
    event, cens = cwo.make_times(X, seed, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, X, keep = cox_preprocess(event, cens, X)
    return event, cens, X, cwo.index_arrays(event, cens, a[keep])


@pytest.mark.parametrize('n,n_grid', [(60, 5), (257, 1), (700, 40),
                                      (300, None)])
def test_the_oracles_two_forms_agree(n, n_grid):
    """Several ties per time, all events tied (one grid point) and no ties."""
    event, cens, X, idx = _sorted_problem(n, 6, n, n_grid=n_grid)
    a = idx[4]
    assert a.max() / a.min() > 20
    rs = np.random.RandomState(1)
    for scale in (.1, 1.):
        beta, v = rs.randn(6) * scale, rs.randn(6)
        ll, grad = cwo.explicit_loglik_grad(X, beta, event, cens, a)
        assert ll == cwo.explicit_loglik(X, beta, event, cens, a)
        hv = cwo.explicit_hessian_matvec(X, beta, v, event, cens, a)
        # the scan form in extended precision is the same function
        ll2, grad2 = cwo.scans_loglik_grad(X, beta, idx, np.longdouble)
        hv2 = cwo.scans_hessian_matvec(X, beta, v, idx, np.longdouble)
        assert abs(ll2 - ll) <= 1e-14 * abs(ll)
        assert np.abs(grad2 - grad).max() <= 1e-13 * np.abs(grad).max()
        assert np.abs(hv2 - hv).max() <= 1e-13 * np.abs(hv).max()
        # and in float64 it stays within the device's tolerances
        ll3, grad3 = cwo.scans_loglik_grad(X, beta, idx)
        hv3 = cwo.scans_hessian_matvec(X, beta, v, idx)
        assert abs(ll3 - ll) <= LL_TOL * abs(ll)
        assert np.abs(grad3 - grad).max() <= GRAD_TOL * np.abs(grad).max()
        assert np.abs(hv3 - hv).max() <= HESS_TOL * np.abs(hv).max()


def test_gradient_and_hessian_match_central_differences():
    event, cens, X, idx = _sorted_problem(120, 4, 3, n_grid=6)
    a = idx[4]
    rs = np.random.RandomState(2)
    beta, v = rs.randn(4) * .3, rs.randn(4)

    def ll(b):
        return cwo.explicit_loglik(X, b, event, cens, a)

    def grad(b):
        return cwo.explicit_loglik_grad(X, b, event, cens, a)[1]

    eps = 1e-5
    fd_grad = np.array([(ll(beta + eps * e) - ll(beta - eps * e)) / (2 * eps)
                        for e in np.eye(4)])
    np.testing.assert_allclose(grad(beta), fd_grad, rtol=1e-6, atol=1e-7)
    fd_hv = (grad(beta + eps * v) - grad(beta - eps * v)) / (2 * eps)
    np.testing.assert_allclose(
        cwo.explicit_hessian_matvec(X, beta, v, event, cens, a), fd_hv,
        rtol=1e-6, atol=1e-7)
    # the scan form is the same function
    np.testing.assert_allclose(cwo.scans_loglik_grad(X, beta, idx)[1],
                               fd_grad, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cwo.scans_hessian_matvec(X, beta, v, idx),
                               fd_hv, rtol=1e-6, atol=1e-7)


def test_closed_form_two_events_and_one_censored_row():
    """beta = 0, weights (2, 3, 5), distinct times: H = 10 and 8, loglik =
    -2 log 10 - 3 log 8."""
    event = np.array([1., 2., INF])
    cens = np.array([INF, INF, 3.])
    X = np.array([[1., 0.], [0., 1.], [1., 1.]])
    a = np.array([2., 3., 5.])
    idx = cwo.index_arrays(event, cens, a)
    want = -2 * np.log(10.) - 3 * np.log(8.)
    for dtype in (np.float64, np.longdouble):
        ll = cwo.scans_loglik_grad(X, np.zeros(2), idx, dtype)[0]
        assert ll == pytest.approx(want, rel=1e-15)
    assert cwo.explicit_loglik(X, np.zeros(2), event, cens, a) \
        == pytest.approx(want, rel=1e-15)


def test_unit_weights_give_the_plain_oracle():
    """Every product by a weight of 1 is exact: the same bits."""
    event, cens, X, idx = _sorted_problem(500, 5, 4, weights='unit', n_grid=25)
    rs = np.random.RandomState(3)
    for scale in (.1, 1.):
        beta, v = rs.randn(5) * scale, rs.randn(5)
        ll, grad = cwo.scans_loglik_grad(X, beta, idx)
        pll, pgrad = co.loglik_grad(X, beta, *idx[:4])
        assert ll == pll and np.array_equal(grad, pgrad)
        hv = cwo.scans_hessian_matvec(X, beta, v, idx)
        phv = co.hessian_matvec(X, beta, v, *idx[:4])
        assert np.abs(hv - phv).max() <= 1e-13 * np.abs(phv).max()
        bll, bgrad = co.brute_loglik_grad(X, beta, *idx[:3])
        ell, egrad = cwo.explicit_loglik_grad(X, beta, event, cens, idx[4])
        assert abs(ell - bll) <= 1e-12 * abs(bll)
        assert np.abs(egrad - bgrad).max() <= 1e-12 * np.abs(bgrad).max()


# widths 1, 2 and 7; censoring times equal to event times stay in the risk set
TIED = (np.array([1.] + [2.] * 2 + [3.] + [4.] * 7 + [5.] + [INF] * 5),
        np.array([INF] * 12 + [6., 4., 4., 2., 1.5]))


@pytest.mark.parametrize('data', ['tied', 'grid', 'continuous'])
def test_integer_weights_are_replicated_rows(data):
    """Weights in {1, 2, 3}: the plain oracle's values on the rows written
    that many times; under Breslow's rule the copies of an event share one
    risk set."""
    from bayesbridge_amd.model import cox_risk_sets
    rs = np.random.RandomState(6)
    if data == 'tied':
        event, cens = TIED
        X = rs.randn(len(event), 3)
        a = rs.randint(1, 4, len(event)).astype(np.float64)
        idx = cwo.index_arrays(event, cens, a)
    else:
        event, cens, X, idx = _sorted_problem(
            400, 3, 5, weights='integer',
            n_grid=15 if data == 'grid' else None)
        a = idx[4]
    assert set(a) == {1., 2., 3.}
    if data != 'continuous':
        assert np.intersect1d(event, cens).size
        assert np.any(idx[1] != np.arange(idx[0]))
    revent, rcens, rX = cwo.replicate(event, cens, X, a)
    assert len(revent) == int(a.sum())
    risk = cox_risk_sets(revent, rcens)
    # the copies of event k share risk set k
    assert risk[0] == int(a[:idx[0]].sum())
    for scale in (.2, 1.):
        beta, v = rs.randn(3) * scale, rs.randn(3)
        pll, pgrad = co.loglik_grad(rX, beta, *risk)
        phv = co.hessian_matvec(rX, beta, v, *risk, dtype=np.longdouble)
        for dtype in (np.float64, np.longdouble):
            ll, grad = cwo.scans_loglik_grad(X, beta, idx, dtype)
            hv = cwo.scans_hessian_matvec(X, beta, v, idx, dtype)
            assert abs(ll - pll) <= LL_TOL * abs(pll)
            assert np.abs(grad - pgrad).max() <= GRAD_TOL * np.abs(pgrad).max()
            assert np.abs(hv - phv).max() <= HESS_TOL * np.abs(phv).max()
        ell, egrad = cwo.explicit_loglik_grad(X, beta, event, cens, a)
        assert abs(ell - pll) <= LL_TOL * abs(pll)
        assert np.abs(egrad - pgrad).max() <= GRAD_TOL * np.abs(pgrad).max()


def test_refusals_are_value_errors():
    """All raised before a design is built or the library is called."""
    from bayesbridge_amd import RegressionModel
    from bayesbridge_amd.model import CoxModel
    event, cens = TIED
    n = len(event)
    X = np.random.RandomState(0).randn(n, 2)
    good = np.linspace(.5, 2., n)
    strata = np.arange(n) % 2
    entry = np.full(n, -INF)

    def both(match, weights, outcome=(event, cens), **kw):
        with pytest.raises(ValueError, match=match):
            RegressionModel(outcome, X, 'cox', weights=weights, **kw)
        with pytest.raises(ValueError, match=match):
            CoxModel(event, cens, None, weights=weights,
                     strata=outcome[2] if len(outcome) == 3 else None, **kw)

    for bad in (good[:-1], np.append(good, 1.), good.reshape(1, n),
                good.reshape(n, 1), 1.5, np.empty(0)):
        both('one weight for each observation', bad)
    for value in (np.nan, INF, -INF, 0., -1., -1e-300):
        bad = good.copy()
        bad[5] = value
        both('strictly positive and finite', bad)
    both('weights together with strata is not supported.*not built', good,
         outcome=(event, cens, strata))
    both('weights together with entry_time is not supported.*not built', good,
         entry_time=entry)
    both("weights together with ties='efron' is not supported.*not built",
         good, ties='efron')
    for family, outcome in (('linear', event), ('logit', np.ones(n)),
                            ('poisson', np.ones(n))):
        with pytest.raises(ValueError,
                           match="weights is an argument of family='cox' "
                                 "only"):
            RegressionModel(outcome, X, family, weights=good)
    # the refusals that were there before keep their precedence and wording
    with pytest.raises(ValueError, match="'breslow' or 'efron'"):
        RegressionModel((event, cens), X, 'cox', ties='exact', weights=good)
    with pytest.raises(ValueError, match='entry_time together with strata'):
        RegressionModel((event, cens, strata), X, 'cox', entry_time=entry,
                        weights=good)


class _FakeDesign():
    intercept_added = False
    handle = c_void_p(1)

    def __init__(self, X, **kw):
        self.shape = X.shape
        self.X = X


class _FakeLib():
    """Records the create call a model makes, with copies of its three index
    arrays (n_event, n_event and n int32) and, for bbx_coxw_create, of the n
    weights."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            n = self.n
            arrays = [np.ctypeslib.as_array(
                (c_int32 * length).from_address(a.value)).copy()
                for a, length in zip(args[2:5], (args[1], args[1], n))]
            weights = None
            if name == 'bbx_coxw_create':
                assert len(args) == 7
                weights = np.ctypeslib.as_array(
                    (c_double * n).from_address(args[5].value)).copy()
            else:
                assert len(args) == 6
            self.calls.append((name, args[1], arrays, weights))
            return 0
        return fn


def _built(monkeypatch, event, cens, X, n_kept, **kw):
    from bayesbridge_amd import RegressionModel, _lib, model
    lib = _FakeLib()
    lib.n = n_kept
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    monkeypatch.setattr(model, 'HipDenseDesignMatrix', _FakeDesign)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = RegressionModel((event, cens), X, 'cox', **kw)
    (name, n_event, arrays, weights), = lib.calls
    return m, name, n_event, arrays, weights


def test_regression_model_permutes_and_prunes_the_weights(monkeypatch):
    """Shuffled rows, three of them censored before the first event: the
    weights travel with their rows and those of the pruned rows go."""
    event, cens = (t.copy() for t in TIED)
    event = np.concatenate((event, [INF] * 3))
    cens = np.concatenate((cens, [.5, .25, .75]))
    n = len(event)
    rs = np.random.RandomState(4)
    X = rs.randn(n, 2)
    # the weight of a row is a tag of the row: 1000 + its first predictor
    a = 1000. + X[:, 0]
    shuffle = rs.permutation(n)
    m, name, ne, arrays, sent = _built(
        monkeypatch, event[shuffle], cens[shuffle], X[shuffle], n - 3,
        weights=a[shuffle])
    assert name == 'bbx_coxw_create' and ne == 12
    assert m._ham_prefix == 'bbx_coxw_' and m.name == 'cox'
    assert m.ties == 'breslow' and m.strata is None and m.entry_time is None
    assert m.n_obs == n - 3 and len(sent) == n - 3
    assert np.array_equal(sent, m.weights)
    assert np.array_equal(m.weights, 1000. + m.design.X[:, 0])
    assert np.array_equal(m.event_time[:12], TIED[0][:12])
    assert np.all(m.censoring_time[12:] >= 1.)
    assert not np.isin(1000. + X[n - 3:, 0], m.weights).any()
    # the index arrays are the plain model's of the same rows
    p, pname, pne, parrays, none = _built(
        monkeypatch, event[shuffle], cens[shuffle], X[shuffle], n - 3)
    assert pname == 'bbx_cox_create' and pne == ne and none is None
    for x, y in zip(arrays, parrays):
        assert np.array_equal(x, y)
    # the caller's array is not kept: changing it later changes nothing
    given = a[:n - 3].copy()
    m2 = _built(monkeypatch, event[:n - 3], cens[:n - 3], X[:n - 3], n - 3,
                weights=given)[0]
    given[:] = -1.
    assert np.array_equal(m2.weights, a[:n - 3])


def test_no_weights_is_the_model_without_the_argument(monkeypatch):
    event, cens = TIED
    X = np.random.RandomState(0).randn(len(event), 2)
    n = len(event)
    plain, name, ne, arrays, w = _built(monkeypatch, event, cens, X, n)
    named, name2, ne2, arrays2, w2 = _built(monkeypatch, event, cens, X, n,
                                            weights=None)
    assert name == name2 == 'bbx_cox_create' and ne == ne2 == 12
    assert w is None and w2 is None
    assert plain._ham_prefix == named._ham_prefix == 'bbx_cox_'
    assert plain.weights is None and named.weights is None
    a, b = vars(plain), vars(named)
    assert set(a) == set(b)
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        elif key not in ('design', '_cox'):
            assert a[key] == b[key], key
    for x, y in zip(arrays, arrays2):
        assert np.array_equal(x, y)
    # and the arrays are cox_risk_sets' of these rows
    from bayesbridge_amd.model import cox_risk_sets
    for x, y in zip(arrays, cox_risk_sets(event, cens)[1:]):
        assert np.array_equal(x, y)


def test_entry_points_are_declared_and_exported():
    from bayesbridge_amd import _lib
    from ham_cabi import SHARED
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_coxw_[a-z_]+)\s*\(', header))
    assert declared == {'bbx_coxw_%s' % e
                        for e in SHARED + ('create', 'destroy')}
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 113
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'bbx_coxw_create' in doc


def test_null_handles_and_designs_are_refused_on_the_host():
    import ham_cabi as hc
    from bayesbridge_amd import _lib
    lib = _lib.load()
    calls = hc.Calls(lib, 'coxw')
    for name in hc.SHARED:
        assert calls.call(name, None) == (
            hc.ERR_INVALID, 'NULL coxw handle'), name
    assert calls.destroy(None) == hc.OK
    h = c_void_p()
    i32 = np.zeros(4, dtype=np.int32).ctypes.data_as(c_void_p)
    f64 = np.ones(4).ctypes.data_as(c_void_p)
    assert lib.bbx_coxw_create(None, 1, i32, i32, i32, f64, byref(h)) == -1
    assert 'invalid design' in _lib.last_error() and not h.value
    assert lib.bbx_coxw_create(None, 1, i32, i32, i32, f64, None) == -1
    assert 'NULL output pointer' in _lib.last_error()
