"""CPU: the host side of Efron's tied event times in the Cox model -- the
oracle's two forms against each other and against central differences, a
closed form, Efron against Breslow, the tie groups against loops, the
ValueErrors, what RegressionModel hands to the library, and the C ABI's
declarations and host-side refusals."""
import math
import os
import re
import warnings
from ctypes import byref, c_int32, c_void_p

import numpy as np
import pytest

import cox_efron_oracle as ceo
from conftest import ROOT

# the tolerances tests/test_hip_cox.py holds the device to against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10
INF = float('inf')


def _sorted_problem(n, p, seed, **kw):
    from bayesbridge_amd.model import cox_preprocess
    X = np.random.RandomState(seed + 1000).randn(n, p)
    event, cens = ceo.grid_times(X, seed, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, X, _ = cox_preprocess(event, cens, X)
    return event, cens, X, ceo.index_arrays(event, cens)


@pytest.mark.parametrize('n,n_grid', [(60, 5), (257, 1), (700, 40),
                                      (300, 100000)])
def test_the_oracles_two_forms_agree(n, n_grid):
    """Several ties per time, all events tied (one grid point) and no ties."""
    event, cens, X, idx = _sorted_problem(n, 6, n, n_grid=n_grid)
    gsize = idx[4]
    if n_grid == 1:
        assert np.all(gsize == idx[0])
    elif n_grid > n:
        assert np.all(gsize == 1)
    else:
        assert gsize.max() > 2 and len(np.unique(gsize)) > 1
    rs = np.random.RandomState(1)
    for scale in (.1, 1.):
        beta, v = rs.randn(6) * scale, rs.randn(6)
        ll, grad = ceo.explicit_loglik_grad(X, beta, event, cens)
        hv = ceo.explicit_hessian_matvec(X, beta, v, event, cens)
        # the scan form in extended precision is the same function
        ll2, grad2 = ceo.scans_loglik_grad(X, beta, idx, np.longdouble)
        hv2 = ceo.scans_hessian_matvec(X, beta, v, idx, np.longdouble)
        assert abs(ll2 - ll) <= 1e-14 * abs(ll)
        assert np.abs(grad2 - grad).max() <= 1e-13 * np.abs(grad).max()
        assert np.abs(hv2 - hv).max() <= 1e-13 * np.abs(hv).max()
        # and in float64 it stays within the device's tolerances
        ll3, grad3 = ceo.scans_loglik_grad(X, beta, idx)
        hv3 = ceo.scans_hessian_matvec(X, beta, v, idx)
        assert abs(ll3 - ll) <= LL_TOL * abs(ll)
        assert np.abs(grad3 - grad).max() <= GRAD_TOL * np.abs(grad).max()
        assert np.abs(hv3 - hv).max() <= HESS_TOL * np.abs(hv).max()


def test_gradient_and_hessian_match_central_differences():
    event, cens, X, idx = _sorted_problem(120, 4, 3, n_grid=6)
    assert idx[4].max() > 3
    rs = np.random.RandomState(2)
    beta, v = rs.randn(4) * .3, rs.randn(4)

    def ll(b):
        return ceo.explicit_loglik(X, b, event, cens)

    def grad(b):
        return ceo.explicit_loglik_grad(X, b, event, cens)[1]

    eps = 1e-5
    fd_grad = np.array([(ll(beta + eps * e) - ll(beta - eps * e)) / (2 * eps)
                        for e in np.eye(4)])
    np.testing.assert_allclose(grad(beta), fd_grad, rtol=1e-6, atol=1e-7)
    fd_hv = (grad(beta + eps * v) - grad(beta - eps * v)) / (2 * eps)
    np.testing.assert_allclose(
        ceo.explicit_hessian_matvec(X, beta, v, event, cens), fd_hv,
        rtol=1e-6, atol=1e-7)
    # the scan form is the same function
    np.testing.assert_allclose(ceo.scans_loglik_grad(X, beta, idx)[1],
                               fd_grad, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(ceo.scans_hessian_matvec(X, beta, v, idx),
                               fd_hv, rtol=1e-6, atol=1e-7)


def test_closed_form_two_tied_events_and_one_censored_row():
    """beta = 0: phi = 3 and 3 - 1/2 2 = 2, loglik = -log 6; Breslow's rule
    gives -2 log 3."""
    event = np.array([1., 1., INF])
    cens = np.array([INF, INF, 2.])
    X = np.array([[1., 0.], [0., 1.], [1., 1.]])
    idx = ceo.index_arrays(event, cens)
    assert list(idx[4]) == [2, 2]
    beta = np.zeros(2)
    for dtype in (np.float64, np.longdouble):
        ll = ceo.scans_loglik_grad(X, beta, idx, dtype)[0]
        assert ll == pytest.approx(-math.log(6.), rel=1e-15)
        br = ceo.scans_loglik_grad(X, beta, idx, dtype, ties='breslow')[0]
        assert br == pytest.approx(-2 * math.log(3.), rel=1e-15)
    assert ceo.explicit_loglik(X, beta, event, cens) \
        == pytest.approx(-math.log(6.), rel=1e-15)


def test_efron_is_at_least_breslow_and_equal_without_ties():
    rs = np.random.RandomState(5)
    event, cens, X, idx = _sorted_problem(400, 5, 7, n_grid=12)
    for scale in (0., .1, 1., 3.):
        beta = rs.randn(5) * scale
        ef = ceo.scans_loglik_grad(X, beta, idx, np.longdouble)[0]
        br = ceo.scans_loglik_grad(X, beta, idx, np.longdouble, 'breslow')[0]
        assert ef > br
    event, cens, X, idx = _sorted_problem(400, 5, 8, n_grid=10 ** 6)
    assert np.all(idx[4] == 1)
    for scale in (0., .1, 1., 3.):
        beta, v = rs.randn(5) * scale, rs.randn(5)
        ef, efg = ceo.scans_loglik_grad(X, beta, idx)
        br, brg = ceo.scans_loglik_grad(X, beta, idx, ties='breslow')
        assert ef >= br - 1e-12 * abs(br)
        assert abs(ef - br) <= 1e-12 * abs(br)
        assert np.abs(efg - brg).max() <= 1e-12 * np.abs(brg).max()
        efh = ceo.scans_hessian_matvec(X, beta, v, idx)
        brh = ceo.scans_hessian_matvec(X, beta, v, idx, ties='breslow')
        assert np.abs(efh - brh).max() <= 1e-12 * np.abs(brh).max()


TIE_DATA = {
    # widths 1, 2 and 7
    'widths': (np.array([1.] + [2.] * 2 + [3.] + [4.] * 7 + [5.]
                        + [INF] * 3),
               np.array([INF] * 12 + [6., 3.5, 1.5])),
    'all_tied': (np.array([2.] * 9 + [INF] * 2),
                 np.array([INF] * 9 + [3., 2.5])),
    # censoring times equal to event times stay inside the risk set
    'censoring_ties': (np.array([1., 2., 2., 3., 3., 3., INF, INF, INF, INF]),
                       np.array([INF] * 6 + [3., 3., 2., 1.])),
}


@pytest.mark.parametrize('name', sorted(TIE_DATA))
def test_tie_groups_match_loops(name):
    from bayesbridge_amd.model import cox_risk_sets, cox_tie_groups
    event, cens = TIE_DATA[name]
    gstart, gsize = cox_tie_groups(event)
    want_start, want_size = ceo.tie_groups_by_loops(event)
    assert np.array_equal(gstart, want_start)
    assert np.array_equal(gsize, want_size)
    n_event, start, end, n_app = cox_risk_sets(event, cens)
    assert len(gstart) == n_event and np.array_equal(gstart, start)
    if name == 'widths':
        assert sorted(set(gsize)) == [1, 2, 7]
    if name == 'all_tied':
        assert np.all(gsize == 9) and np.all(gstart == 0)
    if name == 'censoring_ties':
        x = np.minimum(event, cens)
        for k in range(n_event):
            assert end[k] == max(i for i in range(len(x))
                                 if x[i] >= event[k])
        assert end[0] == 9 and end[1] == 8 and end[3] == 7
    # every n_app ends on a group boundary: what bbx_coxef_create checks
    assert np.all(np.isin(n_app, gstart + gsize))
    # the explicit likelihood on these rows is the scan form's
    X = np.random.RandomState(3).randn(len(event), 2)
    beta = np.array([.4, -.7])
    idx = ceo.index_arrays(event, cens)
    ll, grad = ceo.explicit_loglik_grad(X, beta, event, cens)
    ll2, grad2 = ceo.scans_loglik_grad(X, beta, idx)
    assert abs(ll2 - ll) <= LL_TOL * abs(ll)
    assert np.abs(grad2 - grad).max() <= GRAD_TOL * np.abs(grad).max()
    with pytest.raises(ValueError, match='need to be sorted'):
        cox_tie_groups(event[::-1])


def test_refusals_are_value_errors():
    """All raised before a design is built or the library is called."""
    from bayesbridge_amd import RegressionModel
    from bayesbridge_amd.model import CoxModel
    event, cens = TIE_DATA['widths']
    n = len(event)
    X = np.random.RandomState(0).randn(n, 2)
    strata = np.arange(n) % 2
    entry = np.full(n, -INF)
    for bad in ('exact', 'Efron', None, 1):
        with pytest.raises(ValueError, match="'breslow' or 'efron'"):
            RegressionModel((event, cens), X, 'cox', ties=bad)
        with pytest.raises(ValueError, match="'breslow' or 'efron'"):
            CoxModel(event, cens, None, ties=bad)
    with pytest.raises(ValueError, match='strata is not supported.*not built'):
        RegressionModel((event, cens, strata), X, 'cox', ties='efron')
    with pytest.raises(ValueError,
                       match='entry_time is not supported.*not built'):
        RegressionModel((event, cens), X, 'cox', entry_time=entry,
                        ties='efron')
    with pytest.raises(ValueError, match='strata is not supported.*not built'):
        CoxModel(event, cens, None, strata=strata, ties='efron')
    with pytest.raises(ValueError,
                       match='entry_time is not supported.*not built'):
        CoxModel(event, cens, None, entry_time=entry, ties='efron')
    # entry_time together with strata keeps its own refusal
    for ties in ('breslow', 'efron'):
        with pytest.raises(ValueError, match='entry_time together with strata'):
            RegressionModel((event, cens, strata), X, 'cox',
                            entry_time=entry, ties=ties)
        with pytest.raises(ValueError, match='entry_time together with strata'):
            CoxModel(event, cens, None, strata=strata, entry_time=entry,
                     ties=ties)
    for family, outcome in (('linear', event), ('logit', np.ones(n)),
                            ('poisson', np.ones(n))):
        for ties in ('efron', 'exact'):
            with pytest.raises(ValueError, match="family='cox' only"):
                RegressionModel(outcome, X, family, ties=ties)


class _FakeDesign():
    intercept_added = False
    handle = c_void_p(1)

    def __init__(self, X, **kw):
        self.shape = X.shape


class _FakeLib():
    """Records the create call a model makes, with copies of its three index
    arrays (n_event, n_event and n int32)."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def __getattr__(self, name):
        def fn(*args):
            lengths = (args[1], args[1], self.n)
            arrays = [np.ctypeslib.as_array(
                (c_int32 * length).from_address(a.value)).copy()
                for a, length in zip(args[2:5], lengths)]
            self.calls.append((name, args[1], arrays))
            return 0
        return fn


def _built(monkeypatch, **kw):
    from bayesbridge_amd import RegressionModel, _lib, model
    event, cens = TIE_DATA['widths']
    lib = _FakeLib(len(event))
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    monkeypatch.setattr(model, 'HipDenseDesignMatrix', _FakeDesign)
    X = np.random.RandomState(0).randn(len(event), 2)
    m = RegressionModel((event, cens), X, 'cox', **kw)
    (name, n_event, arrays), = lib.calls
    return m, name, n_event, arrays


def test_breslow_is_the_model_without_the_argument(monkeypatch):
    plain, name, ne, arrays = _built(monkeypatch)
    named, name2, ne2, arrays2 = _built(monkeypatch, ties='breslow')
    assert name == name2 == 'bbx_cox_create' and ne == ne2 == 12
    assert plain._ham_prefix == named._ham_prefix == 'bbx_cox_'
    a, b = vars(plain), vars(named)
    assert set(a) == set(b) and 'tie_group_size' not in a
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        elif key not in ('design', '_cox'):
            assert a[key] == b[key], key
    for x, y in zip(arrays, arrays2):
        assert np.array_equal(x, y)
    # ties='efron': the same rows and arrays on the other handle
    efron, name3, ne3, arrays3 = _built(monkeypatch, ties='efron')
    assert name3 == 'bbx_coxef_create' and ne3 == 12
    assert efron._ham_prefix == 'bbx_coxef_' and efron.name == 'cox'
    assert efron.ties == 'efron' and plain.ties == 'breslow'
    for x, y in zip(arrays, arrays3):
        assert np.array_equal(x, y)
    assert list(efron.tie_group_size) == [1, 2, 2, 1] + [7] * 7 + [1]
    for key in ('n_event', 'risk_set_start_index', 'risk_set_end_index',
                'n_appearance_in_risk_set', 'event_time', 'censoring_time'):
        assert np.array_equal(getattr(efron, key), getattr(plain, key)), key


def test_entry_points_are_declared_and_versions_agree():
    from bayesbridge_amd import _lib
    from ham_cabi import SHARED
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_coxef_[a-z_]+)\s*\(', header))
    assert declared == {'bbx_coxef_%s' % e
                        for e in SHARED + ('create', 'destroy')}
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() == 113
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'bbx_coxef_create' in doc and '!= 113' in doc


def test_null_handles_and_designs_are_refused_on_the_host():
    import ham_cabi as hc
    from bayesbridge_amd import _lib
    lib = _lib.load()
    calls = hc.Calls(lib, 'coxef')
    for name in hc.SHARED:
        assert calls.call(name, None) == (
            hc.ERR_INVALID, 'NULL coxef handle'), name
    assert calls.destroy(None) == hc.OK
    h = c_void_p()
    i32 = np.zeros(4, dtype=np.int32).ctypes.data_as(c_void_p)
    assert lib.bbx_coxef_create(None, 1, i32, i32, i32, byref(h)) == -1
    assert 'invalid design' in _lib.last_error() and not h.value
    assert lib.bbx_coxef_create(None, 1, i32, i32, i32, None) == -1
    assert 'NULL output pointer' in _lib.last_error()
