"""CPU: the host side of the counting-process Cox model -- the oracle's two
forms against each other and against central differences, the preprocessing
and the index arrays against their definitions on awkward data, the
ValueErrors, and the C ABI's declarations and host-side refusals."""
import os
import re
import warnings
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

import cox_interval_oracle as cio
from conftest import ROOT

# the tolerances tests/test_hip_cox.py holds the device to against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10


def _sorted_problem(n, p, seed, **kw):
    from bayesbridge_amd.model import (cox_interval_risk_sets,
                                       cox_preprocess_interval)
    entry, event, cens, X = cio.make_data(n, p, seed, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        entry, event, cens, X, keep = cox_preprocess_interval(
            entry, event, cens, X)
    return entry, event, cens, X, cox_interval_risk_sets(entry, event, cens)


@pytest.mark.parametrize('n,ties', [(60, False), (257, True), (700, False)])
def test_the_oracles_two_forms_agree(n, ties):
    entry, event, cens, X, idx = _sorted_problem(n, 6, n, ties=ties)
    assert np.isfinite(entry).sum() > n // 4       # real delayed entry
    assert np.any(idx[3] < len(event))             # something is subtracted
    mask, evrow = cio.risk_matrix(entry, event, cens)
    assert np.array_equal(evrow, idx[1])
    rs = np.random.RandomState(1)
    for scale in (.1, 1.):
        beta, v = rs.randn(6) * scale, rs.randn(6)
        ll, grad = cio.explicit_loglik_grad(X, beta, mask, evrow)
        hv = cio.explicit_hessian_matvec(X, beta, v, mask, evrow)
        # the scan form in extended precision is the same function
        ll2, grad2 = cio.scans_loglik_grad(X, beta, idx, np.longdouble)
        hv2 = cio.scans_hessian_matvec(X, beta, v, idx, np.longdouble)
        assert abs(ll2 - ll) <= 1e-14 * abs(ll)
        assert np.abs(grad2 - grad).max() <= 1e-13 * np.abs(grad).max()
        assert np.abs(hv2 - hv).max() <= 1e-13 * np.abs(hv).max()
        # and in float64 it stays within the device's tolerances
        ll3, grad3 = cio.scans_loglik_grad(X, beta, idx)
        hv3 = cio.scans_hessian_matvec(X, beta, v, idx)
        assert abs(ll3 - ll) <= LL_TOL * abs(ll)
        assert np.abs(grad3 - grad).max() <= GRAD_TOL * np.abs(grad).max()
        assert np.abs(hv3 - hv).max() <= HESS_TOL * np.abs(hv).max()


def test_gradient_and_hessian_match_central_differences():
    entry, event, cens, X, idx = _sorted_problem(120, 4, 3)
    mask, evrow = cio.risk_matrix(entry, event, cens)
    rs = np.random.RandomState(2)
    beta, v = rs.randn(4) * .3, rs.randn(4)

    def ll(b):
        return cio.explicit_loglik_grad(X, b, mask, evrow)[0]

    def grad(b):
        return cio.explicit_loglik_grad(X, b, mask, evrow)[1]

    eps = 1e-5
    fd_grad = np.array([(ll(beta + eps * e) - ll(beta - eps * e)) / (2 * eps)
                        for e in np.eye(4)])
    np.testing.assert_allclose(grad(beta), fd_grad, rtol=1e-6, atol=1e-7)
    fd_hv = (grad(beta + eps * v) - grad(beta - eps * v)) / (2 * eps)
    np.testing.assert_allclose(
        cio.explicit_hessian_matvec(X, beta, v, mask, evrow), fd_hv,
        rtol=1e-6, atol=1e-7)
    # the scan form is the same function
    np.testing.assert_allclose(cio.scans_loglik_grad(X, beta, idx)[1],
                               fd_grad, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cio.scans_hessian_matvec(X, beta, v, idx),
                               fd_hv, rtol=1e-6, atol=1e-7)


INF = float('inf')
# row: (entry, event, censoring).  Events at 2, 2, 3 and 5.
AWKWARD = np.array([
    (-INF, 5., INF),     # 0 an event, at risk from the start
    (2., 3., INF),       # 1 entry equal to an event time: not at risk at 2
    (-INF, INF, 2.),     # 2 censoring equal to an event time: at risk at 2
    (0., 2., INF),       # 3 a tied event
    (1., 2., INF),       # 4 its twin
    (3., INF, 4.),       # 5 between two events: never at risk (dropped)
    (-INF, INF, 1.),     # 6 censored before the first event (dropped)
    (5., INF, 9.),       # 7 enters at the last event: never at risk (dropped)
    (2.5, INF, 7.),      # 8 at risk at 3 and 5
    (-INF, INF, 3.),     # 9 censored at an event time, sorts after event 1
])


def test_preprocessing_and_index_arrays_on_awkward_rows():
    from bayesbridge_amd.model import (cox_interval_risk_sets,
                                       cox_preprocess_interval)
    entry, event, cens = AWKWARD.T
    X = np.arange(20.).reshape(10, 2)
    with pytest.warns(UserWarning) as rec:
        e, t, c, Xs, keep = cox_preprocess_interval(entry, event, cens, X)
    text = ' '.join(str(w.message) for w in rec)
    assert 'sorted' in text and 'removed' in text
    # by exit time, events before censored rows at an equal exit, stable
    assert list(keep) == [3, 4, 2, 1, 9, 0, 8]
    assert np.array_equal(e, entry[keep]) and np.array_equal(t, event[keep])
    assert np.array_equal(c, cens[keep]) and np.array_equal(Xs, X[keep])
    idx = cox_interval_risk_sets(e, t, c)
    want = cio.index_arrays_by_loops(e, t, c)
    assert idx[0] == want[0] == 4
    for got, ref, name in zip(idx[1:], want[1:], 'evrow a b p q perm'.split()):
        assert np.array_equal(got, ref), (name, got, ref)
    # the index arrays describe exactly the risk sets of the definition
    mask, evrow = cio.risk_matrix(e, t, c)
    n = len(e)
    n_event, evrow2, a, b, p, q, perm = idx
    for k in range(n_event):
        rows = set(range(a[k], n)) - set(perm[b[k]:])
        assert rows == set(np.flatnonzero(mask[k])), k
    assert np.array_equal(p - q, mask.sum(axis=0))
    # original row 1 (entry 2) is not at risk at time 2; row 2 (censored at
    # 2) is
    at2 = set(keep[np.flatnonzero(mask[0])])
    assert 1 not in at2 and 2 in at2 and {3, 4} <= at2
    # idempotent: sorted rows come back unchanged, without a warning
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        e2, t2, c2, X2, keep2 = cox_preprocess_interval(e, t, c, Xs)
    assert np.array_equal(keep2, np.arange(n)) and X2 is Xs
    assert np.array_equal(e2, e) and np.array_equal(t2, t)


@pytest.mark.parametrize('seed', range(4))
def test_index_arrays_match_their_definitions_on_random_ties(seed):
    entry, event, cens, X, idx = _sorted_problem(90, 2, seed, ties=True)
    want = cio.index_arrays_by_loops(entry, event, cens)
    for got, ref in zip(idx, want):
        assert np.array_equal(got, ref)
    assert len(np.unique(event[np.isfinite(event)])) < idx[0]     # tied events


def test_value_errors():
    from bayesbridge_amd.model import (cox_interval_risk_sets,
                                       cox_preprocess_interval)
    entry, event, cens = (x.copy() for x in AWKWARD.T)
    for fn in (cox_preprocess_interval, cox_interval_risk_sets):
        with pytest.raises(ValueError, match='same length'):
            fn(entry[:-1], event, cens)
        with pytest.raises(ValueError, match='same length'):
            fn(entry.reshape(5, 2), event.reshape(5, 2), cens.reshape(5, 2))
        with pytest.raises(ValueError, match='must be infinity'):
            fn(entry, np.where(np.arange(10) == 2, 1.5, event), cens)
        with pytest.raises(ValueError, match='must be infinity'):
            fn(entry, np.full(10, INF), np.full(10, INF))
        with pytest.raises(ValueError, match='strictly before'):
            fn(np.where(np.arange(10) == 0, 5., entry), event, cens)
        with pytest.raises(ValueError, match='strictly before'):
            fn(np.where(np.arange(10) == 2, 2.5, entry), event, cens)
        with pytest.raises(ValueError, match='NaN'):
            fn(np.where(np.arange(10) == 0, np.nan, entry), event, cens)
    # unsorted rows and rows never at risk: the risk-set builder refuses
    with pytest.raises(ValueError, match='need to be sorted'):
        cox_interval_risk_sets(entry, event, cens)
    order = np.lexsort((np.isinf(event), np.minimum(event, cens)))
    with pytest.raises(ValueError, match='never appear in the risk set'):
        cox_interval_risk_sets(entry[order], event[order], cens[order])
    # a censored row ahead of an event at the same time
    with pytest.raises(ValueError, match='need to be sorted'):
        cox_interval_risk_sets(np.full(2, -INF), np.array([INF, 1.]),
                               np.array([1., INF]))


def test_entry_points_are_declared_and_versions_agree():
    from bayesbridge_amd import _lib
    from ham_cabi import SHARED
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_coxcp_[a-z_]+)\s*\(', header))
    assert declared == {'bbx_coxcp_%s' % e
                        for e in SHARED + ('create', 'destroy')}
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 112
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'bbx_coxcp_create' in doc


def test_null_handles_and_designs_are_refused_on_the_host():
    from bayesbridge_amd import _lib
    lib = _lib.load()
    vec, ll, h = np.zeros(3), c_double(), c_void_p()
    ptr = vec.ctypes.data_as(c_void_p)
    assert lib.bbx_coxcp_loglik_grad(None, ptr, byref(ll), None) == -1
    assert 'NULL coxcp handle' in _lib.last_error()
    assert lib.bbx_coxcp_set_location(None, ptr) == -1
    assert lib.bbx_coxcp_nuts_sample(None, None, byref(ll), None) == -1
    assert lib.bbx_coxcp_destroy(None) == 0
    i32 = np.zeros(4, dtype=np.int32).ctypes.data_as(c_void_p)
    assert lib.bbx_coxcp_create(None, 1, i32, i32, i32, i32, i32, i32,
                                byref(h)) == -1
    assert 'invalid design' in _lib.last_error() and not h.value
    assert lib.bbx_coxcp_create(None, 1, i32, i32, i32, i32, i32, i32,
                                None) == -1
    assert 'NULL output pointer' in _lib.last_error()
