"""CPU: the host side of the Fine-Gray competing-risks model -- the oracle's
two forms against each other, against central differences and against a
likelihood worked out by hand; the identities with the plain Cox likelihood
(no competing rows; no censored rows, where G = 1); the censoring survivor
function taken from the left and on all the rows given; the preprocessing
and the index arrays against their definitions; the ValueErrors; the C ABI's
declarations and host-side refusals."""
import math
import os
import re
import warnings
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

import cox_finegray_oracle as cfo
import cox_interval_oracle as cio
from conftest import ROOT

# the tolerances tests/test_hip_cox.py holds the device to against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10
INF = float('inf')


def _sorted_problem(n, p, seed, **kw):
    """(sorted event, censoring, competing, X, idx from the model's own
    functions, the unsorted times)."""
    from bayesbridge_amd.model import (cox_finegray_risk_sets,
                                       cox_preprocess_finegray)
    X = np.random.RandomState(seed + 1000).randn(n, p)
    full = cfo.make_times(X, seed, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, comp, X, keep, g, r = cox_preprocess_finegray(*full, X)
    idx = cox_finegray_risk_sets(event, cens, comp) + (g, r)
    return event, cens, comp, X, idx, full


@pytest.mark.parametrize('n,n_grid', [(60, None), (257, 20), (700, 40)])
def test_the_oracles_two_forms_agree(n, n_grid):
    event, cens, comp, X, idx, full = _sorted_problem(n, 6, n, n_grid=n_grid)
    assert len(idx[5]) > n // 5 and idx[0] > n // 5      # real competing rows
    assert idx[6].min() < .9 and np.any(idx[3] > 0)      # real censoring
    W, evrow = cfo.weight_matrix(event, cens, comp, full)
    assert np.array_equal(evrow, idx[1])
    assert np.any((W > 0) & (W < 1))
    rs = np.random.RandomState(1)
    for scale in (.1, 1.):
        beta, v = rs.randn(6) * scale, rs.randn(6)
        ll, grad = cfo.explicit_loglik_grad(X, beta, W, evrow)
        hv = cfo.explicit_hessian_matvec(X, beta, v, W, evrow)
        # the scan form in extended precision is the same function (g and r
        # are the model's float64 ones: a relative 1e-16 each)
        ll2, grad2 = cfo.scans_loglik_grad(X, beta, idx, np.longdouble)
        hv2 = cfo.scans_hessian_matvec(X, beta, v, idx, np.longdouble)
        assert abs(ll2 - ll) <= 1e-13 * abs(ll)
        assert np.abs(grad2 - grad).max() <= 1e-13 * np.abs(grad).max()
        assert np.abs(hv2 - hv).max() <= 1e-13 * np.abs(hv).max()
        # and in float64 it stays within the device's tolerances
        ll3, grad3 = cfo.scans_loglik_grad(X, beta, idx)
        hv3 = cfo.scans_hessian_matvec(X, beta, v, idx)
        assert abs(ll3 - ll) <= LL_TOL * abs(ll)
        assert np.abs(grad3 - grad).max() <= GRAD_TOL * np.abs(grad).max()
        assert np.abs(hv3 - hv).max() <= HESS_TOL * np.abs(hv).max()


def test_gradient_and_hessian_match_central_differences():
    event, cens, comp, X, idx, full = _sorted_problem(120, 4, 3, n_grid=15)
    W, evrow = cfo.weight_matrix(event, cens, comp, full)
    rs = np.random.RandomState(2)
    beta, v = rs.randn(4) * .3, rs.randn(4)

    def ll(b):
        return cfo.explicit_loglik_grad(X, b, W, evrow)[0]

    def grad(b):
        return cfo.explicit_loglik_grad(X, b, W, evrow)[1]

    eps = 1e-5
    fd_grad = np.array([(ll(beta + eps * e) - ll(beta - eps * e)) / (2 * eps)
                        for e in np.eye(4)])
    np.testing.assert_allclose(grad(beta), fd_grad, rtol=1e-6, atol=1e-7)
    fd_hv = (grad(beta + eps * v) - grad(beta - eps * v)) / (2 * eps)
    np.testing.assert_allclose(
        cfo.explicit_hessian_matvec(X, beta, v, W, evrow), fd_hv,
        rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cfo.scans_loglik_grad(X, beta, idx)[1],
                               fd_grad, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cfo.scans_hessian_matvec(X, beta, v, idx),
                               fd_hv, rtol=1e-6, atol=1e-7)


# row: (event, censoring, competing), unsorted
FOUR = np.array([
    (3., INF, INF),      # 0 D: the last event
    (INF, 2., INF),      # 1 B: censored at the time of event C
    (INF, INF, 1.),      # 2 A: a competing event before everything
    (2., INF, INF),      # 3 C: an event tied with the censoring time
])


def test_four_rows_by_hand_pin_the_left_limit():
    """One censoring time, 2, with Y(2) = 3 rows (B, C, D): G(s-) = 1 for
    s <= 2 and 2/3 beyond.  The event at 2 sees G(2-) = 1 -- the censoring AT 2
    is not before it -- so A stays with weight 1 / G(1-) = 1; the event at 3
    sees G(3-) = 2/3, so A stays with weight 2/3:
        H_C = h_A + h_B + h_C + h_D,   H_D = h_D + (2/3) h_A.
    A right-continuous G would give A the weight 2/3 at the event at 2."""
    from bayesbridge_amd.model import (cox_finegray_censoring_survivor,
                                       cox_finegray_risk_sets,
                                       cox_preprocess_finegray)
    event, cens, comp = FOUR.T
    x = np.array([.7, -.4, 1.1, .2])           # D, B, A, C
    X = x[:, None]
    np.testing.assert_allclose(
        cox_finegray_censoring_survivor(event, cens, comp),
        [2 / 3, 1., 1., 1.], rtol=1e-15)
    with pytest.warns(UserWarning, match='sorted'):
        e, c, k, Xs, keep, g, r = cox_preprocess_finegray(event, cens, comp, X)
    assert list(keep) == [2, 3, 1, 0]          # A, C, B, D
    np.testing.assert_allclose(g, [1., 2 / 3], rtol=1e-15)
    assert g[0] == 1. and np.array_equal(r, [1.])
    idx = cox_finegray_risk_sets(e, c, k) + (g, r)
    assert idx[0] == 2 and list(idx[1]) == [1, 3]
    assert list(idx[2]) == [1, 3] and list(idx[3]) == [1, 1]
    assert list(idx[4]) == [0, 1, 1, 2] and list(idx[5]) == [0]
    W, evrow = cfo.weight_matrix(e, c, k)
    np.testing.assert_allclose(W.astype(np.float64),
                               [[1., 1., 1., 1.], [2 / 3, 0., 0., 1.]],
                               rtol=1e-15)
    b = .9
    hD, hB, hA, hC = np.exp(b * x)
    H_C, H_D = hA + hB + hC + hD, hD + (2 / 3) * hA
    want_ll = b * x[3] - math.log(H_C) + b * x[0] - math.log(H_D)
    want_grad = (x[3] + x[0]
                 - (x[2] * hA + x[1] * hB + x[3] * hC + x[0] * hD) / H_C
                 - (x[0] * hD + x[2] * (2 / 3) * hA) / H_D)

    def var(ws, xs):
        ws = np.array(ws) / np.sum(ws)
        return np.sum(ws * np.array(xs) ** 2) - np.sum(ws * np.array(xs)) ** 2

    want_hess = -(var([hA, hB, hC, hD], [x[2], x[1], x[3], x[0]])
                  + var([hD, (2 / 3) * hA], [x[0], x[2]]))
    beta, one = np.array([b]), np.array([1.])
    for ll, grad, hv in (
            cfo.explicit_loglik_grad(Xs, beta, W, evrow)
            + (cfo.explicit_hessian_matvec(Xs, beta, one, W, evrow),),
            cfo.scans_loglik_grad(Xs, beta, idx)
            + (cfo.scans_hessian_matvec(Xs, beta, one, idx),)):
        assert ll == pytest.approx(want_ll, rel=1e-14)
        assert grad[0] == pytest.approx(want_grad, rel=1e-12)
        assert hv[0] == pytest.approx(want_hess, rel=1e-12)


def _plain(X, beta, v, event, cens):
    """The plain Cox likelihood (Breslow): the counting-process oracle with
    every row at risk from the start; rows sorted by time here."""
    order = np.lexsort((np.isinf(event), np.minimum(event, cens)))
    event, cens, X = event[order], cens[order], X[order]
    mask, evrow = cio.risk_matrix(np.full(len(event), -INF), event, cens)
    return cio.explicit_loglik_grad(X, beta, mask, evrow) + (
        cio.explicit_hessian_matvec(X, beta, v, mask, evrow),)


def _finegray(X, beta, v, idx):
    return cfo.scans_loglik_grad(X, beta, idx, np.longdouble) + (
        cfo.scans_hessian_matvec(X, beta, v, idx, np.longdouble),)


def _close(got, want, tol=1e-13):
    assert abs(got[0] - want[0]) <= tol * abs(want[0])
    for g, w in zip(got[1:], want[1:]):
        assert np.abs(g - w).max() <= tol * np.abs(w).max()


def test_without_competing_rows_it_is_the_plain_likelihood():
    event, cens, comp, X, idx, _ = _sorted_problem(300, 5, 4, n_grid=25,
                                                   fracs=(0., .4))
    assert len(idx[5]) == 0 and not np.any(idx[3]) and idx[6].min() < .9
    rs = np.random.RandomState(3)
    beta, v = rs.randn(5) * .5, rs.randn(5)
    _close(_finegray(X, beta, v, idx), _plain(X, beta, v, event, cens))


def test_without_censored_rows_G_is_one_and_competing_rows_never_leave():
    """No censoring: G = 1, a competing row stays in every later risk set with
    weight 1 -- the plain likelihood with every competing row censored after
    the last event."""
    event, cens, comp, X, idx, _ = _sorted_problem(300, 5, 5, n_grid=25,
                                                   fracs=(.5, 0.))
    assert len(idx[5]) > 100 and np.all(np.isinf(cens))
    assert np.all(idx[6] == 1.) and np.all(idx[7] == 1.)
    last = event[np.isfinite(event)].max()
    recoded = np.where(np.isfinite(comp), last + 1., INF)
    rs = np.random.RandomState(3)
    beta, v = rs.randn(5) * .5, rs.randn(5)
    want = _plain(X, beta, v, event, recoded)
    _close(_finegray(X, beta, v, idx), want)
    W, evrow = cfo.weight_matrix(event, cens, comp)
    _close(cfo.explicit_loglik_grad(X, beta, W, evrow)
           + (cfo.explicit_hessian_matvec(X, beta, v, W, evrow),), want)
    # in float64 too: every product by g = r = 1 is exact
    f64 = cfo.scans_loglik_grad(X, beta, idx)
    order = np.lexsort((np.isinf(event), np.minimum(event, recoded)))
    pidx = _plain_idx(event[order], recoded[order])
    p64 = cio.scans_loglik_grad(X[order], beta, pidx)
    assert f64[0] == pytest.approx(p64[0], rel=1e-13)
    np.testing.assert_allclose(f64[1], p64[1], rtol=1e-11, atol=1e-12)


def _plain_idx(event, cens):
    from bayesbridge_amd.model import cox_interval_risk_sets
    return cox_interval_risk_sets(np.full(len(event), -INF), event, cens)


# (event, censoring, competing): a competing event, then a row censored
# before the first event (dropped), then events and a late censoring
EARLY = np.array([
    (INF, INF, 1.),      # 0 competing before the early censoring
    (INF, 2., INF),      # 1 censored before the first event: dropped
    (3., INF, INF),      # 2
    (INF, INF, 3.5),     # 3 competing between the events
    (INF, 4., INF),      # 4
    (5., INF, INF),      # 5
    (6., INF, INF),      # 6
])


def test_G_is_estimated_before_uninformative_rows_are_dropped():
    """Row 1 is censored at 2, before the first event, and is dropped; its
    factor 1 - 1/6 stays in G(t-) of every event but not in G(1-) of row 0,
    so row 0's weights keep it.  Estimating G after the drop would lose it."""
    from bayesbridge_amd.model import (cox_finegray_censoring_survivor,
                                       cox_finegray_risk_sets,
                                       cox_preprocess_finegray)
    event, cens, comp = EARLY.T
    X = np.random.RandomState(0).randn(7, 2)
    with pytest.warns(UserWarning, match='removed'):
        e, c, k, Xs, keep, g, r = cox_preprocess_finegray(event, cens, comp, X)
    assert list(keep) == [0, 2, 3, 4, 5, 6]
    # G(s-): 1 up to 2, 5/6 up to 4, 5/6 * 2/3 beyond
    np.testing.assert_allclose(g, [5 / 6, 5 / 9, 5 / 9], rtol=1e-15)
    np.testing.assert_allclose(r, [1., 6 / 5], rtol=1e-15)
    after = cox_finegray_censoring_survivor(e, c, k)
    np.testing.assert_allclose(after[[1, 4, 5]], [1., 2 / 3, 2 / 3],
                               rtol=1e-15)
    idx = cox_finegray_risk_sets(e, c, k) + (g, r)
    W, evrow = cfo.weight_matrix(e, c, k, full=(event, cens, comp))
    W_after, _ = cfo.weight_matrix(e, c, k)
    np.testing.assert_allclose(W[:, 0].astype(float), [5 / 6, 5 / 9, 5 / 9],
                               rtol=1e-15)
    np.testing.assert_allclose(W_after[:, 0].astype(float), [1., 2 / 3, 2 / 3],
                               rtol=1e-15)
    beta, v = np.array([.4, -.7]), np.array([1., .5])
    want = cfo.explicit_loglik_grad(Xs, beta, W, evrow) + (
        cfo.explicit_hessian_matvec(Xs, beta, v, W, evrow),)
    wrong = cfo.explicit_loglik_grad(Xs, beta, W_after, evrow)
    _close(_finegray(Xs, beta, v, idx), want)
    assert abs(wrong[0] - want[0]) > 1e-3 * abs(want[0])
    # the oracle's own index arrays and factors are the model's
    for got, ref in zip(idx, cfo.index_arrays(e, c, k,
                                              full=(event, cens, comp))):
        np.testing.assert_allclose(got, ref, rtol=1e-15)


@pytest.mark.parametrize('seed', range(4))
def test_preprocessing_permutes_and_prunes_consistently(seed):
    from bayesbridge_amd.model import (cox_finegray_risk_sets,
                                       cox_preprocess_finegray)
    n = 90
    X = np.random.RandomState(seed).randn(n, 2)
    full = cfo.make_times(X, seed, n_grid=12)
    # some rows censored before the first event
    first = np.min(full[0])
    early = np.flatnonzero(np.isfinite(full[1]))[:3]
    full[1][early] = first - 1.
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        e, c, k, Xs, keep, g, r = cox_preprocess_finegray(*full, X)
    assert len(keep) == n - 3 and not set(early) & set(keep)
    assert len(set(keep)) == len(keep)
    for got, orig in zip((e, c, k, Xs), full + (X,)):
        assert np.array_equal(got, orig[keep])
    T, status = cfo.times_and_status(e, c, k)
    assert np.all(np.diff(T) >= 0)
    assert np.all((np.diff(T) > 0) | (np.diff(status) >= 0))
    # stable: rows that tie in time and status keep their order
    tied = (np.diff(T) == 0) & (np.diff(status) == 0)
    assert tied.any() and np.all(np.diff(keep)[tied] > 0)
    # competing rows are never dropped
    assert np.sum(np.isfinite(k)) == np.sum(np.isfinite(full[2]))
    idx = cox_finegray_risk_sets(e, c, k) + (g, r)
    want = cfo.index_arrays(e, c, k, full=full)
    names = 'ne evrow a b p comp_row g r'.split()
    for got, ref, name in zip(idx, want, names):
        np.testing.assert_allclose(got, ref, rtol=1e-14, err_msg=name)
    assert len(np.unique(e[np.isfinite(e)])) < idx[0]          # tied events
    # the index arrays describe exactly the weights of the definition
    W, evrow = cfo.weight_matrix(e, c, k, full=full)
    W2 = np.zeros(W.shape)
    for j in range(idx[0]):
        W2[j, idx[2][j]:] = 1.
        rows = idx[5][:idx[3][j]]
        W2[j, rows] = g[j] * r[:idx[3][j]]
    np.testing.assert_allclose(W2, W.astype(float), rtol=1e-14)
    # idempotent: sorted rows come back unchanged, without a warning
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        e2, c2, k2, X2, keep2, _, _ = cox_preprocess_finegray(e, c, k, Xs)
    assert np.array_equal(keep2, np.arange(len(e))) and X2 is Xs
    assert np.array_equal(e2, e) and np.array_equal(k2, k)


def test_value_errors():
    from bayesbridge_amd import RegressionModel
    from bayesbridge_amd.model import (CoxModel, cox_finegray_risk_sets,
                                       cox_preprocess_finegray)
    event, cens, comp = (x.copy() for x in EARLY.T)
    at = np.arange(7)
    for fn in (cox_preprocess_finegray, cox_finegray_risk_sets):
        with pytest.raises(ValueError, match='same length'):
            fn(event[:-1], cens, comp)
        with pytest.raises(ValueError, match='same length'):
            fn(event[:6].reshape(3, 2), cens[:6].reshape(3, 2),
               comp[:6].reshape(3, 2))
        # two finite times, none, a NaN, minus infinity
        with pytest.raises(ValueError, match='Exactly one'):
            fn(event, cens, np.where(at == 2, 1.5, comp))
        with pytest.raises(ValueError, match='Exactly one'):
            fn(event, cens, np.where(at == 0, INF, comp))
        with pytest.raises(ValueError, match='NaN'):
            fn(event, cens, np.where(at == 0, np.nan, comp))
        with pytest.raises(ValueError, match='Exactly one'):
            fn(event, cens, np.where(at == 2, -INF, comp))
    # unsorted rows, and a row censored before the first event
    with pytest.raises(ValueError, match='need to be sorted'):
        cox_finegray_risk_sets(event[::-1], cens[::-1], comp[::-1])
    with pytest.raises(ValueError, match='never appear in the risk set'):
        cox_finegray_risk_sets(event, cens, comp)
    # a competing row ahead of an event at the same time
    with pytest.raises(ValueError, match='need to be sorted'):
        cox_finegray_risk_sets(np.array([INF, 1.]), np.full(2, INF),
                               np.array([1., INF]))
    # the combinations that are not built, before the design is looked at
    X = np.zeros((7, 2))
    others = [(dict(strata=np.zeros(7)), 'competing_time together with strata '
               'is not supported: .* not built'),
              (dict(entry_time=np.full(7, -INF)), 'competing_time together '
               'with entry_time is not supported: .* not built'),
              (dict(ties='efron'), "competing_time together with "
               "ties='efron' is not supported: .* not built"),
              (dict(weights=np.ones(7)), 'competing_time together with '
               'weights is not supported: .* not built')]
    for kw, text in others:
        with pytest.raises(ValueError, match=text):
            CoxModel(event, cens, None, competing_time=comp, **kw)
        outcome = (event, cens)
        if 'strata' in kw:
            outcome += (kw.pop('strata'),)
        with pytest.raises(ValueError, match=text):
            RegressionModel(outcome, X, 'cox', competing_time=comp, **kw)
    for family in ('linear', 'logit', 'poisson'):
        with pytest.raises(ValueError, match="family='cox' only"):
            RegressionModel(np.ones(7), X, family, competing_time=comp)
    # the keyword is the last one of both signatures
    import inspect
    for fn in (CoxModel.__init__, RegressionModel):
        assert list(inspect.signature(fn).parameters)[-1] == 'competing_time'


def test_entry_points_are_declared_and_versions_agree():
    from bayesbridge_amd import _lib
    from ham_cabi import SHARED
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_coxfg_[a-z_]+)\s*\(', header))
    assert declared == {'bbx_coxfg_%s' % e
                        for e in SHARED + ('create', 'destroy')}
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 113
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'bbx_coxfg_create' in doc


def test_null_handles_and_designs_are_refused_on_the_host():
    from bayesbridge_amd import _lib
    lib = _lib.load()
    vec, ll, h = np.zeros(3), c_double(), c_void_p()
    ptr = vec.ctypes.data_as(c_void_p)
    assert lib.bbx_coxfg_loglik_grad(None, ptr, byref(ll), None) == -1
    assert 'NULL coxfg handle' in _lib.last_error()
    assert lib.bbx_coxfg_set_location(None, ptr) == -1
    assert lib.bbx_coxfg_nuts_sample(None, None, byref(ll), None) == -1
    assert lib.bbx_coxfg_destroy(None) == 0
    i32 = np.zeros(4, dtype=np.int32).ctypes.data_as(c_void_p)
    f64 = np.ones(4).ctypes.data_as(c_void_p)
    assert lib.bbx_coxfg_create(None, 1, i32, i32, i32, i32, 1, i32, f64, f64,
                                byref(h)) == -1
    assert 'invalid design' in _lib.last_error() and not h.value
    assert lib.bbx_coxfg_create(None, 1, i32, i32, i32, i32, 1, i32, f64, f64,
                                None) == -1
    assert 'NULL output pointer' in _lib.last_error()
