"""CPU: the host side of the Cox family's prediction -- the
brute-force oracle (tests/cox_predict_oracle.py) against the closed forms it
must reduce to (Nelson-Aalen at coef = 0, replicated rows for integer weights,
one plain model per stratum, the plain model for Fine-Gray without competing
rows, residuals that sum to 0), the grid helper cox_hazard_grid, every
ValueError / TypeError of the prediction methods without a device, the
refusals of the C entry points that need none, and (hipcc cross-compile) the
resources of the new kernels."""
import os
import types
from ctypes import c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_predict_oracle as cpo
from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table

INF = np.inf
EPS = np.finfo(np.float64).eps


def _data(n=60, n_times=7, frac_event=.6, seed=0):
    """Tied times on a small grid: (event_time, censoring_time, eta)."""
    rs = np.random.RandomState(seed)
    T = rs.randint(1, n_times + 1, n).astype(np.float64)
    is_event = rs.rand(n) < frac_event
    is_event[np.argmin(T)] = True
    event = np.where(is_event, T, INF)
    cens = np.where(is_event, INF, T)
    return event, cens, rs.randn(n)


def _close(a, b, tol=1e-15):
    a, b = np.asarray(a, dtype=cpo.LD), np.asarray(b, dtype=cpo.LD)
    return np.all(np.abs(a - b) <= tol * np.abs(b))


def test_oracle_at_zero_is_nelson_aalen():
    event, cens, _ = _data()
    grid = np.arange(0., 9., .5)
    for ties in ('breslow', 'efron'):
        r = cpo.rows(event, cens, ties=ties)
        lam = np.exp(cpo.log_baseline_hazard(grid, np.zeros(len(event)), r))
        # the closed form, written out once more: sum d / Y, or sum 1 / (Y - l)
        want = np.zeros(len(grid), dtype=cpo.LD)
        T = np.minimum(event, cens)
        for t in np.unique(event[np.isfinite(event)]):
            Y, d = int(np.sum(T >= t)), int(np.sum(event == t))
            jump = cpo.LD(d) / Y if ties == 'breslow' else \
                sum(cpo.LD(1) / (Y - l) for l in range(d))
            want[grid >= t] += jump
        assert lam[0] == 0 and _close(lam, want)
        assert _close(cpo.nelson_aalen(grid, r), want)


def test_oracle_integer_weights_are_replicated_rows():
    event, cens, eta = _data(seed=1)
    w = np.random.RandomState(2).randint(1, 4, len(event))
    rep = np.repeat(np.arange(len(event)), w)
    grid = np.arange(0., 9., .5)
    a = cpo.log_baseline_hazard(
        grid, eta, cpo.rows(event, cens, weights=w.astype(np.float64)))
    b = cpo.log_baseline_hazard(grid, eta[rep],
                                cpo.rows(event[rep], cens[rep]))
    assert _close(np.exp(a), np.exp(b))
    assert _close(cpo.nelson_aalen(grid, cpo.rows(event, cens, weights=w)),
                  cpo.nelson_aalen(grid, cpo.rows(event[rep], cens[rep])))


def test_oracle_strata_are_plain_models():
    event, cens, eta = _data(n=90, seed=3)
    strata = np.random.RandomState(4).randint(0, 3, len(event))
    for s in range(3):                     # every stratum has an event
        event[np.flatnonzero(strata == s)[0]] = 2.
        cens[np.flatnonzero(strata == s)[0]] = INF
    grid = np.arange(0., 9., .5)
    r = cpo.rows(event, cens, strata=strata)
    both = cpo.log_baseline_hazard(grid, eta, r)
    res = cpo.residuals(eta, r)
    assert both.shape == (3, len(grid))
    for s in range(3):
        m = strata == s
        one = cpo.rows(event[m], cens[m])
        assert _close(np.exp(both[s]),
                      np.exp(cpo.log_baseline_hazard(grid, eta[m], one)))
        assert _close(res[m], cpo.residuals(eta[m], one), 1e-14)


def test_oracle_finegray_without_competing_rows_is_plain():
    event, cens, eta = _data(seed=5)
    grid = np.arange(0., 9., .5)
    fg = cpo.rows(event, cens, competing_time=np.full(len(event), INF))
    plain = cpo.rows(event, cens)
    assert np.array_equal(cpo.log_baseline_hazard(grid, eta, fg),
                          cpo.log_baseline_hazard(grid, eta, plain))
    assert np.array_equal(cpo.residuals(eta, fg), cpo.residuals(eta, plain))


def test_oracle_finegray_keeps_competing_rows_with_the_censoring_weight():
    """Three rows, by hand: a competing row at 1, a censored row at 2, an
    event at 3.  G(3-) = 1 - 1/2, G(1-) = 1: H = e3 + (1/2) e1."""
    event = np.array([INF, INF, 3.])
    cens = np.array([INF, 2., INF])
    comp = np.array([1., INF, INF])
    eta = np.array([.3, -.2, .1])
    r = cpo.rows(event, cens, competing_time=comp)
    lam = np.exp(cpo.log_baseline_hazard([3.], eta, r))[0]
    e = np.exp(eta.astype(cpo.LD))
    assert _close(lam, 1 / (e[2] + e[0] / 2))


def test_oracle_residuals_sum_to_zero():
    event, cens, eta = _data(n=120, seed=6)
    rs = np.random.RandomState(7)
    strata = rs.randint(0, 3, len(event))
    T = np.minimum(event, cens)
    cases = [cpo.rows(event, cens), cpo.rows(event, cens, ties='efron'),
             cpo.rows(event, cens, weights=rs.rand(len(event)) + .5),
             cpo.rows(event, cens, entry=T - rs.randint(1, 4, len(T)))]
    for r in cases:
        n_event = int(np.sum(r.status == 1))
        assert abs(np.sum(cpo.residuals(eta, r))) <= 1e-12 * n_event
    r = cpo.rows(event, cens, strata=strata)
    res = cpo.residuals(eta, r)
    for s in range(3):
        n_event = int(np.sum((r.status == 1) & (strata == s)))
        assert abs(np.sum(res[strata == s])) <= 1e-12 * max(n_event, 1)
    # Fine-Gray: the competing rows' weights G(t-) / G(T-) are part of the sum
    comp = np.where(~np.isfinite(event) & (rs.rand(len(T)) < .5), T, INF)
    fg = cpo.rows(event, np.where(np.isfinite(comp), INF, cens),
                  competing_time=comp)
    n_event = int(np.sum(fg.status == 1))
    assert abs(np.sum(cpo.residuals(eta, fg))) <= 1e-12 * n_event


# ----------------------------------------------------------- cox_hazard_grid
def _plain_stub(event_time):
    event_time = np.asarray(event_time, dtype=np.float64)
    return types.SimpleNamespace(
        event_time=event_time, strata=None,
        n_event=int(np.sum(np.isfinite(event_time))))


def test_hazard_grid_indexes_the_last_event_at_or_before():
    from bayesbridge_amd.model import cox_hazard_grid
    m = _plain_stub([1., 2., 2., 2., 5., INF, INF])
    times, grid = cox_hazard_grid(m, [.5, 1., 1.5, 2., 4.9, 5., 9.])
    assert grid.dtype == np.int32 and grid.shape == (7,)
    # before the first event; on a tied time: the LAST event tied there; past
    # the last event: n_event - 1
    assert grid.tolist() == [-1, 0, 0, 3, 3, 4, 4]
    times, grid = cox_hazard_grid(m)
    assert times.tolist() == [1., 2., 5.] and grid.tolist() == [0, 3, 4]
    # a model whose events are rows event_row of rows sorted by exit time
    cp = types.SimpleNamespace(
        event_time=np.array([1., INF, 2., 2., INF, 3.]), strata=None,
        n_event=4, event_row=np.array([0, 2, 3, 5]))
    assert cox_hazard_grid(cp, [0., 1., 2., 2.5, 3.])[1].tolist() == \
        [-1, 0, 2, 2, 3]


def test_hazard_grid_indexes_strata_independently():
    from bayesbridge_amd.model import cox_hazard_grid
    # stratum 0: rows 0-3 (events at 1, 4, 4), stratum 1: rows 4-6 (2, 3)
    m = types.SimpleNamespace(
        event_time=np.array([1., 4., 4., INF, 2., 3., INF]),
        strata=np.array([0, 0, 0, 0, 1, 1, 1]),
        stratum_ptr=np.array([0, 4, 7]), stratum_n_event=np.array([3, 2]),
        n_event=5)
    times, grid = cox_hazard_grid(m, [0., 1., 2., 3., 4.])
    assert grid.shape == (2, 5) and grid.dtype == np.int32
    assert grid.tolist() == [[-1, 0, 0, 0, 2], [-1, -1, 3, 4, 4]]
    with pytest.raises(ValueError, match='grid of times is required'):
        cox_hazard_grid(m)


def test_hazard_grid_refuses_bad_grids():
    from bayesbridge_amd.model import cox_hazard_grid
    m = _plain_stub([1., 2., INF])
    for bad, text in (([1., INF], 'finite'), ([np.nan], 'finite'),
                      ([2., 1.], 'ascending'), ([], 'non-empty'),
                      ([[1., 2.]], '1-d')):
        with pytest.raises(ValueError, match=text):
            cox_hazard_grid(m, bad)


def _stub_model(strata=None, centered=True, column_offset=None, p=3):
    """A CoxModel that was never given a device: every check of the
    prediction methods comes before the first device call."""
    from bayesbridge_amd import CoxModel
    model = CoxModel.__new__(CoxModel)
    model.design = types.SimpleNamespace(
        shape=(4, p), centered=centered, column_offset=column_offset,
        device=0)
    model.event_time = np.array([1., 2., INF, INF])
    model.n_event = 2
    model.strata = strata
    if strata is not None:
        model.stratum_ptr = np.array([0, 2, 4])
        model.stratum_n_event = np.array([1, 1])
        model.event_time = np.array([1., INF, 2., INF])
    model._cox = c_void_p()
    return model


def test_prediction_arguments_are_checked_before_the_device():
    m = _stub_model(column_offset=np.zeros(3))
    coef, X = np.zeros(3), np.zeros((2, 3))
    with pytest.raises(ValueError, match='Exactly one of X_new and'):
        m.predict_survival(coef)
    with pytest.raises(ValueError, match='Exactly one of X_new and'):
        m.predict_survival(coef, X_new=X, linear_predictor=np.zeros(2))
    with pytest.raises(ValueError, match="model's 3 columns"):
        m.predict_survival(coef, X_new=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="model's 3 columns"):
        m.predict_survival(coef, X_new=sparse.csr_matrix((2, 2)))
    with pytest.raises(ValueError, match='coef must have shape'):
        m.predict_survival(np.zeros(4), X_new=X)
    with pytest.raises(ValueError, match='coef must have shape'):
        m.cumulative_baseline_hazard(np.zeros((2, 3)))
    with pytest.raises(ValueError, match='coef must have length 3'):
        m.martingale_residuals(np.zeros((3, 2)))
    with pytest.raises(ValueError, match='linear_predictor must have shape'):
        m.predict_survival(np.zeros((3, 2)), linear_predictor=np.zeros(5))
    with pytest.raises(ValueError, match='linear_predictor must have shape'):
        m.predict_survival(coef, linear_predictor=np.zeros((5, 2)))
    with pytest.raises(ValueError, match='stratified model only'):
        m.predict_survival(coef, X_new=X, strata_new=np.zeros(2))
    with pytest.raises(ValueError, match='ascending'):
        m.predict_survival(coef, X_new=X, times=[2., 1.])
    with pytest.raises(ValueError, match='finite'):
        m.cumulative_baseline_hazard(coef, times=[1., INF])
    # a training design adopted from device pointers has no host offsets
    adopted = _stub_model(column_offset=None)
    with pytest.raises(TypeError, match='linear_predictor'):
        adopted.predict_survival(coef, X_new=X)
    # with strata: a grid and the stratum of every new row
    s = _stub_model(strata=np.array(['a', 'a', 'b', 'b']),
                    column_offset=np.zeros(3))
    with pytest.raises(ValueError, match='strata_new .* is required'):
        s.predict_survival(coef, X_new=X, times=[1.])
    with pytest.raises(ValueError, match='one label for each new row'):
        s.predict_survival(coef, X_new=X, times=[1.], strata_new=['a'])
    with pytest.raises(ValueError, match='must be a stratum of the training'):
        s.predict_survival(coef, X_new=X, times=[1.], strata_new=['a', 'c'])
    with pytest.raises(ValueError, match='grid of times is required'):
        s.predict_survival(coef, X_new=X, strata_new=['a', 'b'])
    with pytest.raises(ValueError, match='grid of times is required'):
        s.cumulative_baseline_hazard(coef)


# ------------------------------------------------------------------ the C ABI
FAMILIES = ('cox', 'coxcp', 'coxef', 'coxw', 'coxfg')


def test_entry_points_are_exported_and_documented():
    from bayesbridge_amd import _lib
    lib = _lib.load()
    assert _lib.COX_FAMILIES == FAMILIES
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for fam in FAMILIES:
        for entry in ('baseline_hazard', 'residuals'):
            assert getattr(lib, 'bbx_%s_%s' % (fam, entry)).restype is not None
        assert 'BBX_COX_PREDICT_DECL(%s)' % fam in header
    assert 'bbx_cox_survival_summary' in _lib.EXPORTED_SYMBOLS
    for text in (header, doc):
        assert 'bbx_<fam>_baseline_hazard' in text
        assert 'bbx_<fam>_residuals' in text
        assert 'bbx_cox_survival_summary' in text
    makefile = open(os.path.join(ROOT, 'bayes-bridge_amd', 'csrc',
                                 'Makefile')).read()
    assert 'cox_predict.hip' in makefile


def test_null_arguments_are_refused_on_the_host():
    from bayesbridge_amd import _lib
    lib = _lib.load()
    vec = np.zeros(4)
    ptr = vec.ctypes.data_as(c_void_p)
    i32 = np.zeros(4, dtype=np.int32).ctypes.data_as(c_void_p)
    for fam in FAMILIES:
        assert getattr(lib, 'bbx_%s_baseline_hazard' % fam)(
            None, ptr, 1, 1, i32, ptr) == -1
        assert 'NULL %s handle' % fam in _lib.last_error()
        assert getattr(lib, 'bbx_%s_residuals' % fam)(None, ptr, ptr) == -1
        assert 'NULL %s handle' % fam in _lib.last_error()
    call = lib.bbx_cox_survival_summary
    assert call(0, 1, 1, 1, 1, None, ptr, None, ptr, ptr, None) == -1
    assert 'NULL argument' in _lib.last_error()
    assert call(0, 1, 1, 1, 1, ptr, ptr, None, None, ptr, None) == -1
    assert call(0, 0, 1, 1, 1, ptr, ptr, None, ptr, ptr, None) == -1
    assert 'n_row' in _lib.last_error()
    assert call(0, 1, 0, 1, 1, ptr, ptr, None, ptr, ptr, None) == -1
    assert 'n_time' in _lib.last_error()
    assert call(0, 1, 1, 0, 1, ptr, ptr, None, ptr, ptr, None) == -1
    assert 'n_draw' in _lib.last_error()
    assert call(0, 1, 1, 1, 0, ptr, ptr, None, ptr, ptr, None) == -1
    assert 'n_group' in _lib.last_error()
    assert call(0, 1, 1, 1, 2, ptr, ptr, None, ptr, ptr, None) == -1
    assert 'NULL group' in _lib.last_error()
    bad = np.array([2], dtype=np.int32).ctypes.data_as(c_void_p)
    assert call(0, 1, 1, 1, 2, ptr, ptr, bad, ptr, ptr, None) == -1
    assert 'group[0] outside [0, n_group)' in _lib.last_error()


# ------------------------------------------------------------------ resources
def _no_spill(table, names):
    for k in names:
        assert sum(k in name for name in table) >= 1, (k, sorted(table))
    for name, res in table.items():
        if any(k in name for k in names):
            assert res["VGPRs Spill"] == 0, (name, res)
            assert res["SGPRs Spill"] == 0, (name, res)
            assert res["ScratchSize [bytes/lane]"] == 0, (name, res)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_survival_kernels_do_not_spill(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "cox_predict.hip"),
        tmp_path)
    # with and without groups
    assert sum("cox_survival_kernel" in name for name in table) == 2
    _no_spill(table, ("cox_survival_kernel",))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", ["cox.hip", "cox_interval.hip",
                                 "cox_efron.hip", "cox_weighted.hip",
                                 "cox_finegray.hip"])
def test_hazard_grid_kernel_does_not_spill(src, tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", src), tmp_path)
    assert sum("cox_hazard_grid_kernel" in name for name in table) == 1
    _no_spill(table, ("cox_hazard_grid_kernel",))
