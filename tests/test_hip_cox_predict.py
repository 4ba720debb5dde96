"""GPU: baseline hazard, martingale residuals and posterior survival of the
Cox family (csrc/cox_family.hpp's cox_hazard_grid_kernel and the
two entry points of every handle type, csrc/cox_predict.hip) against the
brute-force long-double oracle of tests/cox_predict_oracle.py, which states
the definitions from the observed times alone.  There is no reference
implementation of these quantities: the oracle, the Nelson-Aalen closed form
at coef = 0 and the identities between the calls are the yardsticks."""
import warnings
from ctypes import c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_cases as cc
import cox_predict_oracle as cpo
from test_hip_cox_efron import _within

pytestmark = pytest.mark.gpu

INF = np.inf
EPS = np.finfo(np.float64).eps
KINDS = ('plain', 'strata', 'entry', 'efron', 'weights', 'finegray')
PREFIX = {'plain': 'bbx_cox_', 'strata': 'bbx_cox_', 'entry': 'bbx_coxcp_',
          'efron': 'bbx_coxef_', 'weights': 'bbx_coxw_',
          'finegray': 'bbx_coxfg_'}
HAZ_TOL = 1e-11      # on log Lambda0: the gradient tests' GRAD_TOL holds c
SURV_TOL = .37 * 1e-11 + 4 * EPS    # x exp(-x) <= 1/e times the hazard's
STRATA_SIZES = (1, 2, 46, 300, 400, 600, 700)          # 2049 rows


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _haz_ok(got, want):
    """|got - want| <= 1e-11 + 4 eps |want|, -inf where the oracle has it;
    returns the largest error in units of the tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    none = np.isneginf(want.astype(np.float64))
    assert np.array_equal(np.isneginf(got), none)
    err = np.abs(got[~none] - want[~none]).astype(np.float64)
    tol = HAZ_TOL + 4 * EPS * np.abs(want[~none]).astype(np.float64)
    worst = float(np.max(err / tol)) if err.size else 0.
    assert worst <= 1., worst
    return worst


class Problem():
    """Rows in the model's order, the device model on a centred design, the
    oracle's rows and the centred matrix in long double."""

    def __init__(self, kind, design='dense64', n=2049, p=40, seed=0,
                 n_times=12, event_frac=.5):
        from bayesbridge_amd import CoxModel, HipDenseDesignMatrix, \
            HipSparseDesignMatrix
        from bayesbridge_amd import model as bm
        rs = np.random.RandomState(seed)
        X = cc._design(n, p, 'binary' if design == 'tiled_binary'
                       else 'normal', rs, .1)
        T = rs.randint(1, n_times + 1, n).astype(np.float64)
        u = rs.rand(n)
        is_event = u < event_fraction(kind, event_frac)
        is_comp = (u > 2 / 3) if kind == 'finegray' else np.zeros(n, bool)
        strata = None
        if kind == 'strata':
            sizes = STRATA_SIZES if n == 2049 else (1, n - 1)
            strata = np.repeat(np.arange(len(sizes)), sizes)
            first = np.concatenate(([0], np.cumsum(sizes)[:-1]))
            T[first], is_event[first] = .5, True     # no stratum is dropped
        else:
            T[0], is_event[0], is_comp[0] = .5, True, False
        event = np.where(is_event, T, INF)
        comp = np.where(is_comp & ~is_event, T, INF)
        cens = np.where(np.isfinite(event) | np.isfinite(comp), INF, T)
        kw = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if kind == 'strata':
                event, cens, strata, X, _ = bm.cox_preprocess_stratified(
                    event, cens, strata, X)
                kw['strata'] = strata
            elif kind == 'entry':
                entry = np.where(rs.rand(n) < .5, T - rs.randint(1, 4, n),
                                 -INF)
                entry, event, cens, X, _ = bm.cox_preprocess_interval(
                    entry, event, cens, X)
                kw['entry'] = entry
            elif kind == 'finegray':
                event, cens, comp, X, keep, _, _ = bm.cox_preprocess_finegray(
                    event, cens, comp, X)
                assert len(keep) == n      # G is the model's: the same rows
                kw['competing_time'] = comp
            else:
                event, cens, X, keep = bm.cox_preprocess(event, cens, X)
                if kind == 'weights':
                    kw['weights'] = (rs.rand(n) + .5)[keep]
                if kind == 'efron':
                    kw['ties'] = 'efron'
        if design == 'tiled_binary':
            self.design = HipSparseDesignMatrix(
                sparse.csr_matrix(X), center_predictor=True,
                add_intercept=False, storage='tiled')
        else:
            self.design = HipDenseDesignMatrix(X, center_predictor=True,
                                               add_intercept=False)
        assert self.design.shape == X.shape        # no column was dropped
        mkw = dict(kw)
        if 'entry' in mkw:
            mkw['entry_time'] = mkw.pop('entry')
        self.model = CoxModel(event, cens, self.design, **mkw)
        assert self.model._ham_prefix == PREFIX[kind]
        self.kind, self.X = kind, X
        self.event, self.cens = event, cens
        self.rows = cpo.rows(event, cens, **kw)
        Xd = np.asarray(X.todense()) if sparse.issparse(X) else X
        self.Xc = Xd.astype(cpo.LD) - np.mean(Xd.astype(cpo.LD), axis=0)
        self.beta = rs.randn(p) * .5
        ev = np.unique(event[np.isfinite(event)])
        self.event_times = ev
        self.grid = np.sort(np.concatenate(
            (ev, rs.uniform(0., ev[-1] + 1., 257))))

    def eta(self, beta):
        return self.Xc @ np.asarray(beta, dtype=cpo.LD)


def event_fraction(kind, event_frac):
    return 1 / 3 if kind == 'finegray' else event_frac


_CACHE = {}


def _problem(kind, design='dense64', **kw):
    """One problem per (kind, design, shape) for the whole module: the
    tests read it and leave it unchanged."""
    key = (kind, design) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        _CACHE[key] = Problem(kind, design, **kw)
    return _CACHE[key]


# 1 ------------------------------------------------------------------------
@pytest.mark.parametrize('design', ['tiled_binary', 'dense64'])
@pytest.mark.parametrize('kind', KINDS)
def test_hazard_matches_the_oracle(kind, design):
    """2049 x 40, times on a 12-point grid (tie groups a hundred deep), three
    draws in one call (coefficient scales 0, 0.1, 1), at every distinct event
    time and at 257 arbitrary points.  Largest error seen on the device, in
    units of the tolerance: see DESIGN 10i."""
    pr = _problem(kind, design)
    assert pr.model.n_obs > 1900
    coef = pr.beta[:, None] * np.array([0., .1, 1.])
    times, got = pr.model.cumulative_baseline_hazard(coef, pr.grid, log=True)
    assert np.array_equal(times, pr.grid)
    if kind == 'strata':
        assert got.shape == (len(STRATA_SIZES), len(pr.grid), 3)
    else:
        assert got.shape == (len(pr.grid), 3)
        # times=None is the distinct event times
        t0, own = pr.model.cumulative_baseline_hazard(coef[:, 2], log=True)
        assert np.array_equal(t0, pr.event_times)
        _haz_ok(own, cpo.log_baseline_hazard(t0, pr.eta(coef[:, 2]), pr.rows))
    worst = 0.
    for d in range(3):
        want = cpo.log_baseline_hazard(pr.grid, pr.eta(coef[:, d]), pr.rows)
        worst = max(worst, _haz_ok(got[..., d], want))
    print('%s %s: largest error %.3g of the tolerance' % (kind, design, worst))
    # log=False is its exponential
    assert np.array_equal(
        pr.model.cumulative_baseline_hazard(coef, pr.grid)[1], np.exp(got))


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize('n_event', [1, 255, 256, 257, 513])
def test_event_scan_edges(n_event):
    """SCAN_G = 256 chunks over the events: from one event per chunk to two.
    Distinct event times; one grid point before the first event, every event
    time, one past the last; and n_grid = 1, n_draw = 1."""
    from bayesbridge_amd import CoxModel, HipDenseDesignMatrix
    rs = np.random.RandomState(n_event)
    n, p = n_event + 300, 5
    X = rs.randn(n, p)
    event = np.concatenate((np.arange(1., n_event + 1.), np.full(300, INF)))
    cens = np.concatenate((np.full(n_event, INF),
                           np.sort(rs.uniform(1., n_event + 1., 300))[::-1]))
    model = CoxModel(event, cens, HipDenseDesignMatrix(
        X, center_predictor=True, add_intercept=False))
    assert model.n_event == n_event
    rows = cpo.rows(event, cens)
    Xc = X.astype(cpo.LD) - np.mean(X.astype(cpo.LD), axis=0)
    coef = rs.randn(p, 2) * .5
    grid = np.concatenate(([.5], np.arange(1., n_event + 1.),
                           [n_event + 7.]))
    _, got = model.cumulative_baseline_hazard(coef, grid, log=True)
    assert np.all(np.isneginf(got[0]))
    for d in range(2):
        _haz_ok(got[:, d], cpo.log_baseline_hazard(
            grid, Xc @ coef[:, d].astype(cpo.LD), rows))
    assert np.array_equal(got[-1], got[-2])        # past the last event
    one = model.cumulative_baseline_hazard(coef[:, 1], [float(n_event)],
                                           log=True)[1]
    assert one.shape == (1,) and one[0] == got[-2, 1]


# 3 ------------------------------------------------------------------------
def test_the_shift_is_per_stratum():
    """Two strata whose eta lie 800 apart: both rows of log Lambda0 are finite
    and the oracle's; with ONE max over all rows the lower stratum's hazards
    underflow (the oracle's global-shift mutant is not finite there)."""
    from bayesbridge_amd import CoxModel, HipDenseDesignMatrix
    import torch
    rs = np.random.RandomState(5)
    n = 60
    strata = np.repeat([0, 1], n // 2)
    X = np.column_stack((800. * strata, rs.randn(n)))
    event = np.tile(np.concatenate((np.arange(1., 21.), np.full(10, INF))), 2)
    cens = np.tile(np.concatenate((np.full(20, INF),
                                   np.arange(15., 5., -1.))), 2)
    t = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    design = HipDenseDesignMatrix.from_device_array(
        n, 2, t.data_ptr(), add_intercept=False, in_dtype='float64',
        storage_dtype='float64')
    torch.cuda.synchronize()
    model = CoxModel(event, cens, design, strata=strata)
    beta = np.array([1., .3])
    grid = np.arange(.5, 22.)
    _, got = model.cumulative_baseline_hazard(beta, grid, log=True)
    rows = cpo.rows(event, cens, strata=strata)
    eta = X.astype(cpo.LD) @ beta.astype(cpo.LD)
    want = cpo.log_baseline_hazard(grid, eta, rows)
    assert got.shape == (2, len(grid)) and np.all(np.isfinite(got[:, 1:]))
    _haz_ok(got, want)
    assert abs((got[0, -1] - got[1, -1]) - 800.) < 5.
    with np.errstate(all='ignore'):
        mutant = cpo.log_baseline_hazard(grid, eta, rows, global_shift=True)
    assert not np.all(np.isfinite(mutant[0, 1:].astype(np.float64)))


# 4 ------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'efron', 'weights'])
def test_zero_coefficients_give_nelson_aalen(kind):
    pr = _problem(kind)
    times, lam = pr.model.cumulative_baseline_hazard(np.zeros(40))
    want = cpo.nelson_aalen(times, pr.rows)
    assert np.all(np.abs(lam - want) <= (HAZ_TOL + 4 * EPS) * np.abs(want))


# 5 ------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'strata', 'finegray'])
def test_batch_and_repeat_give_the_same_bits(kind):
    pr = _problem(kind)
    coef = pr.beta[:, None] * np.array([.3, 1., -.7])
    _, all3 = pr.model.cumulative_baseline_hazard(coef, pr.grid, log=True)
    _, again = pr.model.cumulative_baseline_hazard(coef, pr.grid, log=True)
    assert np.array_equal(all3, again)
    for d in range(3):
        _, one = pr.model.cumulative_baseline_hazard(coef[:, d], pr.grid,
                                                     log=True)
        assert np.array_equal(one, all3[..., d])
    res = pr.model.martingale_residuals(pr.beta)
    assert np.array_equal(res, pr.model.martingale_residuals(pr.beta))


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'efron', 'weights'])
def test_an_empty_risk_set_sum_names_its_draw(kind):
    """test_underflowing_risk_set_gives_minus_infinity's case (dense 2000 x
    20, times on a 50-point grid, beta[0] = 2000) as draw 1 of 3."""
    pr = _problem(kind, n=2000, p=20, seed=9, n_times=50)
    bad = np.zeros(20)
    bad[0] = 2000.
    assert pr.model.compute_loglik_and_gradient(bad, loglik_only=True) \
        == (-INF, None)
    coef = np.column_stack((np.zeros(20), bad, pr.beta))
    with pytest.raises(ValueError, match='draw 1: a risk-set sum'):
        pr.model.cumulative_baseline_hazard(coef, pr.grid)
    with pytest.raises(ValueError, match='residuals: a risk-set sum'):
        pr.model.martingale_residuals(bad)
    # the flags were that call's only
    good = coef[:, [0, 2]]
    _, got = pr.model.cumulative_baseline_hazard(good, pr.grid, log=True)
    for d in range(2):
        _haz_ok(got[:, d], cpo.log_baseline_hazard(
            pr.grid, pr.eta(good[:, d]), pr.rows))
    ll = pr.model.compute_loglik_and_gradient(pr.beta)[0]
    assert np.isfinite(ll)


# 7 ------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'strata', 'efron'])
def test_launches_per_draw(kind):
    from bayesbridge_amd import _lib
    lib = _lib.load()
    pr = _problem(kind)

    def launches(f):
        before = lib.bbx_launch_count()
        f()
        return lib.bbx_launch_count() - before

    yard = launches(lambda: pr.model.compute_loglik_and_gradient(
        pr.beta, loglik_only=True))
    counts = {}
    for S in (1, 4):
        coef = np.ascontiguousarray(pr.beta[:, None] * np.linspace(.1, 1., S))
        for n_grid in (1, 257):
            grid = np.sort(np.random.RandomState(n_grid).uniform(0., 13.,
                                                                 n_grid))
            counts[S, n_grid] = launches(
                lambda: pr.model.cumulative_baseline_hazard(coef, grid))
    per_draw = counts[1, 1]
    print(kind, 'launches per draw', per_draw, 'loglik_only', yard)
    assert per_draw <= yard + 1
    for (S, n_grid), c in counts.items():
        assert c == S * per_draw, (S, n_grid, c)


# 8 ------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_the_hessian_location_survives(kind):
    pr = _problem(kind)
    v = np.random.RandomState(1).randn(40)
    op = pr.model.get_hessian_matvec_operator(pr.beta)
    before = op(v)
    pr.model.cumulative_baseline_hazard(pr.beta[:, None] * np.array([0., 2.]),
                                        pr.grid)
    pr.model.martingale_residuals(.5 * pr.beta)
    assert np.array_equal(op(v), before)


# 9 ------------------------------------------------------------------------
@pytest.mark.parametrize('design', ['tiled_binary', 'dense64'])
@pytest.mark.parametrize('kind', KINDS)
def test_residuals_match_the_oracle(kind, design):
    pr = _problem(kind, design)
    got = pr.model.martingale_residuals(pr.beta)
    assert got.shape == (pr.model.n_obs,)
    want = cpo.residuals(pr.eta(pr.beta), pr.rows)
    print(kind, design, 'residuals: %.3g relative'
          % (np.abs(got - want).max() / np.abs(want).max()))
    assert _within(got, want, 1e-11)
    assert abs(np.sum(got)) <= 1e-11 * pr.model.n_event
    if kind == 'plain':
        # delta_i - exp(eta_i + log Lambda0(T_i)), Lambda0 from the hazard call
        T = np.minimum(pr.event, pr.cens)
        order = np.argsort(T, kind='stable')
        _, lh = pr.model.cumulative_baseline_hazard(pr.beta, T[order],
                                                    log=True)
        lam = np.empty(len(T))
        lam[order] = lh
        eta = pr.eta(pr.beta).astype(np.float64)
        ident = np.isfinite(pr.event) - np.exp(eta + lam)
        assert _within(got, ident, 1e-11)


# 10 -----------------------------------------------------------------------
def _summary(eta, lh, group, draws=True, n_group=None):
    from bayesbridge_amd import _lib
    n_draw, n_row = eta.shape
    n_group = lh.shape[1] if n_group is None else n_group
    n_time = lh.shape[2]
    mean, sd = np.full((n_row, n_time), 7.), np.full((n_row, n_time), 7.)
    out = np.full((n_row, n_time, n_draw), 7.) if draws else None
    st = _lib.load().bbx_cox_survival_summary(
        0, n_row, n_time, n_draw, n_group, _ptr(eta), _ptr(lh), _ptr(group),
        _ptr(mean), _ptr(sd), _ptr(out))
    return st, mean, sd, out


@pytest.mark.parametrize('n_group', [1, 3])
@pytest.mark.parametrize('n_draw', [1, 5])
@pytest.mark.parametrize('n_time', [1, 3])
@pytest.mark.parametrize('n_row', [1, 255, 257])
def test_survival_summary_matches_the_oracle(n_row, n_time, n_draw, n_group):
    rs = np.random.RandomState(n_row + 10 * n_time + 100 * n_draw + n_group)
    eta = np.ascontiguousarray(rs.randn(n_draw, n_row) * 1.5)
    lh = np.ascontiguousarray(
        np.sort(rs.randn(n_draw, n_group, n_time), axis=2) - 1.)
    group = None
    if n_group > 1:
        group = rs.randint(0, n_group, n_row).astype(np.int32)
        group[0] = n_group - 1
    # the edges: no event yet, a certain event, a NaN draw
    last = 0 if group is None else int(group[n_row - 1])
    lh[0, 0, 0] = -INF
    eta[0, n_row - 1] = 800.
    lh[0, last, n_time - 1] = 0.
    if n_row > 1:
        eta[n_draw - 1, 1] = np.nan
    st, mean, sd, draws = _summary(eta, lh, group)
    assert st == 0
    S, omean, osd = cpo.survival(eta, lh, group)
    nan = np.isnan(S.astype(np.float64))
    assert np.array_equal(np.isnan(draws), nan)
    assert np.all(np.abs(draws[~nan] - S[~nan]) <= SURV_TOL)
    cell = np.any(nan, axis=-1)
    assert np.array_equal(np.isnan(mean), cell)
    assert np.array_equal(np.isnan(sd), cell)
    assert np.all(np.abs(mean[~cell] - omean[~cell]) <= SURV_TOL)
    assert np.all(np.abs(sd[~cell] - osd[~cell]) <= 2 * SURV_TOL)
    # exactly 1 before the first event, exactly 0 for a certain event: the
    # long-double oracle reaches either value later than float64 does
    S64 = S.astype(np.float64)
    assert np.all(draws[S64 == 1.] == 1.)
    assert np.all(draws[S64 == 0.] == 0.)
    assert S64[n_row - 1, n_time - 1, 0] == 0.
    if n_draw == 1:
        assert np.all(sd[~cell] == 0.)
    # without the draws the summaries have the same bits
    st, mean2, sd2, _ = _summary(eta, lh, group, draws=False)
    assert st == 0
    assert np.array_equal(mean2, mean, equal_nan=True)
    assert np.array_equal(sd2, sd, equal_nan=True)


def test_survival_edges_are_exact():
    """-inf gives exactly 1, eta = 800 at log_hazard = 0 exactly 0, a NaN
    draw is a NaN in its own cell of `draws` only, one draw has sd == 0."""
    eta = np.array([[0., 800., 1.], [0., 800., np.nan]])
    lh = np.array([[[-INF, 0.]], [[-INF, 0.]]])
    st, mean, sd, draws = _summary(eta, lh, None)
    assert st == 0
    assert np.all(draws[:2, 0, :] == 1.) and np.all(draws[1, 1, :] == 0.)
    assert np.all(mean[:2, 0] == 1.) and mean[1, 1] == 0.
    assert np.all(sd[:2] == 0.)
    assert np.isnan(draws[2, 1, 1]) and np.isfinite(draws[2, 1, 0])
    assert draws[2, 0, 0] == 1. and np.isnan(draws[2, 0, 1])
    assert np.all(np.isnan(mean[2])) and np.all(np.isnan(sd[2]))
    st, mean, sd, draws = _summary(eta[:1], lh[:1], None)
    assert st == 0 and np.all(sd == 0.)
    assert np.array_equal(draws[..., 0], mean)


def test_more_groups_than_the_staging_buffer():
    """Past 2048 groups the kernel reads log_hazard lane by lane."""
    rs = np.random.RandomState(3)
    n_group, n_row = 2100, 300
    eta = np.ascontiguousarray(rs.randn(2, n_row))
    lh = np.ascontiguousarray(rs.randn(2, n_group, 2) - 1.)
    group = rs.randint(0, n_group, n_row).astype(np.int32)
    group[:2] = 0, n_group - 1
    st, mean, sd, draws = _summary(eta, lh, group)
    assert st == 0
    S, omean, osd = cpo.survival(eta, lh, group)
    assert np.all(np.abs(draws - S) <= SURV_TOL)
    assert np.all(np.abs(mean - omean) <= SURV_TOL)
    assert np.all(np.abs(sd - osd) <= 2 * SURV_TOL)


# 11 -----------------------------------------------------------------------
def _oracle_survival(pr, coef, X_rows, times, group=None):
    """The oracle's (S, mean, sd) on rows of the centred training matrix."""
    lh = np.stack([np.atleast_2d(cpo.log_baseline_hazard(
        times, pr.eta(coef[:, d]), pr.rows)) for d in range(coef.shape[1])])
    eta = np.stack([X_rows @ coef[:, d].astype(cpo.LD)
                    for d in range(coef.shape[1])])
    return cpo.survival(eta, lh, group)


@pytest.mark.parametrize('design', ['tiled_binary', 'dense64'])
def test_predict_survival_end_to_end(design):
    pr = _problem('plain', design)
    rows = np.arange(0, 2000, 40)                  # 50 training rows
    X_new = pr.X[rows]
    coef = pr.beta[:, None] * np.array([.2, 1., .6])
    times = pr.grid[::16]
    got = pr.model.predict_survival(coef, X_new, times, return_draws=True)
    assert np.array_equal(got['time'], times)
    S, mean, sd = _oracle_survival(pr, coef, pr.Xc[rows], times)
    assert got['draws'].shape == (50, len(times), 3)
    assert np.all(np.abs(got['draws'] - S) <= SURV_TOL)
    assert np.all(np.abs(got['mean'] - mean) <= SURV_TOL)
    assert np.all(np.abs(got['sd'] - sd) <= 2 * SURV_TOL)
    assert 'draws' not in pr.model.predict_survival(coef, X_new, times)
    # a single new row: every column of it is constant
    one = pr.model.predict_survival(coef, X_new[:1], times)
    assert np.all(np.abs(one['mean'] - mean[:1]) <= SURV_TOL)
    assert np.all(np.abs(one['sd'] - sd[:1]) <= 2 * SURV_TOL)
    # linear_predictor = the new design's product: the same bits
    new_design = pr.model._new_design(X_new)
    lp = np.column_stack([new_design.dot(np.ascontiguousarray(coef[:, d]))
                          for d in range(3)])
    same = pr.model.predict_survival(coef, linear_predictor=lp, times=times,
                                     return_draws=True)
    for key in ('mean', 'sd', 'draws'):
        assert np.array_equal(same[key], got[key])
    # coef = 0: exp(-Nelson-Aalen) for every row, no spread
    zero = pr.model.predict_survival(np.zeros(40), X_new)
    na = np.exp(-cpo.nelson_aalen(zero['time'], pr.rows))
    assert np.array_equal(zero['time'], pr.event_times)
    assert np.all(np.abs(zero['mean'] - na) <= SURV_TOL)
    assert np.all(zero['sd'] == 0.)


def test_prediction_is_centred_with_the_training_offsets():
    """A constant added to one column of the training matrix and of X_new
    leaves the prediction alone: X_new is centred with the training means
    (centred with its own, 50 rows would give another eta)."""
    from bayesbridge_amd import CoxModel, HipDenseDesignMatrix
    pr = _problem('plain', 'dense64')
    shifted = pr.X.copy()
    shifted[:, 3] += 5.
    model = CoxModel(pr.event, pr.cens, HipDenseDesignMatrix(
        shifted, center_predictor=True, add_intercept=False))
    rows = np.arange(0, 2000, 40)
    coef = pr.beta[:, None] * np.array([.2, 1.])
    times = pr.grid[::16]
    a = pr.model.predict_survival(coef, pr.X[rows], times)
    b = model.predict_survival(coef, shifted[rows], times)
    assert np.all(np.abs(a['mean'] - b['mean']) <= 2 * SURV_TOL)
    assert np.all(np.abs(a['sd'] - b['sd']) <= 4 * SURV_TOL)
    own = pr.X[rows] - pr.X[rows].mean(axis=0) + pr.X.mean(axis=0)
    c = pr.model.predict_survival(coef, own, times)
    assert np.abs(a['mean'] - c['mean']).max() > 1e-3


def test_predict_survival_uses_the_row_stratum():
    pr = _problem('strata', 'dense64')
    rows = np.concatenate(([0, 1, 2], np.arange(3, 2049, 45)))
    strata_new = pr.rows.strata[rows]
    assert len(np.unique(strata_new)) == len(STRATA_SIZES)
    coef = pr.beta[:, None] * np.array([.2, 1.])
    times = pr.grid[::16]
    got = pr.model.predict_survival(coef, pr.X[rows], times,
                                    strata_new=strata_new, return_draws=True)
    S, mean, sd = _oracle_survival(pr, coef, pr.Xc[rows], times, strata_new)
    assert np.all(np.abs(got['draws'] - S) <= SURV_TOL)
    assert np.all(np.abs(got['mean'] - mean) <= SURV_TOL)
    assert np.all(np.abs(got['sd'] - sd) <= 2 * SURV_TOL)
    # the stratum matters
    other = pr.model.predict_survival(
        coef, pr.X[rows], times, strata_new=np.full(len(rows), 6))
    assert np.abs(other['mean'] - got['mean']).max() > 1e-3


# 12 -----------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_refusals_are_status_codes(kind):
    from bayesbridge_amd import _lib
    lib = _lib.load()
    pr = _problem(kind, n=300, p=6, seed=2)
    model, P = pr.model, 6
    fam = PREFIX[kind]
    hazard = getattr(lib, fam + 'baseline_hazard')
    resid = getattr(lib, fam + 'residuals')
    beta = np.ascontiguousarray(pr.beta)
    grid = np.array([-1, 0, model.n_event - 1], dtype=np.int32)
    out, res = np.empty(3), np.empty(model.n_obs)
    h = model.handle
    INVALID, STATE = -1, -5

    def refused(st, text, code=INVALID):
        assert st == code, st
        assert text in _lib.last_error(), _lib.last_error()

    refused(hazard(None, _ptr(beta), 1, 3, _ptr(grid), _ptr(out)), 'NULL')
    refused(hazard(h, None, 1, 3, _ptr(grid), _ptr(out)), 'NULL argument')
    refused(hazard(h, _ptr(beta), 1, 3, None, _ptr(out)), 'NULL argument')
    refused(hazard(h, _ptr(beta), 1, 3, _ptr(grid), None), 'NULL argument')
    refused(hazard(h, _ptr(beta), 0, 3, _ptr(grid), _ptr(out)), 'n_draw')
    refused(hazard(h, _ptr(beta), 1, 0, _ptr(grid), _ptr(out)), 'n_grid')
    for bad in (-2, model.n_event):
        g = np.array([0, bad, 0], dtype=np.int32)
        refused(hazard(h, _ptr(beta), 1, 3, _ptr(g), _ptr(out)),
                'grid_event[1] outside [-1, n_event)')
    refused(resid(None, _ptr(beta), _ptr(res)), 'NULL')
    refused(resid(h, None, _ptr(res)), 'NULL argument')
    refused(resid(h, _ptr(beta), None), 'NULL argument')
    # the summary: n_time < 1, a group outside [0, n_group)
    eta, lh = np.zeros((1, 2)), np.zeros((1, 2, 1))
    st = _summary(eta, lh, np.array([0, 2], dtype=np.int32))[0]
    refused(st, 'group[1] outside [0, n_group)')
    st = _summary(eta, lh, np.array([-1, 0], dtype=np.int32))[0]
    refused(st, 'group[0] outside [0, n_group)')
    st = _summary(eta, np.zeros((1, 1, 0)), None)[0]
    refused(st, 'n_time')
    # between nuts_begin and the draw's end
    ll, grad = model.compute_loglik_and_gradient(beta)
    model.nuts_begin(np.ones(P), np.ones(P), beta, np.ones(P) * .1, ll, grad,
                     ll - .005 * P, ll - 100.)
    refused(hazard(h, _ptr(beta), 1, 3, _ptr(grid), _ptr(out)),
            'No-U-Turn tree', STATE)
    refused(resid(h, _ptr(beta), _ptr(res)), 'No-U-Turn tree', STATE)
    model.nuts_doubling(.01, 1, 0, np.array([.5]))
    refused(hazard(h, _ptr(beta), 1, 3, _ptr(grid), _ptr(out)),
            'No-U-Turn tree', STATE)
    model.nuts_sample()
    # the handle is as usable as before
    assert hazard(h, _ptr(beta), 1, 3, _ptr(grid), _ptr(out)) == 0
    assert np.isneginf(out[0]) and np.all(np.isfinite(out[1:]))
    assert resid(h, _ptr(beta), _ptr(res)) == 0
    assert _within(res, cpo.residuals(pr.eta(beta), pr.rows), 1e-11)
    assert model.compute_loglik_and_gradient(beta)[0] == ll


# 13 -----------------------------------------------------------------------
def test_prediction_from_a_chain():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior, \
        RegressionModel
    case = cc.cox_case(120, 180, p=6, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((case.event_time, case.censoring_time),
                                case.X, 'cox')
        prior = RegressionCoefPrior(sd_for_intercept=2.,
                                    regularizing_slab_size=1.,
                                    bridge_exponent=.25)
        samples, info = BayesBridge(model, prior).gibbs(
            8, init={'global_scale': .1, 'local_scale': np.ones(6)}, seed=0)
    assert info['coef_sampler_type'] == 'hmc'
    coef = samples['coef']
    assert coef.shape == (6, 8)
    times = np.linspace(0., 125., 40)
    got = model.predict_survival(coef, case.X[::10], times)
    assert got['mean'].shape == (30, 40)
    assert np.all((got['mean'] >= 0.) & (got['mean'] <= 1.))
    assert np.all(np.diff(got['mean'], axis=1) <= 0.)
    assert np.all(got['sd'] >= 0.)
    assert np.all(got['mean'][:, 0] == 1.) and got['mean'][:, -1].max() < 1.
