"""GPU: posterior prediction, log pointwise predictive density and WAIC of the
linear, logit and Poisson models (model.predict on
bbx_design_predictive_summary, csrc/predict.hip) against the NumPy oracle
(tests/predict_oracle.py): four kinds of design, row and draw-block edges,
bit-equality across block sizes and with bbx_design_dot, extreme linear
predictors, new rows centred with the training means, WAIC, prediction after
a chain, and the refusals of the C call.  The oracle's long-double explicit
form is the yardstick; each comparison first checks on the CPU that the
oracle's own float64 recurrence form meets the tolerance the device is held
to."""
import warnings
from ctypes import c_void_p

import numpy as np
import pytest

import predict_cases as pc
import predict_oracle as po

pytestmark = pytest.mark.gpu

# Tolerances, relative to the largest magnitude of the vector compared.  They
# are measured, not chosen: over every input of tests 1, 2, 3, 6 and 7
# (predict_cases.measured_cases) the largest error of the oracle's float64
# recurrence form against its long-double explicit form is MEASURED, and the
# tolerance is 16 x that, rounded up to a power of ten.  The factor covers the
# device's other summation order in X~ beta and its exp / log1p, which differ
# from NumPy's in the last bits: both of the order of the recurrence's own
# rounding.  tests/test_predict_host_logic.py repeats the measurement.
MEASURED = {'mean': 6.27e-16, 'sd': 2.73e-15, 'lpd': 7.29e-16,
            'loglik_mean': 5.32e-16, 'loglik_var': 5.99e-15}
TOL = {'mean': 1e-13, 'sd': 1e-13, 'lpd': 1e-13, 'loglik_mean': 1e-14,
       'loglik_var': 1e-13}


def _design(kind, X, shifted):
    """The design of a case.  With `shifted` the library's own constructors
    (they centre and add the intercept); without, the raw paths that keep
    constant columns (a single row makes every column constant)."""
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if kind in ('dense64', 'dense32'):
        dtype = 'float32' if kind == 'dense32' else 'float64'
        return HipDenseDesignMatrix(X, add_intercept=shifted,
                                    center_predictor=shifted,
                                    storage_dtype=dtype)
    storage = 'csr' if kind == 'csr_valued' else 'tiled'
    X = pc.csr(X)
    if shifted:
        return HipSparseDesignMatrix(X, add_intercept=True,
                                     center_predictor=True, storage=storage)
    return HipSparseDesignMatrix.from_csr_arrays(
        X.shape, X.indptr, X.indices, X.data, add_intercept=False,
        storage=storage)


def _model(case):
    from bayesbridge_amd import RegressionModel
    design = _design(case['kind'], case['X'], case['shifted'])
    assert design.shape == case['Xt'].shape
    if case['shifted']:
        assert np.array_equal(design.column_offset, case['center'])
    outcome = {'linear': case['y'], 'logit': (case['y'], case['n_trial']),
               'poisson': (case['y'], case['exposure'])}[case['family']]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return RegressionModel(outcome, design, case['family'])


def _kw(case):
    return {'obs_prec': case['obs_prec']} if case['family'] == 'linear' \
        else {}


def _new_kw(case, outcome=True):
    """The arguments that carry a case's rows as new rows."""
    kw = dict(_kw(case), X_new=case['X'])
    if outcome:
        kw['y_new'] = case['y']
    if case['family'] == 'logit' and outcome:
        kw['n_trial_new'] = case['n_trial']
    if case['family'] == 'poisson':
        kw['exposure_new'] = case['exposure']
    return kw


def _check(got, case, outcome=True, want=None):
    """The float64 recurrence form within the tolerances of the long-double
    explicit form on the CPU (the inputs are benign), then the device."""
    want = pc.oracle(case, po.explicit, outcome) if want is None else want
    rec = pc.oracle(case, po.recurrence, outcome)
    keys = po.KEYS if outcome else po.KEYS[:2]
    assert set(got) >= set(keys)
    assert outcome == ('lpd' in got)
    for key in keys:
        assert got[key].shape == (case['Xt'].shape[0],)
        print('%-11s oracle f64 vs ext %.2e   device vs ext %.2e   tol %.0e'
              % (key, po.rel_err(rec[key], want[key]),
                 po.rel_err(got[key], want[key]), TOL[key]))
    for key in keys:
        assert np.all(np.isfinite(np.asarray(want[key], dtype=np.float64)))
        assert po.within(rec[key], want[key], TOL[key]), key
    for key in keys:
        assert po.within(got[key], want[key], TOL[key]), key
    return want


def _same_bits(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


# ---- 1. the device against the explicit oracle ------------------------------

@pytest.mark.parametrize('family', po.FAMILIES)
def test_every_family_and_design_matches_the_oracle(family):
    for case in pc.oracle_cases():
        if case['family'] != family:
            continue
        print(case['family'], case['kind'], 'shifted' if case['shifted']
              else 'raw')
        model = _model(case)
        _check(model.predict(case['coef'], **_kw(case)), case)
        # the same rows as new rows without an outcome
        got = model.predict(case['coef'], **_new_kw(case, outcome=False))
        _check(got, case, outcome=False)


# ---- 2. row edges -----------------------------------------------------------

def test_row_edges_and_one_past_65536_rows():
    for case in pc.row_edge_cases():
        n = case['Xt'].shape[0]
        print('n', n, case['kind'])
        got = _model(case).predict(case['coef'], return_draws=True)
        want = _check(got, case)
        assert got['draws'].shape == (n, 5)
        # every row was written, the last one included
        assert po.within(got['draws'], want['mu'], TOL['mean'])


# ---- 3. draw-block edges ----------------------------------------------------

def test_draw_counts_around_the_default_block():
    for case in pc.draw_edge_cases():
        S = case['coef'].shape[1]
        print('S', S)
        model = _model(case)
        if S == 1:
            got = model.predict(case['coef'], **_new_kw(case, outcome=False))
            _check(got, case, outcome=False)
            assert np.all(got['sd'] == 0.)
            # one draw given without a draw axis is the same call
            _same_bits(got, model.predict(
                case['coef'][:, 0], **_new_kw(case, outcome=False)))
            continue
        got = model.predict(case['coef'])
        _check(got, case)
        _same_bits(got, model.predict(case['coef']))


@pytest.mark.parametrize('family', po.FAMILIES)
def test_results_do_not_depend_on_the_block_size(family):
    case, = [c for c in pc.draw_block_cases() if c['family'] == family]
    model = _model(case)
    first = model.predict(case['coef'], return_draws=True, **_kw(case))
    _check(first, case)
    for K in pc.DRAW_BLOCKS:
        _same_bits(first, model.predict(case['coef'], return_draws=True,
                                        _draws_per_pass=K, **_kw(case)))


# ---- 4. the linear predictor is the design's own ----------------------------

@pytest.mark.parametrize('kind', pc.KINDS)
def test_linear_draws_are_the_designs_dot_bit_for_bit(kind):
    case = pc.problem('linear', kind, 1000, 33, 19, 600)
    model = _model(case)
    got = model.predict(case['coef'], return_draws=True, **_kw(case))
    want = np.stack([model.design.dot(b) for b in case['coef'].T]).T
    assert got['draws'].shape == want.shape == (1000, 19)
    assert np.array_equal(got['draws'], want)


# ---- 5. extremes ------------------------------------------------------------

def _raw_model(family, X, y, intercept=False):
    """An uncentred float64 dense design: X~ is X itself, after a column of
    ones with `intercept`."""
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    design = HipDenseDesignMatrix(X, add_intercept=intercept,
                                  center_predictor=False)
    assert design.shape == (X.shape[0], X.shape[1] + int(intercept))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return RegressionModel(y, design, family)


def test_logit_saturates_exactly():
    rs = np.random.RandomState(0)
    sign = np.where(rs.rand(300) < .5, -1., 1.)
    X = np.column_stack((sign, rs.randn(300)))
    y = (sign > 0).astype(np.float64)
    coef = np.zeros((2, 6))
    coef[0] = 800.
    got = _raw_model('logit', X, y).predict(coef)
    assert np.array_equal(got['mean'], y)
    assert np.all(got['sd'] == 0.)
    for key in ('lpd', 'loglik_mean', 'loglik_var'):
        assert np.all(got[key] == 0.), key
    assert got['waic'] == 0.


def test_poisson_overflow_in_one_draw_and_in_all():
    rs = np.random.RandomState(1)
    n, S = 300, 7
    x = rs.randn(n, 1)
    y = rs.poisson(2., n).astype(np.float64)
    coef = np.vstack((.5 + .1 * rs.randn(S), .1 * rs.randn(S)))
    coef[0, 3] = 12000.    # exp overflows in draw 3 (in long double too)
    model = _raw_model('poisson', x, y, intercept=True)
    got = model.predict(coef)
    case = {'family': 'poisson', 'Xt': po.design_matrix(x), 'coef': coef,
            'y': y, 'obs_prec': None, 'offset': np.zeros(n), 'n_trial': None,
            'const': po.ll_const('poisson', y)}
    want = pc.oracle(case, po.explicit)
    assert np.all(want['mean'] == np.inf)
    assert np.all(got['mean'] == np.inf)
    assert np.all(got['loglik_mean'] == -np.inf)
    assert np.all(np.isfinite(got['lpd']))
    assert po.within(pc.oracle(case, po.recurrence)['lpd'], want['lpd'],
                     TOL['lpd'])
    assert po.within(got['lpd'], want['lpd'], TOL['lpd'])
    # every draw overflows: the means are the infinities and lpd is -inf, no
    # NaN among them (the two spreads of infinite values are NaN, as the
    # explicit form's are)
    coef[0] = 12000.
    got = model.predict(coef)
    assert np.all(got['mean'] == np.inf)
    assert np.all(got['loglik_mean'] == -np.inf)
    assert np.all(got['lpd'] == -np.inf) and got['lppd'] == -np.inf
    want = pc.oracle(dict(case, coef=coef), po.explicit)
    assert np.all(want['lpd'] == -np.inf) and np.isnan(want['sd']).all()


def _c_summary(design, family, coef, offset=None, y=None, n_trial=None,
               const=None):
    """The C call on coef (P, S): a dict of the five n-vectors."""
    from bayesbridge_amd import _lib
    n = design.shape[0]
    draws = np.ascontiguousarray(coef.T)
    out = {key: np.full(n, 7.) for key in po.KEYS}
    assert _lib.load().bbx_design_predictive_summary(
        design.handle, family, len(draws), _ptr(draws), None, _ptr(offset),
        _ptr(y), _ptr(n_trial), _ptr(const), 0,
        *[_ptr(out[key]) for key in po.KEYS], None) == 0, _lib.last_error()
    return out


def test_a_nan_stays_a_nan_in_its_rows_only():
    """The products X~ beta carry a NaN coefficient into every row (0 x NaN
    in a dense row, the centring sum <offset, beta> in a sparse one), so
    through a coefficient every row is an affected row.  A NaN that belongs
    to some rows -- here in the row offset -- stays in those rows."""
    from bayesbridge_amd import _lib
    case = pc.problem('logit', 'csr_valued', 300, 3, 5, 700)
    model = _model(case)
    coef = case['coef'].copy()
    coef[2, 1] = np.nan
    got = model.predict(coef)
    for key in po.KEYS:
        assert np.isnan(got[key]).all(), key
    assert np.isnan(got['waic'])
    args = (model.design, _lib.PRED_LOGIT, case['coef'])
    kw = {'y': case['y'], 'n_trial': case['n_trial'], 'const': case['const']}
    offset = np.zeros(300)
    clean = _c_summary(*args, offset=offset, **kw)
    _check(clean, case)
    hit = np.zeros(300, dtype=bool)
    hit[[0, 63, 64, 255, 256, 299]] = True
    offset[hit] = np.nan
    got = _c_summary(*args, offset=offset, **kw)
    for key in po.KEYS:
        assert np.isnan(got[key][hit]).all(), key
        assert np.array_equal(got[key][~hit], clean[key][~hit]), key


# ---- 6. new rows are centred with the training means ------------------------

def test_new_rows_take_the_training_means():
    for case, rows in pc.new_row_cases():
        print(case['kind'])
        model = _model(case)
        sub = pc.subset(case, rows)
        got = model.predict(sub['coef'], **_new_kw(sub))
        want = _check(got, sub)
        # centred with its own means X_new gives another answer, far enough
        # for the tolerance to see it
        own = pc.oracle_matrix(sub['kind'], sub['X'], sub['X'].mean(axis=0),
                               True)
        wrong = pc.oracle(sub, po.explicit, Xt=own)
        for key in ('mean', 'lpd'):
            assert po.rel_err(wrong[key], want[key]) > 100 * TOL[key], key
            assert not po.within(got[key], wrong[key], TOL[key])


# ---- 7. WAIC ----------------------------------------------------------------

def test_waic_of_the_training_rows():
    for case in pc.waic_cases():
        print(case['family'], case['kind'])
        model = _model(case)
        got = model.predict(case['coef'], **_kw(case))
        want = _check(got, case)
        n = len(case['y'])
        lppd, p_waic, waic = (float(v) for v in po.waic(want))
        # n terms, each within its tolerance of the oracle's: the sums are
        # within n times that
        e_lpd = n * TOL['lpd'] * float(np.abs(want['lpd']).max())
        e_var = n * TOL['loglik_var'] * float(np.abs(want['loglik_var']).max())

        def check_sums(res):
            print('lppd %.12g (%.2e)  p_waic %.12g (%.2e)  waic %.12g (%.2e)'
                  % (res['lppd'], res['lppd'] - lppd, res['p_waic'],
                     res['p_waic'] - p_waic, res['waic'], res['waic'] - waic))
            assert abs(res['lppd'] - lppd) <= e_lpd
            assert abs(res['p_waic'] - p_waic) <= e_var
            assert abs(res['waic'] - waic) <= 2 * (e_lpd + e_var)
            assert res['lppd'] == float(np.sum(res['lpd']))
            assert res['p_waic'] == float(np.sum(res['loglik_var']))

        check_sums(got)
        # the training rows passed as new rows with their outcome
        again = model.predict(case['coef'], **_new_kw(case))
        _check(again, case, want=want)
        check_sums(again)


# ---- 8. after a chain -------------------------------------------------------

def _bridge(family, seed):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    case = pc.problem(family, 'tiled_binary' if family == 'logit'
                      else 'dense64', 2000, 30, 2, seed)
    model = _model(case)
    prior = RegressionCoefPrior(bridge_exponent=.5,
                                regularizing_slab_size=2.)
    return case, model, BayesBridge(model, prior)


@pytest.mark.parametrize('family', ['logit', 'linear'])
def test_predict_after_a_chain_and_the_chain_goes_on_unchanged(family):
    case, model, bridge = _bridge(family, 800)
    init = {'global_scale': .1}
    save = ('coef', 'global_scale', 'logp') \
        + (('obs_prec',) if family == 'linear' else ())

    def chain(b):
        return b.gibbs(80, n_burnin=0, thin=1, init=init, seed=5,
                       params_to_save=save)

    samples, info = chain(bridge)
    coef = samples['coef']
    assert coef.shape == (31, 80)
    kw = {}
    if family == 'linear':
        assert samples['obs_prec'].shape == (80,)
        kw['obs_prec'] = samples['obs_prec']
    got = model.predict(coef, **kw)
    run = dict(case, coef=coef, obs_prec=kw.get('obs_prec'))
    _check(got, run)
    assert got['mean'].shape == (2000,) and np.isfinite(got['waic'])
    more, _ = bridge.gibbs_resume(info, n_add_iter=5, merge=False)
    # the same chain without the predict call in between
    _, _, other = _bridge(family, 800)
    samples2, info2 = chain(other)
    assert np.array_equal(samples2['coef'], coef)
    more2, _ = other.gibbs_resume(info2, n_add_iter=5, merge=False)
    assert more['coef'].shape == (31, 5)
    assert np.array_equal(more['coef'], more2['coef'])


# ---- 9. the C call's refusals on the device ---------------------------------

def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def test_c_call_refuses_with_a_message_and_the_design_stays_usable():
    from bayesbridge_amd import _lib
    lib = _lib.load()
    case = pc.problem('linear', 'dense64', 300, 4, 3, 900)
    design = _design('dense64', case['X'], True)
    n, P = design.shape
    coef = np.ascontiguousarray(case['coef'].T)
    tau = np.ascontiguousarray(case['obs_prec'])
    y = np.ascontiguousarray(case['y'])
    out = [np.empty(n) for _ in range(5)]
    LIN, LOGIT = _lib.PRED_LINEAR, _lib.PRED_LOGIT

    def call(design_h=design.handle, family=LIN, n_draw=3, coef=coef,
             tau=tau, y=y, K=0, out=out):
        return lib.bbx_design_predictive_summary(
            design_h, family, n_draw, _ptr(coef), _ptr(tau), None, _ptr(y),
            None, None, K, *[_ptr(a) for a in out], None)

    bad_tau = tau.copy()
    bad_tau[1] = 0.
    nan_tau = tau.copy()
    nan_tau[2] = np.nan
    refusals = [
        (dict(design_h=None), 'design is NULL or destroyed'),
        (dict(family=3), 'family 3'),
        (dict(family=-1), 'family -1'),
        (dict(n_draw=0), 'n_draw must be at least 1'),
        (dict(coef=None), 'coef is NULL'),
        (dict(out=[None] + out[1:]), 'mean is NULL'),
        (dict(out=[out[0], None] + out[2:]), 'sd is NULL'),
        (dict(out=out[:2] + [None] + out[3:]), 'lpd is NULL'),
        (dict(out=out[:3] + [None, out[4]]), 'll_mean is NULL'),
        (dict(out=out[:4] + [None]), 'll_var is NULL'),
        (dict(tau=None), 'linear model needs obs_prec'),
        (dict(family=LOGIT), 'obs_prec is an argument of the linear'),
        (dict(tau=bad_tau), r'obs_prec[1] is not finite and positive'),
        (dict(tau=nan_tau), r'obs_prec[2] is not finite and positive'),
        (dict(K=-1), 'draws_per_pass must not be negative'),
    ]
    v = np.arange(1., P + 1.)
    before = design.dot(v)
    for kw, message in refusals:
        assert call(**kw) == -1, kw
        assert message in _lib.last_error(), (message, _lib.last_error())
        assert np.array_equal(design.dot(v), before)
    assert call() == 0
    want = pc.oracle(case, po.explicit)
    # (no ll_const in this call: the oracle's ll carries it)
    assert po.within(out[0], want['mean'], TOL['mean'])
    assert po.within(out[3] + case['const'], want['loglik_mean'],
                     TOL['loglik_mean'])
    # without y the three score arrays may be NULL
    assert call(y=None, out=out[:2] + [None] * 3) == 0
    # a destroyed design is refused by its address alone
    dead = c_void_p(design.handle.value)
    del design
    assert call(design_h=dead) == -1
    assert 'design is NULL or destroyed' in _lib.last_error()
