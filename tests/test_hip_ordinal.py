"""GPU: the ordinal model (csrc/ordinal.hip on csrc/hamiltonian.hpp,
csrc/ordinal_predict.hip) -- the likelihood, its gradient, its Hessian matvec
and the cutpoint sums against the long-double oracle (tests/ordinal_oracle.py)
at the row counts where the row kernel changes path, the K = 2 model against
the logit handle, bit-equality of the cutpoint sums across n_c and position,
set_cutpoints, infinite and extreme linear predictors, the trajectory against
a host velocity Verlet, No-U-Turn doublings against tests/nuts_oracle.py,
whole seeded chains with sampled cutpoints against the same driver on the
oracle model, prediction against a long-double oracle and the refusals.
There is no reference implementation of this family: the oracle is the
yardstick throughout.

Tolerances are measured: the same formulas in NumPy float64
against the long-double oracle on the test's own inputs; the device gets 4
times that error, because its exp / log1p are not the host's.  The measured
numbers are the constants *_MEASURED below; every test repeats its
measurement, holds the float64 form to the constant first and then the device
to 4 times it."""
import math
import warnings
from ctypes import byref, c_double, c_int, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import logit_oracle as lo
import ordinal_oracle as oo
import predict_oracle as pro
from test_hip_poisson import (KINDS, LAP, NPART, VEC_BLOCK, _compare_doublings,
                              _constant, _design_and_matrix)

pytestmark = pytest.mark.gpu

LD = np.longdouble
RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance

U = _constant('GLM_ROW_U', 'glm_rows.hpp')
ROWS = (1, VEC_BLOCK - 1, VEC_BLOCK + 1, LAP + 1, U * LAP + 3)
P = 23
# K = 2, 3, 7 (one gap of 1e-8, one of 80) and 16
CUTS = {2: np.array([.3]), 3: np.array([-1., 1.5]),
        7: np.array([-3., -1., -1. + 1e-8, .5, 2., 82.]),
        16: np.linspace(-6., 6., 15)}
KS = (2, 3, 7, 16)
ETA_MAX = 50.


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _host_matrix(kind, n, p, seed, center=True):
    """The matrix of test_hip_poisson._design_and_matrix without a device:
    what the tolerances are measured on where there is no GPU."""
    from bayesbridge_amd import simulate
    rs = np.random.RandomState(seed)
    if kind == 'tiled_binary':
        X = simulate.simulate_binary_csr_fast(n, p, .2, seed=seed)
    elif kind == 'csr_valued':
        X = sparse.random(n, p, density=.3, format='csr', random_state=rs)
    elif kind == 'mixed':
        X = simulate.simulate_design_csr(n, p, binary_frac=.8, seed=seed)
    else:
        X = rs.randn(n, p)
    if kind == 'dense32':
        if center:
            X = X - X.mean(axis=0)
        return lo.design(X.astype(np.float32).astype(np.float64), False, False)
    return lo.design(X, center, False)


class _AnyRows:
    """The device model on rows that do not hold every category (a single
    row): the C ABI takes them, the model's constructor does not."""

    def __new__(cls, y, design, offset, K, cuts):
        from bayesbridge_amd import OrdinalModel, cutpoints
        m = object.__new__(OrdinalModel)
        m.y, m.offset = np.asarray(y, dtype=np.float64), offset
        m.n_category, m.design, m.name = K, design, 'ordinal'
        m.cutpoints_fixed = False
        m._cutpoints = np.array(cuts, dtype=np.float64)
        m.cutpoint_prior = cutpoints.check_prior(None)
        m._ham_prefix, m._ordinal = 'bbx_ordinal_', c_void_p()
        m._location_serial = 0
        return m


def _case(kind, n, K, offset, seed, host=False):
    """(model or None, D, y, o, beta, v): every category present (n >= K),
    the coefficients scaled so that max |eta| = ETA_MAX."""
    from bayesbridge_amd import RegressionModel
    center = n > 1          # (a single centred row is a row of zeros)
    if host:
        dsn, D = None, _host_matrix(kind, n, P, seed, center)
    else:
        dsn, D = _design_and_matrix(kind, n, P, False, center, seed)
    rs = np.random.RandomState(seed + 1)
    y = rs.permutation(np.arange(n) % K).astype(np.float64)
    o = rs.randn(n) * .5 if offset else np.zeros(n)
    beta, v = rs.randn(P), rs.randn(P)
    top = np.abs(oo.dot(D, beta)).max()
    beta *= ETA_MAX / (top if top > 0 else 1.)
    model = None
    if not host:
        if n >= K:
            model = RegressionModel((y, o) if offset else y, dsn, 'ordinal',
                                    cutpoints=CUTS[K])
            assert model.name == 'ordinal' and model.design is dsn
        else:
            model = _AnyRows(y, dsn, o, K, CUTS[K])
    return model, D, y, o, beta, v


def _rel(got, want):
    """max |got - want| relative to the largest magnitude of `want`."""
    return pro.rel_err(np.atleast_1d(got), np.atleast_1d(want))


def _candidates(K, rs, n_c=4):
    """n_c cutpoint vectors next to CUTS[K], the first CUTS[K] itself."""
    out = [CUTS[K]]
    while len(out) < n_c:
        c = CUTS[K] + rs.randn(K - 1) * .05
        if np.all(np.diff(c) > 0):
            out.append(c)
    return np.array(out)


def _measure(D, y, o, beta, v, K):
    """The float64 forms against the long-double oracle on these inputs:
    (the oracle's values, the float64 forms' errors)."""
    cuts = CUTS[K]
    cand = _candidates(K, np.random.RandomState(5))
    want = {'loglik': oo.loglik_grad(D, y, o, beta, cuts, LD)}
    want['grad'] = want['loglik'][1]
    want['loglik'] = want['loglik'][0]
    want['hessian'] = oo.hessian_matvec(D, y, o, beta, v, cuts, LD)
    want['cutsum'] = np.array(
        [oo.loglik_grad(D, y, o, beta, c, LD)[0] for c in cand], dtype=LD)
    ll, grad = oo.loglik_grad(D, y, o, beta, cuts)
    f64 = {'loglik': ll, 'grad': grad,
           'hessian': oo.hessian_matvec(D, y, o, beta, v, cuts),
           'cutsum': oo.cutpoint_loglik(D, y, o, beta, cand, np.float64)}
    return want, cand, {key: _rel(f64[key], want[key]) for key in want}


# (kind, n, K, offset): every kind at every row count, K and the offset
# cycling so that every K and both offsets meet every kind and every row
# count, and all K x offset at one shape
CASES = [(kind, n, KS[(a + b) % 4], (a + b // 2) % 2 == 0)
         for a, kind in enumerate(KINDS) for b, n in enumerate(ROWS)] + [
    ('dense64', VEC_BLOCK + 1, K, off) for K in KS for off in (True, False)]

# The largest error of the float64 forms over the CASES of each row count
# (measured on the CPU: `_measure` on `_case(..., host=True)`), relative to the
# largest magnitude of the vector compared; (loglik, grad, hessian, cutsum).
# A single row at |eta| = 50 carries the rounding of eta itself, 50 eps, into
# exp(-50 +- c); the products X~^T w of the long designs cancel.  The device's
# bound is 4 times these (`_bound`).
ROW_MEASURED = {
    1: (2.9e-14, 2.9e-14, 2.9e-14, 3.0e-14),
    VEC_BLOCK - 1: (9.4e-17, 5.7e-16, 7.4e-16, 2.1e-16),
    VEC_BLOCK + 1: (1.3e-16, 1.2e-15, 7.3e-16, 1.9e-16),
    LAP + 1: (1.5e-16, 1.3e-14, 1.1e-14, 3.0e-16),
    U * LAP + 3: (2.7e-16, 2.1e-14, 1.2e-14, 3.1e-16)}
ROW_KEYS = ('loglik', 'grad', 'hessian', 'cutsum')


def _bound(measured):
    """The device's tolerance: 4 times the float64 forms' measured error --
    its exp and log1p are not the host's -- where a measurement below half an
    ulp (a lucky rounding: no float64 result is promised closer) counts as
    half an ulp."""
    return 4 * max(measured, 2. ** -53)


@pytest.mark.parametrize('case', range(len(CASES)))
def test_likelihood_gradient_hessian_and_cutpoint_sums_match_the_oracle(
        case, monkeypatch):
    kind, n, K, offset = CASES[case]
    if n == 1:
        # every column of a single row is "constant", and the design classes
        # drop constant columns as hand-made intercepts: keep them, the row
        # kernel is what this case is about
        from bayesbridge_amd import design_matrix
        monkeypatch.setattr(design_matrix, 'remove_intercept_indicator',
                            lambda X: X)
    model, D, y, o, beta, v = _case(kind, n, K, offset, seed=case)
    assert (o != 0).any() == offset
    if n >= K:
        assert len(set(y)) == K
    eta = oo.dot(D, beta)
    # (a single sparse row may hold no entry at all)
    assert abs(np.abs(eta).max() - ETA_MAX) < 1e-9 or (n == 1 and not
                                                        eta.any())
    want, cand, err64 = _measure(D, y, o, beta, v, K)
    assert np.isfinite(float(want['loglik']))
    ll, grad = model.compute_loglik_and_gradient(beta)
    hv = model.get_hessian_matvec_operator(beta)(v)
    L = model.cutpoint_loglik(beta, cand)
    got = {'loglik': ll, 'grad': grad, 'hessian': hv, 'cutsum': L}
    err = {key: _rel(got[key], want[key]) for key in want}
    measured = dict(zip(ROW_KEYS, ROW_MEASURED[n]))
    for key in ROW_KEYS:
        print('%-12s n %7d K %2d %-7s float64 %.2e device %.2e bound %.2e'
              % (kind, n, K, key, err64[key], err[key],
                 _bound(measured[key])))
    for key in ROW_KEYS:
        assert err64[key] <= measured[key], key
    for key in ROW_KEYS:
        assert err[key] <= _bound(measured[key]), key
    # the same bits on every call; the cached predictor; the handle's own
    # cutpoints are the first candidate and were not touched
    ll2, grad2 = model.compute_loglik_and_gradient(beta)
    assert ll2 == ll and np.array_equal(grad2, grad)
    assert np.array_equal(model.get_hessian_matvec_operator(beta)(v), hv)
    assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
        == (ll, None)
    assert model.hamiltonian_loglik_and_gradient(beta)[0] == ll
    for k in range(len(cand)):
        one = model.cutpoint_loglik(None, cand[k])
        assert isinstance(one, float) and one == L[k]
    assert np.array_equal(model.cutpoints, CUTS[K])
    assert model.compute_loglik_and_gradient(beta)[0] == ll


# d itself, row by row: a diagonal design gives Hv_j = -d_j x_jj^2 v_j, so the
# RELATIVE error of every d_j shows, down to d = 2e-22 at |eta| = 50.  The
# largest relative error of the float64 form on these inputs:
D_MEASURED = 3.5e-16


def test_d_is_relatively_accurate_to_eta_50():
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    n = P
    scale = np.linspace(-ETA_MAX, ETA_MAX, n)
    scale[n // 2] = .25
    X = np.diag(scale)
    dsn = HipDenseDesignMatrix(X, add_intercept=False, center_predictor=False)
    D = lo.design(X, False, False)
    y = (np.arange(n) % 3).astype(np.float64)
    o = np.zeros(n)
    model = RegressionModel(y, dsn, 'ordinal', cutpoints=CUTS[3])
    beta, v = np.ones(n), np.ones(n)
    want = oo.hessian_matvec(D, y, o, beta, v, CUTS[3], LD)
    f64 = oo.hessian_matvec(D, y, o, beta, v, CUTS[3])
    hv = model.get_hessian_matvec_operator(beta)(v)
    assert np.all(want < 0) and float(np.abs(want).min()) < 1e-17
    err64 = float(np.max(np.abs(f64 - want) / np.abs(want)))
    err = float(np.max(np.abs(hv - want) / np.abs(want)))
    print('relative error of d: float64 %.2e device %.2e bound %.2e'
          % (err64, err, _bound(D_MEASURED)))
    assert err64 <= D_MEASURED
    assert err <= _bound(D_MEASURED)


# K = 2, cutpoint 0: the logit model of y >= 1.  Both handles' float64 forms
# against their long-double forms on these inputs (the ordinal oracle, the
# logit oracle's formulas in long double); the two device values may differ
# by 4 times the sum.  Per design kind of the test below.
LOGIT_MEASURED = {'tiled_binary': {'loglik': 2.2e-16, 'grad': 1.9e-14},
                  'dense64': {'loglik': 1.6e-16, 'grad': 7.8e-16}}


@pytest.mark.parametrize('kind,n', [('tiled_binary', LAP + 1),
                                    ('dense64', VEC_BLOCK + 1)])
def test_two_categories_are_the_logit_handle(kind, n):
    from bayesbridge_amd import RegressionModel
    dsn, D = _design_and_matrix(kind, n, P, False, True, 3)
    rs = np.random.RandomState(4)
    y = rs.permutation(np.arange(n) % 2).astype(np.float64)
    beta = rs.randn(P)
    beta *= 8. / np.abs(oo.dot(D, beta)).max()
    model = RegressionModel(y, dsn, 'ordinal', cutpoints=[0.])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        logit = RegressionModel(y, dsn, 'logit')
    ll, grad = model.compute_loglik_and_gradient(beta)
    lll, lgrad = logit.hamiltonian_loglik_and_gradient(beta)
    # the measurement: the logit formulas of logit_oracle in long double
    eta = oo._eta(D, beta, np.zeros(n), LD)
    want_ll = np.sum(y * eta - oo.softplus(eta))
    want_grad = oo._tdot(D, y - oo.sigma(eta), LD)
    o64 = oo.loglik_grad(D, y, np.zeros(n), beta, np.array([0.]))
    l64 = lo.loglik_grad(D, y, np.ones(n), beta)
    err64 = {'loglik': _rel(o64[0], want_ll) + _rel(l64[0], want_ll),
             'grad': _rel(o64[1], want_grad) + _rel(l64[1], want_grad)}
    err = {'loglik': _rel(ll, lll), 'grad': _rel(grad, lgrad)}
    measured = LOGIT_MEASURED[kind]
    for key in err:
        print('%-12s %-6s float64 forms %.2e device handles %.2e bound %.2e'
              % (kind, key, err64[key], err[key], _bound(measured[key])))
    for key in err:
        assert err64[key] <= measured[key], key
        assert err[key] <= _bound(measured[key]), key


@pytest.mark.parametrize('kind,n', [('tiled_binary', U * LAP + 3),
                                    ('dense64', VEC_BLOCK + 1)])
def test_cutpoint_sums_do_not_depend_on_n_c_or_position(kind, n):
    K = 7
    model, D, y, o, beta, v = _case(kind, n, K, True, seed=3)
    rs = np.random.RandomState(2)
    cand = _candidates(K, rs, 8)
    L8 = model.cutpoint_loglik(beta, cand)
    assert len(set(L8)) == 8
    # eight n_c = 1 calls, on the cached eta and on a fresh one
    for k in range(8):
        assert model.cutpoint_loglik(None, cand[k]) == L8[k]
        assert model.cutpoint_loglik(beta, cand[k:k + 1])[0] == L8[k]
    # any position, n_c = 3 and 8
    perm = rs.permutation(8)
    assert np.array_equal(model.cutpoint_loglik(None, cand[perm]), L8[perm])
    for first in (0, 2, 5):
        assert np.array_equal(
            model.cutpoint_loglik(None, cand[first:first + 3]),
            L8[first:first + 3])
    assert np.array_equal(model.cutpoint_loglik(None, cand[[7, 0, 3]]),
                          L8[[7, 0, 3]])
    assert np.array_equal(model.cutpoint_loglik(beta, cand), L8)
    # the handle's own cutpoints: the sum is the likelihood's (the same
    # partials; the two re-add them in their own fixed orders)
    np.testing.assert_allclose(
        L8[0], model.compute_loglik_and_gradient(beta)[0], rtol=1e-13)
    # the cached eta is the last beta's
    other = beta * .5
    Lo = model.cutpoint_loglik(other, cand[:3])
    assert np.array_equal(model.cutpoint_loglik(None, cand[:3]), Lo)
    assert not np.array_equal(Lo, L8[:3])
    for bad in (np.ones((9, K - 1)), np.ones((2, K)), np.ones((0, K - 1))):
        with pytest.raises(ValueError):
            model.cutpoint_loglik(None, bad)


def _small_data(kind, n, p, K=4, seed=0, **model_args):
    """A device model on data simulated from the model (moderate eta), the
    oracle's design, the outcome, the offset and the simulating cutpoints."""
    from bayesbridge_amd import RegressionModel
    dsn, D = _design_and_matrix(kind, n, p, False, True, seed)
    rs = np.random.RandomState(seed + 1)
    beta = rs.randn(p) * .4
    o = rs.randn(n) * .3
    cuts = np.linspace(-1.2, 1.2, K - 1)
    y = oo.simulate(rs, oo.dot(D, beta) + o, cuts)
    assert len(set(y)) == K
    model = RegressionModel((y, o), dsn, 'ordinal', **model_args)
    return model, D, y, o, cuts


def _traj_inputs(D, y, o, cuts, seed=0):
    """f of the preconditioned coordinates and a start next to the maximum of
    the likelihood (see test_hip_poisson._traj_inputs)."""
    n_pred = D[0].shape[1]
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(n_pred) * .3) * .3
    prior_prec = np.ones(n_pred)
    f = oo.precond_f(D, y, o, scale, prior_prec, cuts)
    q0 = oo.newton_mle(D, y, o, cuts) / scale + rs.randn(n_pred) * .02
    p0 = rs.randn(n_pred)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


def _stability_limit(D, y, o, cuts, scale, pp, q0):
    """2 / sqrt(largest curvature of -f at q0), by power iteration on the
    oracle's Hessian."""
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * oo.hessian_matvec(D, y, o, q0 * scale,
                                                scale * v, cuts)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


def test_set_cutpoints_changes_the_gradient_and_invalidates_the_location():
    from bayesbridge_amd import _lib
    model, D, y, o, cuts = _small_data('dense64', 300, 9, seed=4)
    cuts = cuts * 2. + .3          # well away from the empirical logits
    rs = np.random.RandomState(3)
    beta, v = rs.randn(9) * .3, rs.randn(9)
    first = model.cutpoints
    np.testing.assert_array_equal(first, oo.initial_cutpoints(y, 4))
    _, g1 = model.compute_loglik_and_gradient(beta)
    op = model.get_hessian_matvec_operator(beta)
    op(v)
    model.cutpoints = cuts
    _, g2 = model.compute_loglik_and_gradient(beta)
    np.testing.assert_allclose(g1, oo.loglik_grad(D, y, o, beta, first)[1],
                               rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(g2, oo.loglik_grad(D, y, o, beta, cuts)[1],
                               rtol=RTOL, atol=ATOL)
    assert np.abs(g2 - g1).max() > .1
    with pytest.raises(RuntimeError, match='location has moved'):
        op(v)
    # the C call itself: BBX_ERR_STATE until the next set_location
    lib, out = _lib.load(), np.empty(9)
    assert lib.bbx_ordinal_hessian_matvec(model.handle, _ptr(v), _ptr(out)) \
        == -5
    assert 'set_location' in _lib.last_error()
    np.testing.assert_allclose(
        model.get_hessian_matvec_operator(beta)(v),
        oo.hessian_matvec(D, y, o, beta, v, cuts), rtol=RTOL, atol=ATOL)
    # refused while a No-U-Turn tree is open, accepted once its sample is
    # taken
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, y, o, cuts)
    joint = logp0 - .5 * np.dot(p0, p0)
    model.nuts_begin(scale, pp, q0, p0, logp0, grad0, joint, joint - 1.)
    with pytest.raises(_lib.BbxError, match='No-U-Turn tree'):
        model.cutpoints = first
    assert np.array_equal(model.cutpoints, cuts)
    # ... while the cutpoint sums may be asked for
    L = model.cutpoint_loglik(beta, first)
    np.testing.assert_allclose(L, oo.cutpoint_loglik(D, y, o, beta, first),
                               rtol=RTOL, atol=ATOL)
    model.nuts_sample()
    model.cutpoints = first
    assert np.array_equal(model.cutpoints, first)
    np.testing.assert_allclose(model.compute_loglik_and_gradient(beta)[1], g1,
                               rtol=0, atol=0)


# The float64 forms' errors at |eta| = 745 (the inputs of the test below):
# every term is 745 -+ c or a rounding of 0 or 1, so float64 is all but exact
# and the bound is `_bound`'s floor.  d = exp(-745) is a denormal there (the
# float64 form itself is 13 % off the long double's): the Hessian product is
# only asked to be finite and below 1e-300.
EXTREME_MEASURED = {'loglik': 3.7e-17, 'grad': 4.4e-18}


def test_infinite_and_extreme_linear_predictors():
    """|eta| = 745 (exp(-745) is the last denormal) stays finite; eta = +-inf
    gives (-inf, None) and an unstable trajectory where a row's category has
    probability 0, and ll = 0, w = 0 in the end category on that side."""
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    rs = np.random.RandomState(5)
    n, cuts = VEC_BLOCK + 1, CUTS[3]
    X = rs.randn(n, 3)
    X[:, 0] = np.where(np.arange(n) % 2 == 0, 1., -1.)
    dsn = HipDenseDesignMatrix(X, add_intercept=False, center_predictor=False)
    D = lo.design(X, False, False)
    o = np.zeros(n)
    y = (np.arange(n) % 3).astype(np.float64)
    model = RegressionModel(y, dsn, 'ordinal', cutpoints=cuts)
    beta, v = np.array([745., 0., 0.]), rs.randn(3)
    assert set(np.abs(oo.dot(D, beta))) == {745.}
    want = dict(zip(('loglik', 'grad'),
                    oo.loglik_grad(D, y, o, beta, cuts, LD)))
    f64 = dict(zip(('loglik', 'grad'), oo.loglik_grad(D, y, o, beta, cuts)))
    ll, grad = model.compute_loglik_and_gradient(beta)
    got = {'loglik': ll, 'grad': grad}
    assert np.isfinite(ll) and np.all(np.isfinite(grad))
    for key in want:
        e64, e = _rel(f64[key], want[key]), _rel(got[key], want[key])
        print('|eta| = 745 %-7s float64 %.2e device %.2e bound %.2e'
              % (key, e64, e, _bound(EXTREME_MEASURED[key])))
        assert e64 <= EXTREME_MEASURED[key], key
        assert e <= _bound(EXTREME_MEASURED[key]), key
    hv = model.get_hessian_matvec_operator(beta)(v)
    assert np.all(np.isfinite(hv)) and np.abs(hv).max() < 1e-300
    # eta = +-inf in alternating rows, every category on both sides: some
    # row's category has probability 0
    bad = np.array([np.inf, .1, .2])
    with np.errstate(all='ignore'):
        assert oo.loglik_grad(D, y, o, bad, cuts)[0] == -np.inf
    assert model.compute_loglik_and_gradient(bad) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(bad, loglik_only=True) \
        == (-np.inf, None)
    assert model.compute_loglik_and_gradient(-bad) == (-np.inf, None)
    nan = np.array([np.nan, .1, .2])
    assert np.isnan(model.compute_loglik_and_gradient(nan)[0])
    # the flags were that evaluation's only
    small = np.array([.1, .3, .2])
    ll, grad = model.compute_loglik_and_gradient(small)
    np.testing.assert_allclose(ll, oo.loglik_grad(D, y, o, small, cuts)[0],
                               rtol=RTOL, atol=ATOL)
    # the end categories (K = 2: both are): the rows at +inf all in 1, those
    # at -inf all in 0 -- every probability is 1, so the likelihood is 0, and
    # w = 0 and d = 0 in every row: the gradient and the Hessian product are 0
    y_end = np.where(X[:, 0] > 0, 1., 0.)
    ends = RegressionModel(y_end, dsn, 'ordinal', cutpoints=CUTS[2])
    far = np.array([np.inf, .1, .2])
    with np.errstate(all='ignore'):
        oll, ograd = oo.loglik_grad(D, y_end, o, far, CUTS[2])
    assert oll == 0. and np.all(ograd == 0.)
    ll, grad = ends.compute_loglik_and_gradient(far)
    assert ll == 0. and grad is not None and np.all(grad == 0.)
    assert np.all(ends.get_hessian_matvec_operator(far)(v) == 0.)
    # the other side: every row's category has probability 0 there
    assert ends.compute_loglik_and_gradient(-far) == (-np.inf, None)
    # a trajectory whose first step sends a coefficient to -inf: no HIP
    # error, instability at step 1
    scale, pp = np.ones(3), np.ones(3)
    f = oo.precond_f(D, y, o, scale, pp, cuts)
    q0 = small.copy()
    p0 = np.array([-1e300, .1, .1])
    logp0, grad0 = f(q0)
    with np.errstate(all='ignore'):
        want = lo.trajectory(f, 1e10, 10, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(1e10, 10, scale, pp, q0, p0, logp0, grad0)
    assert want[5] and want[4] == 1 and want[2] == -np.inf
    assert got['instability'] is True and got['n_steps'] == 1
    assert got['logp'] == -np.inf and got['grad'] is None
    assert got['q'][0] == -np.inf
    assert got['hamiltonian'][1] == np.inf
    ll2, grad2 = model.compute_loglik_and_gradient(small)
    ll1, grad1 = model.compute_loglik_and_gradient(small)
    assert ll2 == ll1 and np.array_equal(grad2, grad1)
    np.testing.assert_allclose(model.design.dot(v), lo.dot(D, v), rtol=RTOL,
                               atol=ATOL)


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_trajectory_matches_host_velocity_verlet(kind):
    model, D, y, o, cuts = _small_data(kind, 3 * VEC_BLOCK + 5, P)
    model.cutpoints = cuts
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, y, o, cuts)
    limit = _stability_limit(D, y, o, cuts, scale, pp, q0)
    dt = limit / 4
    print('stability limit', limit)
    want = lo.trajectory(f, dt, 64, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(dt, 64, scale, pp, q0, p0, logp0, grad0)
    assert not want[5] and not got['instability']
    assert got['n_steps'] == want[4] == 64
    for key, ref in (('q', want[0]), ('p', want[1]), ('grad', want[3])):
        print(key, np.abs(got[key] - ref).max() / np.abs(ref).max())
        np.testing.assert_allclose(got[key], ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['logp'], want[2], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['hamiltonian'], [want[6], want[7]],
                               rtol=RTOL, atol=ATOL)
    again = model.hmc_trajectory(dt, 64, scale, pp, q0, p0, logp0, grad0)
    for key in ('q', 'p', 'grad', 'hamiltonian'):
        assert np.array_equal(again[key], got[key])
    assert again['logp'] == got['logp']


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_nuts_doublings_match_the_oracle(kind):
    model, D, y, o, cuts = _small_data(kind, 3 * VEC_BLOCK + 5, P)
    model.cutpoints = cuts
    oracle = oo.OracleModel(D, y, o, cutpoints=cuts)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, y, o, cuts)
    limit = _stability_limit(D, y, o, cuts, scale, pp, q0)
    args = (model, oracle, scale, pp, q0, p0, logp0, grad0)
    # every height up to 4 in both directions: a step small enough for the
    # 31 steps to make no U-turn
    for first in (1, -1):
        directions = [first * (-1) ** h for h in range(5)]
        outs = _compare_doublings(*args, limit / 40, directions, 100., 5)
        assert [out['height'] for out in outs] == [1, 2, 3, 4, 5]
        assert sum(out['n_steps'] for out in outs) == 31
        assert not any(out['doubling_rejected'] for out in outs)
    # a step at which the tree turns round within 2^6 steps
    outs = _compare_doublings(*args, limit / 4, [1, 1, -1, 1, -1, 1, 1], 100.,
                              6)
    assert outs[-1]['u_turn_detected']
    assert not outs[-1]['instability_detected']


# ------------------------------------------------------------ whole chains
CHAIN_N, CHAIN_P, CHAIN_K = 2 * VEC_BLOCK + 37, 12, 4
CHAIN_ITER = {'hmc': 6, 'nuts': 8}
# A chain multiplies a rounding difference from iteration to iteration (see
# test_hip_negbin.py).  The seeds were chosen on the oracle alone, on the CPU:
# for seeds 0 to 23 the oracle's own chain was run again with its likelihood,
# its gradient and L(c) perturbed by 1e-11 relative and by +-1e-14 relative,
# and compared with itself at this file's tolerance, rtol 1e-6 / atol 1e-9,
# over every saved parameter and the sampling info.  SEED_SEARCH records the
# outcome: in every case more than two thirds of the seeds are unchanged at
# 1e-11 and all at 1e-14; the seeds taken are the ones that move least.
CHAIN_SEED = {('hmc', 'sparse'): 17, ('hmc', 'dense'): 0,
              ('nuts', 'sparse'): 22, ('nuts', 'dense'): 16}
# (seeds tried, unchanged at 1e-11, unchanged at both +-1e-14), and the taken
# seed's largest deviation in units of the tolerance at 1e-11 / 1e-14
SEED_SEARCH = {('hmc', 'sparse'): (24, 19, 24, .020, 4.9e-5),
               ('hmc', 'dense'): (24, 17, 24, .0062, 3.8e-5),
               ('nuts', 'sparse'): (24, 23, 24, .011, 1.8e-5),
               ('nuts', 'dense'): (24, 24, 24, .0050, 1.8e-5)}


def _chain_problem(fmt):
    rs = np.random.RandomState(11)
    if fmt == 'sparse':
        X = sparse.random(CHAIN_N, CHAIN_P, density=.3, format='csr',
                          random_state=rs)
        X.data[:] = 1.
    else:
        X = rs.randn(CHAIN_N, CHAIN_P) * .5
    beta = np.zeros(CHAIN_P)
    beta[:4] = (.8, -.6, .4, -.3)
    o = rs.randn(CHAIN_N) * .3
    cuts = np.array([-1., 0., 1.2])
    y = oo.simulate(rs, np.asarray(X.dot(beta)).ravel() + o, cuts)
    assert len(set(y)) == CHAIN_K
    return X, y, o


class _HostDesign:
    """What the Gibbs driver reads of a design, for the oracle chain on a
    machine without a GPU (the choice of seeds)."""
    use_hip, is_sparse, intercept_added = True, False, False

    def __init__(self, X):
        self.shape = X.shape
        self.column_offset = np.asarray(X.mean(axis=0)).ravel()


def _chain(fmt, method, seed, oracle=False, n_iter=None, resume=None,
           perturb=0., host=False, **model_args):
    """`n_iter` Gibbs iterations on the device model, or on the oracle model
    behind the same design object.  The chain starts at given coefficients,
    so no mode search runs; the cutpoints start at the empirical logits."""
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, y, o = _chain_problem(fmt)
    n_iter = n_iter or CHAIN_ITER[method]
    if host:
        dsn = _HostDesign(X)
    else:
        model = RegressionModel((y, o), X, 'ordinal', **model_args)
        dsn = model.design
    D0 = lo.design(X, True, False)
    if oracle:
        D = lo.design(X, True, False, offset=dsn.column_offset)
        model = oo.OracleModel(D, y, o, design=dsn, perturb=perturb,
                               **model_args)
    prior = RegressionCoefPrior(bridge_exponent=.5,
                                regularizing_slab_size=1.)
    start = oo.newton_mle(D0, y, o, oo.initial_cutpoints(y, CHAIN_K))
    init = {'coef': start, 'global_scale': .1}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            samples, info = BayesBridge(model, prior).gibbs(
                n_iter, init=init, seed=seed, params_to_save='all',
                coef_sampler_type=method)
            if resume:
                samples, info = BayesBridge(model, prior).gibbs_resume(
                    info, resume, merge=True, prev_samples=samples)
    return samples, info


CHAIN_KEYS = ('coef', 'global_scale', 'logp', 'local_scale', 'cutpoints')


@pytest.mark.parametrize('method,fmt', [('hmc', 'dense'), ('hmc', 'sparse'),
                                        ('nuts', 'dense'), ('nuts', 'sparse')])
def test_seeded_chain_matches_the_driver_on_the_oracle(method, fmt):
    from bayesbridge_amd.bayesbridge import HMC_INFO_KEYS, NUTS_INFO_KEYS
    seed = CHAIN_SEED[method, fmt]
    samples, info = _chain(fmt, method, seed)
    want, winfo = _chain(fmt, method, seed, oracle=True)
    assert info['coef_sampler_type'] == method
    assert info['options']['rng'] == 'reference'
    assert set(samples) == set(CHAIN_KEYS)
    assert 'obs_prec' not in info['_markov_chain_state']
    n_iter = CHAIN_ITER[method]
    assert samples['coef'].shape == (CHAIN_P, n_iter)
    assert samples['cutpoints'].shape == (CHAIN_K - 1, n_iter)
    assert len(set(samples['cutpoints'][0])) == n_iter
    assert np.array_equal(info['_markov_chain_state']['cutpoints'],
                          samples['cutpoints'][:, -1])
    si, wsi = (i['_reg_coef_sampling_info'] for i in (info, winfo))
    assert set(si) == set(wsi) == set(HMC_INFO_KEYS if method == 'hmc'
                                      else NUTS_INFO_KEYS)
    print('cutpoints', samples['cutpoints'][:, -1], 'n_grad_evals',
          si['n_grad_evals'], 'max rel coef',
          np.max(np.abs(samples['coef'] - want['coef'])
                 / (np.abs(want['coef']) + 1e-3)), 'max abs cutpoints',
          np.max(np.abs(samples['cutpoints'] - want['cutpoints'])))
    for key in CHAIN_KEYS:
        np.testing.assert_allclose(samples[key], want[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)
    for key in si:
        np.testing.assert_allclose(si[key], wsi[key], rtol=RTOL, atol=ATOL,
                                   err_msg=key)
    assert np.all(si['n_grad_evals'] > 1)
    # two halves through gibbs_resume against the straight run: bit for bit
    half = n_iter // 2
    resumed, rinfo = _chain(fmt, method, seed, n_iter=half,
                            resume=n_iter - half)
    assert rinfo['n_iter'] == n_iter
    for key in samples:
        assert np.array_equal(resumed[key], samples[key]), key
    for key in si:
        assert np.array_equal(rinfo['_reg_coef_sampling_info'][key],
                              si[key]), key


def test_fixed_cutpoint_chain_draws_no_uniforms_for_them(monkeypatch):
    """cutpoints=[...]: samples['cutpoints'] is constant, the slice updates
    never run -- the chain consumes the uniforms of a chain without cutpoints
    -- and it matches the driver on the oracle with the same fixed values."""
    from bayesbridge_amd import bayesbridge, dispersion
    held = np.array([-.9, .1, 1.1])
    slices = [0]
    real = dispersion.slice_update

    def counting(*args, **kw):
        slices[0] += 1
        return real(*args, **kw)

    from bayesbridge_amd import cutpoints as cutpoints_module
    monkeypatch.setattr(cutpoints_module, 'slice_update', counting)
    fixed, info = _chain('dense', 'nuts', 1, n_iter=4, cutpoints=held)
    assert slices[0] == 0
    want, _ = _chain('dense', 'nuts', 1, n_iter=4, oracle=True,
                     cutpoints=held)
    assert np.all(fixed['cutpoints'] == held[:, None])
    assert np.array_equal(info['_markov_chain_state']['cutpoints'], held)
    for key in CHAIN_KEYS:
        np.testing.assert_allclose(fixed[key], want[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)
    # a sampled chain runs K - 1 slice updates per iteration
    _chain('dense', 'nuts', 1, n_iter=2)
    assert slices[0] == 2 * (CHAIN_K - 1)

    def never(*args, **kw):
        raise AssertionError("the cutpoints are fixed")

    monkeypatch.setattr(bayesbridge, 'update_cutpoints', never)
    again, _ = _chain('dense', 'nuts', 1, n_iter=4, cutpoints=held)
    for key in CHAIN_KEYS:
        assert np.array_equal(again[key], fixed[key]), key


def test_default_sampler_mode_search_and_initial_cutpoints():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, y, o = _chain_problem('dense')
    model = RegressionModel((y, o), X, 'ordinal', cutpoint_prior={'sd': 3.})
    assert not model.intercept_added
    prior = RegressionCoefPrior(bridge_exponent=.5,
                                regularizing_slab_size=1.)
    start = np.array([-.8, .1, 1.])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        samples, info = BayesBridge(model, prior).gibbs(
            3, init={'global_scale': .1, 'cutpoints': start}, seed=1,
            params_to_save=('coef', 'cutpoints'))
    assert info['coef_sampler_type'] == 'hmc'
    assert info['options']['rng'] == 'reference'
    assert info['_init_optim_info']['is_success']
    assert np.array_equal(info['init']['cutpoints'], start)
    assert set(samples) == {'coef', 'cutpoints'}
    assert np.all(np.isfinite(samples['coef']))
    assert np.all(np.diff(samples['cutpoints'], axis=0) > 0)
    assert np.array_equal(model.cutpoints, samples['cutpoints'][:, -1])
    # the search went uphill from its start, at the initial cutpoints
    D = lo.design(X, True, False, offset=model.design.column_offset)
    assert oo.loglik_grad(D, y, o, info['init']['coef'], start)[0] > \
        oo.loglik_grad(D, y, o, np.zeros(CHAIN_P), start)[0]


def test_refusals_are_exceptions():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior, SamplerOptions
    model, D, y, o, cuts = _small_data('dense64', 100, 20)
    bridge = BayesBridge(model, RegressionCoefPrior(bridge_exponent=.5))
    init = {'global_scale': .1}
    for method in ('cg', 'cholesky', 'woodbury'):
        with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
            bridge.gibbs(2, init=init, seed=0, coef_sampler_type=method)
        with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
            bridge.gibbs(2, init=init, seed=0, options=SamplerOptions(method))
    with pytest.raises(ValueError):
        bridge.gibbs(2, init=init, seed=0, options={'rng': 'device'})
    with pytest.raises(ValueError, match="'cg'"):
        bridge.gibbs_batch([0, 1], 2, init=init)
    with pytest.raises(ValueError, match="'cg' only"):
        bridge.gibbs_multichain(2, 2, init=init)
    with pytest.raises(ValueError):
        model.compute_loglik_and_gradient(np.zeros(21))


# ------------------------------------------------------------- prediction
# The largest error of the oracle's float64 recurrence against its long-double
# explicit form on the inputs of the test below, relative to the largest
# magnitude of the array compared (measured on the CPU); 'rowsum': the largest
# |sum_k mean_k - 1| of the recurrence.  The device gets 4 times these.
PREDICT_MEASURED = {'mean': 3.1e-16, 'sd': 1.3e-15, 'lpd': 2.3e-16,
                    'loglik_mean': 3.8e-16, 'loglik_var': 1.2e-15,
                    'rowsum': 4.5e-16}


def _predict_case():
    rs = np.random.RandomState(31)
    n, p, S, K = 2 * VEC_BLOCK + 37, 9, 37, 5
    X = rs.randn(n, p) * .6
    o = rs.randn(n) * .3
    truth = rs.randn(p) * .5
    base = np.array([-1.5, -.4, .5, 1.6])
    y = oo.simulate(rs, X.dot(truth) + o, base)
    assert len(set(y)) == K
    coef = truth[:, None] + rs.randn(p, S) * .05
    cuts = np.sort(base[:, None] + rs.randn(K - 1, S) * .08, axis=0)
    assert np.all(np.diff(cuts, axis=0) > 0)
    return X, o, y, coef, cuts


def test_predict_matches_the_long_double_oracle():
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    X, o, y, coef, cuts = _predict_case()
    K = cuts.shape[0] + 1
    dsn = HipDenseDesignMatrix(X, add_intercept=False, center_predictor=True)
    model = RegressionModel((y, o), dsn, 'ordinal')
    Xt = pro.design_matrix(X, dsn.column_offset, False)
    want = oo.predict_explicit(Xt, coef, cuts, y, o)
    rec = oo.predict_recurrence(Xt, coef, cuts, y, o)
    got = model.predict(coef, cuts)
    rowsum = {'rec': float(np.abs(rec['mean'].sum(axis=1) - 1).max()),
              'got': float(np.abs(got['mean'].sum(axis=1) - 1).max())}
    bound = {key: _bound(m) for key, m in PREDICT_MEASURED.items()}
    for key in pro.KEYS:
        print('%-11s oracle f64 vs ext %.2e   device vs ext %.2e   bound %.2e'
              % (key, pro.rel_err(rec[key], want[key]),
                 pro.rel_err(got[key], want[key]), bound[key]))
    print('rows of mean sum to 1 within: f64 %.2e device %.2e bound %.2e'
          % (rowsum['rec'], rowsum['got'], bound['rowsum']))
    for key in pro.KEYS:
        assert pro.within(rec[key], want[key], PREDICT_MEASURED[key]), key
    assert rowsum['rec'] <= PREDICT_MEASURED['rowsum']
    for key in pro.KEYS:
        assert got[key].shape == ((len(y), K) if key in ('mean', 'sd')
                                  else (len(y),))
        assert pro.within(got[key], want[key], bound[key]), key
    assert rowsum['got'] <= bound['rowsum']
    lppd, p_waic, waic = pro.waic(want)
    for key, value in (('lppd', lppd), ('p_waic', p_waic), ('waic', waic)):
        np.testing.assert_allclose(got[key], float(value), rtol=1e-12)
    # no result depends on the draws per pass
    for per in (1, 16, 37):
        other = model.predict(coef, cuts, _draws_per_pass=per)
        assert set(other) == set(got)
        for key in got:
            assert np.array_equal(other[key], got[key]), (per, key)
    # one cutpoint vector is that vector for every draw; new rows without an
    # outcome give the probabilities only
    one = model.predict(coef, cuts[:, 0])
    same = model.predict(coef, np.repeat(cuts[:, :1], coef.shape[1], axis=1))
    for key in one:
        assert np.array_equal(one[key], same[key]), key
    new = model.predict(coef, cuts, X_new=X, offset_new=o)
    assert set(new) == {'mean', 'sd'}
    assert np.array_equal(new['mean'], got['mean'])
    scored = model.predict(coef, cuts, X_new=X, offset_new=o, y_new=y)
    assert np.array_equal(scored['lpd'], got['lpd'])
    for bad in (np.ones(3), cuts[::-1], np.full(cuts.shape, np.nan),
                cuts[:, :5]):
        with pytest.raises(ValueError):
            model.predict(coef, bad)
    with pytest.raises(ValueError):
        model.predict(coef, cuts, X_new=X, y_new=np.full(len(y), K))


def test_the_other_summaries_still_refuse_this_family():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    design = HipDenseDesignMatrix(rs.randn(40, 3), add_intercept=False)
    coef, y = rs.randn(2, 3) * .1, np.ones(40)
    cuts = np.array([[-1., 1.], [-.5, .8]])
    out = [np.empty(40) for _ in range(5)]
    # the shared summary knows three families; the negative-binomial one
    # wants a dispersion
    for family in (3, 4):
        st = lib.bbx_design_predictive_summary(
            design.handle, family, 2, _ptr(coef), None, None, _ptr(y), None,
            None, 0, *[_ptr(a) for a in out], None)
        assert st == -1 and 'family %d' % family in _lib.last_error()
    assert lib.bbx_design_predictive_summary_negbin(
        design.handle, 2, _ptr(coef), None, None, _ptr(y), None, 0,
        *[_ptr(a) for a in out], None) == -1
    # the family's own call refuses what it must, with the design usable
    mean, sd = np.empty((3, 40)), np.empty((3, 40))

    def call(K=3, coef=coef, cuts=cuts, offset=None, y=y, per=0, mean=mean,
             sd=sd, score=out[2:]):
        return lib.bbx_design_predictive_summary_ordinal(
            design.handle, 2, K, _ptr(coef), _ptr(cuts), _ptr(offset),
            _ptr(y), per, _ptr(mean), _ptr(sd), *[_ptr(a) for a in score])

    for kw in (dict(K=1), dict(K=17), dict(coef=None), dict(cuts=None),
               dict(mean=None), dict(sd=None), dict(per=-1),
               dict(score=[None, None, None]),
               dict(cuts=np.array([[-1., 1.], [.8, -.5]])),
               dict(cuts=np.array([[-1., 1.], [.8, np.inf]])),
               dict(y=np.where(np.arange(40) == 7, 3., y)),
               dict(y=np.where(np.arange(40) == 7, .5, y)),
               dict(offset=np.where(np.arange(40) == 7, np.nan, 0.))):
        assert call(**kw) == -1, kw
        assert _lib.last_error()
    assert lib.bbx_design_predictive_summary_ordinal(
        None, 2, 3, _ptr(coef), _ptr(cuts), None, _ptr(y), 0, _ptr(mean),
        _ptr(sd), *[_ptr(a) for a in out[2:]]) == -1
    assert call() == 0
    assert np.all(np.isfinite(out[2]))
    np.testing.assert_allclose(mean.sum(axis=0), 1., rtol=0, atol=1e-14)
    assert call(y=None, score=[None, None, None]) == 0


def test_c_abi_errors_are_status_codes():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    n, p = 50, 4
    design = HipDenseDesignMatrix(rs.randn(n, p), add_intercept=False)
    y, o = (np.arange(n) % 3).astype(np.float64), np.full(n, .5)
    cuts = np.array([-1., 1.])
    vec, out = rs.randn(p) * .1, np.empty(p)
    ll, k = c_double(), c_int()
    null = c_void_p()
    assert lib.bbx_ordinal_loglik_grad(null, _ptr(vec), byref(ll), None) < 0
    assert lib.bbx_ordinal_set_location(null, _ptr(vec)) < 0
    assert lib.bbx_ordinal_set_cutpoints(null, _ptr(cuts)) < 0
    assert lib.bbx_ordinal_destroy(null) == 0
    # bad arguments at create
    h = c_void_p()
    assert lib.bbx_ordinal_create(design.handle, _ptr(y), _ptr(o), 3,
                                  _ptr(cuts), None) < 0
    assert lib.bbx_ordinal_create(null, _ptr(y), _ptr(o), 3, _ptr(cuts),
                                  byref(h)) < 0
    assert lib.bbx_ordinal_create(design.handle, None, _ptr(o), 3, _ptr(cuts),
                                  byref(h)) < 0
    assert lib.bbx_ordinal_create(design.handle, _ptr(y), _ptr(o), 3, None,
                                  byref(h)) < 0
    at = np.arange(n)
    for bad_y, bad_o, K, bad_c in (
            (np.where(at == 7, -1., y), o, 3, cuts),
            (np.where(at == 7, 3., y), o, 3, cuts),       # out of range
            (np.where(at == 7, 1.5, y), o, 3, cuts),
            (np.where(at == 7, np.nan, y), o, 3, cuts),
            (np.where(at == 7, np.inf, y), o, 3, cuts),
            (y, np.where(at == 9, np.inf, o), 3, cuts),
            (y, np.where(at == 9, np.nan, o), 3, cuts),
            (np.zeros(n), o, 1, cuts), (y, o, 17, np.arange(16.)),
            (y, o, 0, cuts), (y, o, -3, cuts),
            (y, o, 3, np.array([1., -1.])), (y, o, 3, np.array([1., 1.])),
            (y, o, 3, np.array([-1., np.inf])),
            (y, o, 3, np.array([np.nan, 1.]))):
        bad_y, bad_o = np.ascontiguousarray(bad_y), np.ascontiguousarray(bad_o)
        assert lib.bbx_ordinal_create(design.handle, _ptr(bad_y), _ptr(bad_o),
                                      K, _ptr(bad_c), byref(h)) == -1
        assert not h.value
        assert _lib.last_error()
    # no offset: offset = NULL; K = 16 is the largest
    h0, h16 = c_void_p(), c_void_p()
    assert lib.bbx_ordinal_create(design.handle, _ptr(y), None, 3, _ptr(cuts),
                                  byref(h0)) == 0
    assert lib.bbx_ordinal_create(design.handle, _ptr(y), None, 16,
                                  _ptr(np.arange(15.)), byref(h16)) == 0
    assert lib.bbx_ordinal_destroy(h16) == 0
    assert lib.bbx_ordinal_create(design.handle, _ptr(y), _ptr(o), 3,
                                  _ptr(cuts), byref(h)) == 0
    # order of calls
    assert lib.bbx_ordinal_hessian_matvec(h, _ptr(vec), _ptr(out)) == -5
    assert 'set_location' in _lib.last_error()
    u = rs.rand(1)
    assert lib.bbx_ordinal_nuts_doubling(h, .1, 1, 0, _ptr(u), byref(k),
                                         byref(k), None, None, None) < 0
    assert 'nuts_begin' in _lib.last_error()
    cc = np.array([[-1., 1.], [-.5, .5], [0., 2.]])
    L = np.empty(8)
    assert lib.bbx_ordinal_cutpoint_loglik(h, None, 3, _ptr(cc), _ptr(L)) == -5
    assert 'cached' in _lib.last_error()
    for n_c in (0, 9, -1):
        assert lib.bbx_ordinal_cutpoint_loglik(h, _ptr(vec), n_c, _ptr(cc),
                                               _ptr(L)) == -1
    for bad in ([.5, -.5], [.5, .5], [-.5, np.inf], [np.nan, .5]):
        bad_cc = cc.copy()
        bad_cc[1] = bad
        assert lib.bbx_ordinal_cutpoint_loglik(h, _ptr(vec), 3, _ptr(bad_cc),
                                               _ptr(L)) == -1
        assert 'cuts[1]' in _lib.last_error()
        assert lib.bbx_ordinal_set_cutpoints(h, _ptr(np.array(bad))) == -1
    assert lib.bbx_ordinal_set_cutpoints(h, None) == -1
    assert lib.bbx_ordinal_cutpoint_loglik(h, _ptr(vec), 3, None,
                                           _ptr(L)) == -1
    assert lib.bbx_ordinal_cutpoint_loglik(h, _ptr(vec), 3, _ptr(cc),
                                           None) == -1
    # a refused call with beta cached nothing
    assert lib.bbx_ordinal_cutpoint_loglik(h, None, 3, _ptr(cc), _ptr(L)) == -5
    assert lib.bbx_ordinal_cutpoint_loglik(h, _ptr(vec), 3, _ptr(cc),
                                           _ptr(L)) == 0
    assert lib.bbx_ordinal_cutpoint_loglik(h, None, 3, _ptr(cc), _ptr(L)) == 0
    assert np.all(np.isfinite(L[:3]))
    # the design and the handles work afterwards
    ll0 = c_double()
    assert lib.bbx_ordinal_loglik_grad(h0, _ptr(vec), byref(ll0), None) == 0
    assert lib.bbx_ordinal_loglik_grad(h, _ptr(vec), byref(ll), _ptr(out)) == 0
    assert np.isfinite(ll.value) and ll.value != ll0.value
    np.testing.assert_allclose(ll.value, L[0], rtol=1e-13)
    assert lib.bbx_ordinal_set_cutpoints(h, _ptr(cc[2])) == 0
    assert lib.bbx_ordinal_loglik_grad(h, _ptr(vec), byref(ll0), None) == 0
    np.testing.assert_allclose(ll0.value, L[2], rtol=1e-13)
    assert lib.bbx_ordinal_destroy(h0) == 0
    # use after the design is destroyed
    design.__del__()
    assert lib.bbx_ordinal_loglik_grad(h, _ptr(vec), byref(ll), None) < 0
    assert 'destroyed' in _lib.last_error()
    assert lib.bbx_ordinal_set_cutpoints(h, _ptr(cuts)) < 0
    assert lib.bbx_ordinal_destroy(h) == 0
