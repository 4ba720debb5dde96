"""GPU: the Weibull model (csrc/weibull.hip on csrc/glm_rows.hpp and
csrc/hamiltonian.hpp, csrc/weibull_predict.hip) -- the likelihood, its
gradient, its Hessian matvec and the shape sums against the long-double oracle
(tests/weibull_oracle.py) at the row counts where the row kernel changes path,
the exponential model against the Poisson handle bit for bit, bit-equality of
the shape sums across K and position, set_shape, linear predictors at the edge
of exp's range and infinite ones, the trajectory against a host velocity
Verlet, No-U-Turn doublings against tests/nuts_oracle.py, whole seeded chains
with a sampled shape against the same driver on the oracle model, prediction
and survival against a long-double oracle and the refusals.  There is no
reference implementation of this family: the oracle is the yardstick
throughout.

Tolerances are measured: the same formulas in NumPy float64
against the long-double oracle on the test's own inputs, relative to the
largest magnitude of the vector compared; the device gets 4 times that error,
because its exp is not the host's, and a measurement below half an ulp counts
as half an ulp.  Every test computes its figure itself, from the oracle alone,
and prints it beside the device's."""
import math
import warnings
from ctypes import byref, c_double, c_int, c_void_p
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sparse

import logit_oracle as lo
import weibull_oracle as wb
from test_hip_poisson import (LAP, VEC_BLOCK, _compare_doublings, _constant,
                              _design_and_matrix)

pytestmark = pytest.mark.gpu

LD = np.longdouble
RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance

U = _constant('GLM_ROW_U', 'glm_rows.hpp')
# one thread, the block edge, one full lap of NPART x VEC_BLOCK, one row past
# it, one row past GLM_ROW_U laps
ROWS = (1, VEC_BLOCK - 1, VEC_BLOCK, VEC_BLOCK + 1, LAP, LAP + 1, U * LAP + 1)
assert ROWS == (1, 255, 256, 257, 65536, 65537, 262145)
SHAPES = (.3, 1., 4.)
EVENT_FRACTIONS = (0., .5, 1.)
KEYS = ('loglik', 'grad', 'hessian', 'shapesum')


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _rel(got, want):
    """max |got - want| / max |want| (in long double)."""
    want = np.asarray(want, dtype=LD)
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(np.asarray(got, dtype=LD) - want)))
    return err / scale if scale > 0 else err


def _bound(measured):
    """The device's tolerance: 4 times the float64 forms' measured error --
    its exp is not the host's -- where a measurement below half an ulp (a
    lucky rounding: no float64 result is promised closer) counts as half an
    ulp."""
    return 4 * max(measured, 2. ** -53)


def _outcome(n, frac, seed):
    """Event indicators with the fraction asked for and times spanning 1e-6
    .. 1e6."""
    rs = np.random.RandomState(seed)
    lt = math.log(10.) * rs.uniform(-6., 6., n)
    if n > 1:
        lt[0], lt[-1] = -6 * math.log(10.), 6 * math.log(10.)
    d = (rs.uniform(size=n) < frac).astype(np.float64)
    return d, lt


def _times(d, lt):
    t = np.exp(lt)
    return np.where(d == 1., t, np.inf), np.where(d == 1., np.inf, t)


def _model(dsn, d, lt, **kw):
    """A device model on exactly these (d, lt): the constructor takes times,
    and log(exp(lt)) need not be lt, so the rows are set after it."""
    from bayesbridge_amd import RegressionModel
    et, ct = _times(d, lt)
    model = RegressionModel((et, ct), dsn, 'weibull', **kw)
    assert model.name == 'weibull' and model.design is dsn
    assert not model._weibull and np.array_equal(model.event, d)
    np.testing.assert_allclose(model.log_time, lt, rtol=1e-14, atol=1e-14)
    model.log_time = lt.copy()
    return model


def _beta(D, n, seed):
    """Coefficients whose linear predictor spans a few units, and a vector."""
    P = D[0].shape[1] + int(D[2])
    rs = np.random.RandomState(seed)
    beta = rs.randn(P) * .3
    beta[0] = -1.
    return beta, rs.randn(P)


def _measure(D, d, lt, beta, v, k):
    """The long-double values of the four quantities at shape k and the error
    of the float64 forms against them."""
    eta_ld = wb.eta_ld(D, beta)
    want = {
        'loglik': np.sum(wb.row_beta_part(eta_ld, d, lt, k, LD)[0]),
        'grad': wb._tdot_ld(D, wb.row_beta_part(eta_ld, d, lt, k, LD)[1]),
        'hessian': wb.hessian_matvec(D, d, lt, beta, v, k, LD),
        'shapesum': np.sum(wb.row_full(eta_ld, d, lt, k, LD))}
    ll, grad = wb.loglik_grad(D, d, lt, beta, k)
    f64 = {'loglik': ll, 'grad': grad,
           'hessian': wb.hessian_matvec(D, d, lt, beta, v, k),
           'shapesum': wb.shape_loglik(D, d, lt, beta, k)}
    return want, {key: _rel(f64[key], want[key]) for key in KEYS}


def _host_design(kind, n):
    """The oracle's design of a case without a device (the measurement)."""
    if kind == 'dense64':
        return lo.design(np.random.RandomState(n).randn(n, 2), True, True)
    from bayesbridge_amd import simulate
    return lo.design(simulate.simulate_binary_csr_fast(n, 40, .2, seed=n),
                     True, True)


# (kind, n, columns): dense f64 with P = 3 at every row count, and one binary
# CSR design in the tiled layout
CASES = [('dense64', n, 2) for n in ROWS] + [('tiled_binary', 2003, 40)]


@lru_cache(maxsize=None)
def _case_reference(case):
    """Per (shape, event fraction) of a case: the outcome, the long-double
    values and the float64 forms' errors; and the largest error per quantity
    over the case's nine cells, which is the figure the device is held to.
    Computed once, from the oracle alone."""
    kind, n, p = CASES[case]
    D = _host_design(kind, n)
    beta, v = _beta(D, n, case)
    cells, worst = {}, dict.fromkeys(KEYS, 0.)
    for frac in EVENT_FRACTIONS:
        d, lt = _outcome(n, frac, 100 * case + int(10 * frac))
        for k in SHAPES:
            want, err64 = _measure(D, d, lt, beta, v, k)
            cells[frac, k] = (want, err64)
            for key in KEYS:
                worst[key] = max(worst[key], err64[key])
    return beta, v, cells, worst


@pytest.mark.parametrize('case', range(len(CASES)))
def test_likelihood_gradient_hessian_and_L_match_the_oracle(case, monkeypatch):
    kind, n, p = CASES[case]
    if n == 1:
        # every column of a single row is "constant", and the design classes
        # drop constant columns as hand-made intercepts: keep them, the row
        # kernel is what this case is about
        from bayesbridge_amd import design_matrix
        monkeypatch.setattr(design_matrix, 'remove_intercept_indicator',
                            lambda X: X)
    dsn, D = _design_and_matrix(kind, n, p, True, True, n)
    H = _host_design(kind, n)
    assert (abs(D[0] - H[0]) > 0).sum() == 0 and np.array_equal(D[1], H[1])
    assert dsn.shape == (n, p + 1)
    beta, v, cells, worst = _case_reference(case)
    print('%s n %d: float64 forms, largest error %s' % (kind, n, worst))
    for frac in EVENT_FRACTIONS:
        d, lt = _outcome(n, frac, 100 * case + int(10 * frac))
        if n > 100:
            assert abs(d.mean() - frac) < .1
            assert lt.min() == -6 * math.log(10.) \
                and lt.max() == 6 * math.log(10.)
        model = _model(dsn, d, lt)
        L = model.shape_loglik(beta, np.array(SHAPES))
        for j, k in enumerate(SHAPES):
            want, err64 = cells[frac, k]
            assert np.isfinite(float(want['shapesum']))
            model.shape = k
            ll, grad = model.compute_loglik_and_gradient(beta)
            hv = model.get_hessian_matvec_operator(beta)(v)
            got = {'loglik': ll, 'grad': grad, 'hessian': hv,
                   'shapesum': L[j]}
            err = {key: _rel(got[key], want[key]) for key in KEYS}
            for key in KEYS:
                print('%-12s n %7d events %.1f k %.1f %-8s float64 %.2e '
                      'device %.2e bound %.2e'
                      % (kind, n, frac, k, key, err64[key], err[key],
                         _bound(worst[key])))
            for key in KEYS:
                assert err[key] <= _bound(worst[key]), (key, frac, k)
            # the same bits on every call; the cached predictor
            ll2, grad2 = model.compute_loglik_and_gradient(beta)
            assert ll2 == ll and np.array_equal(grad2, grad)
            assert np.array_equal(model.get_hessian_matvec_operator(beta)(v),
                                  hv)
            assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
                == (ll, None)
            assert model.hamiltonian_loglik_and_gradient(beta)[0] == ll
            one = model.shape_loglik(None, k)
            assert isinstance(one, float) and one == L[j]
        # the handle's own k and the likelihood at it were not touched
        assert model.shape == SHAPES[-1]
        assert model.compute_loglik_and_gradient(beta)[0] == ll


@pytest.mark.parametrize('kind,n,p', [('dense64', LAP + 1, 2),
                                      ('dense64', VEC_BLOCK + 1, 2),
                                      ('tiled_binary', 2003, 40)])
def test_the_exponential_model_has_the_poisson_handles_bits(kind, n, p):
    """k = 1: k * lt is lt, so w, the gradient, the beta-dependent
    log-likelihood and the Hessian product are those of a bbx_poisson handle
    on the same design with y = d, log_exposure = lt."""
    from bayesbridge_amd import PoissonModel
    dsn, D = _design_and_matrix(kind, n, p, True, True, n)
    d, lt = _outcome(n, .5, 7)
    model = _model(dsn, d, lt, weibull_shape=1.)
    poisson = PoissonModel(d, np.ones(n), dsn)
    poisson.log_exposure = lt.copy()
    rs = np.random.RandomState(8)
    for _ in range(3):
        beta, v = _beta(D, n, rs.randint(1000))
        ll, grad = model.compute_loglik_and_gradient(beta)
        pll, pgrad = poisson.compute_loglik_and_gradient(beta)
        assert np.isfinite(ll) and ll == pll
        assert np.array_equal(grad, pgrad)
        hv = model.get_hessian_matvec_operator(beta)(v)
        assert np.array_equal(hv, poisson.get_hessian_matvec_operator(beta)(v))
    # (w has no accessor of its own: it is read through X~^T w, every
    # column's product and sum w on the intercept column, bit for bit.)  A
    # second shape is not the Poisson handle's
    model.shape = 1. + 2. ** -40
    assert model.compute_loglik_and_gradient(beta)[0] != pll


@pytest.mark.parametrize('kind,n,p', [('tiled_binary', 2003, 40),
                                      ('dense64', U * LAP + 1, 2)])
def test_shape_sums_do_not_depend_on_K_or_position(kind, n, p):
    dsn, D = _design_and_matrix(kind, n, p, True, True, n)
    d, lt = _outcome(n, .5, 3)
    model = _model(dsn, d, lt)
    beta, _ = _beta(D, n, 2)
    kk = np.array([.05, .3, .7, 1., 1.5, 4., 9., 30.])
    L8 = model.shape_loglik(beta, kk)
    assert len(set(L8)) == 8 and np.all(np.isfinite(L8))
    eta_ld = wb.eta_ld(D, beta)
    for j in (1, 3, 5):
        want = np.sum(wb.row_full(eta_ld, d, lt, kk[j], LD))
        f64 = wb.shape_loglik(D, d, lt, beta, kk[j])
        assert _rel(L8[j], want) <= _bound(_rel(f64, want)), kk[j]
    # K = 1 calls, on the cached eta and on a fresh one
    for j in range(8):
        assert model.shape_loglik(None, kk[j]) == L8[j]
        assert model.shape_loglik(beta, kk[j:j + 1])[0] == L8[j]
    # any position, K = 3 and K = 8
    rs = np.random.RandomState(2)
    perm = rs.permutation(8)
    assert np.array_equal(model.shape_loglik(None, kk[perm]), L8[perm])
    for K in (1, 3, 8):
        for start in range(0, 9 - K):
            assert np.array_equal(
                model.shape_loglik(None, kk[start:start + K]),
                L8[start:start + K])
    assert np.array_equal(model.shape_loglik(None, kk[[5, 0, 3]]),
                          L8[[5, 0, 3]])
    # the cached eta is the last beta's
    other = beta * .5
    Lo = model.shape_loglik(other, kk[:3])
    assert np.array_equal(model.shape_loglik(None, kk[:3]), Lo)
    assert not np.array_equal(Lo, L8[:3])
    # K = 9 and a non-positive k are refused with the design still usable
    for bad in (np.ones(9), np.ones((2, 2)), np.array([])):
        with pytest.raises(ValueError):
            model.shape_loglik(None, bad)
    from bayesbridge_amd import _lib
    lib, out = _lib.load(), np.empty(9)
    nine = np.linspace(.5, 2., 9)
    assert lib.bbx_weibull_shape_loglik(model.handle, None, 9, _ptr(nine),
                                        _ptr(out)) == -1
    assert 'n_k outside [1, 8]' in _lib.last_error()
    for bad in (0., -1., np.inf, np.nan):
        with pytest.raises(_lib.BbxError, match=r'k\[1\]'):
            model.shape_loglik(None, np.array([1., bad]))
    assert np.array_equal(model.shape_loglik(None, kk[:3]), Lo)
    assert np.array_equal(model.shape_loglik(beta, kk), L8)
    # a k that overflows one row gives -inf, not NaN, and only for that k:
    # the largest k lt is 13.8 k, past exp's range (709.78) from k = 52 on
    with np.errstate(over='ignore'):
        L = model.shape_loglik(None, np.array([1., 60., 4., 1e3]))
    assert L[1] == -np.inf and L[3] == -np.inf
    assert L[0] == L8[3] and L[2] == L8[5]


def test_set_shape_changes_the_gradient_and_invalidates_the_location():
    from bayesbridge_amd import _lib
    dsn, D = _design_and_matrix('dense64', 300, 9, True, True, 4)
    d, lt = _outcome(300, .5, 4)
    lt = lt / 6.                       # times 0.1 .. 10
    model = _model(dsn, d, lt)
    beta, v = _beta(D, 300, 3)
    assert model.shape == 1.
    _, g1 = model.compute_loglik_and_gradient(beta)
    op = model.get_hessian_matvec_operator(beta)
    op(v)
    model.shape = 2.5
    _, g2 = model.compute_loglik_and_gradient(beta)
    np.testing.assert_allclose(g1, wb.loglik_grad(D, d, lt, beta, 1.)[1],
                               rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(g2, wb.loglik_grad(D, d, lt, beta, 2.5)[1],
                               rtol=RTOL, atol=ATOL)
    assert np.abs(g2 - g1).max() > 1.
    with pytest.raises(RuntimeError, match='location has moved'):
        op(v)
    # the C call itself: BBX_ERR_STATE until the next set_location
    lib, out = _lib.load(), np.empty(10)
    assert lib.bbx_weibull_hessian_matvec(model.handle, _ptr(v), _ptr(out)) \
        == -5
    assert 'set_location' in _lib.last_error()
    np.testing.assert_allclose(
        model.get_hessian_matvec_operator(beta)(v),
        wb.hessian_matvec(D, d, lt, beta, v, 2.5), rtol=RTOL, atol=ATOL)
    # refused while a No-U-Turn tree is open, accepted once its sample is
    # taken
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, d, lt, 2.5)
    joint = logp0 - .5 * np.dot(p0, p0)
    model.nuts_begin(scale, pp, q0, p0, logp0, grad0, joint, joint - 1.)
    with pytest.raises(_lib.BbxError, match='No-U-Turn tree'):
        model.shape = 2.
    assert model.shape == 2.5
    # ... while the shape's log-likelihood may be asked for
    L = model.shape_loglik(beta, 2.)
    np.testing.assert_allclose(L, wb.shape_loglik(D, d, lt, beta, 2.),
                               rtol=RTOL, atol=ATOL)
    model.nuts_sample()
    model.shape = 2.
    assert model.shape == 2.


EXP_MAX = 709.782712893384       # log of the largest double


def test_predictors_at_the_edge_of_exps_range_and_infinite_ones():
    """eta + k lt just below exp's range: finite values that match the
    oracle; just above: the flag is raised, the log-likelihood reads -inf and
    the shape sum is -inf; eta = +-inf.  Arithmetic only: every value is a
    number the kernels compute with."""
    from bayesbridge_amd import HipDenseDesignMatrix
    n = VEC_BLOCK + 1
    rs = np.random.RandomState(5)
    X = rs.randn(n, 2) * .1
    dsn = HipDenseDesignMatrix(X, add_intercept=True, center_predictor=False)
    D = lo.design(X, False, True)
    d = (np.arange(n) % 2).astype(np.float64)
    k = 4.
    lt = rs.uniform(-1., 1., n)
    beta = np.array([.2, .3, -.2])
    eta = lo.dot(D, beta)
    row = 100                                      # a censored row (d = 0)
    for edge, over in ((EXP_MAX - .5, False), (EXP_MAX + .5, True)):
        lt[row] = (edge - eta[row]) / k
        model = _model(dsn, d, lt, weibull_shape=k)
        with np.errstate(over='ignore', invalid='ignore'):
            oll, ograd = wb.loglik_grad(D, d, lt, beta, k)
            oL = wb.shape_loglik(D, d, lt, beta, np.array([1., k]))
        ll, grad = model.compute_loglik_and_gradient(beta)
        L = model.shape_loglik(beta, np.array([1., k]))
        assert np.isfinite(oL[0]) and L[0] == pytest.approx(oL[0], rel=1e-12)
        if over:
            assert oll == -np.inf and oL[1] == -np.inf
            assert (ll, grad) == (-np.inf, None)
            assert L[1] == -np.inf
            raw = model._device_loglik_and_gradient(
                beta, inf_has_no_gradient=False)
            assert raw[0] == -np.inf
        else:
            assert np.isfinite(oll) and oll < -1e307
            # one row carries the sum: exp magnifies the rounding of its
            # argument, 710 eps, by one
            np.testing.assert_allclose(ll, oll, rtol=1e-12)
            np.testing.assert_allclose(grad, ograd, rtol=1e-12)
            np.testing.assert_allclose(L[1], oL[1], rtol=1e-12)
        # the flags were that evaluation's only
        small = beta * .1
        ll_s, grad_s = model.compute_loglik_and_gradient(small)
        with np.errstate(over='ignore', invalid='ignore'):
            o_s = wb.loglik_grad(D, d, lt, small, k)[0]
        if np.isfinite(o_s):
            np.testing.assert_allclose(ll_s, o_s, rtol=1e-12)
    # An infinite intercept.  +inf: every m is inf, the flag is raised and the
    # log-likelihood reads -inf whatever the rows hold, as for the Poisson
    # handle (the formula alone gives a NaN: inf - inf for an event, 0 * inf
    # for a censored row).  -inf: every m is 0, no flag; an event's d eta is
    # -inf, and a censored row's 0 * -inf is a NaN, as the oracle's.
    lt = rs.uniform(-1., 1., n)
    events = _model(dsn, np.ones(n), lt, weibull_shape=k)
    censored = _model(dsn, np.zeros(n), lt, weibull_shape=k)
    up = np.array([np.inf, .3, -.2])
    down = np.array([-np.inf, .3, -.2])
    with np.errstate(all='ignore'):
        assert np.isnan(wb.loglik_grad(D, np.zeros(n), lt, up, k)[0])
        assert np.isnan(wb.loglik_grad(D, np.ones(n), lt, up, k)[0])
        assert wb.loglik_grad(D, np.ones(n), lt, down, k)[0] == -np.inf
        assert np.isnan(wb.loglik_grad(D, np.zeros(n), lt, down, k)[0])
    assert censored.compute_loglik_and_gradient(up) == (-np.inf, None)
    assert events.compute_loglik_and_gradient(up) == (-np.inf, None)
    assert events.compute_loglik_and_gradient(down) == (-np.inf, None)
    assert np.isnan(censored.compute_loglik_and_gradient(down)[0])
    nan = np.array([np.nan, .3, -.2])
    assert np.isnan(events.compute_loglik_and_gradient(nan)[0])
    model = _model(dsn, d, lt, weibull_shape=k)
    ll, grad = model.compute_loglik_and_gradient(beta)
    np.testing.assert_allclose(ll, wb.loglik_grad(D, d, lt, beta, k)[0],
                               rtol=1e-12)
    # a trajectory whose first step overflows: no HIP error, instability at
    # step 1, as for the Poisson handle
    scale, pp = np.ones(3), np.ones(3)
    f = wb.precond_f(D, d, lt, scale, pp, k)
    q0 = beta.copy()
    p0 = np.array([.5, 1., -1.]) * 1e5
    logp0, grad0 = f(q0)
    with np.errstate(all='ignore'):
        want = lo.trajectory(f, 1., 10, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(1., 10, scale, pp, q0, p0, logp0, grad0)
    assert want[5] and want[4] == 1 and want[2] == -np.inf
    assert got['instability'] is True and got['n_steps'] == 1
    assert got['logp'] == -np.inf and got['grad'] is None
    np.testing.assert_allclose(got['q'], want[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['p'], want[1], rtol=RTOL, atol=ATOL)
    assert got['hamiltonian'][1] == np.inf
    ll2, grad2 = model.compute_loglik_and_gradient(beta)
    assert ll2 == ll and np.array_equal(grad2, grad)
    v = rs.randn(3)
    np.testing.assert_allclose(dsn.dot(v), lo.dot(D, v), rtol=RTOL, atol=ATOL)


def _traj_inputs(D, d, lt, k, seed=0):
    """f of the preconditioned coordinates and a start next to the maximum of
    the likelihood (see test_hip_poisson._traj_inputs)."""
    P = D[0].shape[1] + int(D[2])
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    prior_prec = np.ones(P)
    f = wb.precond_f(D, d, lt, scale, prior_prec, k)
    q0 = wb.newton_mle(D, d, lt, k)[0] / scale + rs.randn(P) * .02
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


def _stability_limit(D, d, lt, k, scale, pp, q0):
    """2 / sqrt(largest curvature of -f at q0), by power iteration on the
    oracle's Hessian."""
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * wb.hessian_matvec(D, d, lt, q0 * scale,
                                                scale * v, k)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


def _survival_data(kind, n, p, k, seed=0):
    """A device model on simulated Weibull times (a likelihood with a
    maximum), the oracle's design, d and lt."""
    from bayesbridge_amd import WeibullModel
    dsn, D = _design_and_matrix(kind, n, p, True, True, seed)
    rs = np.random.RandomState(seed + 1)
    truth = np.concatenate(([-.2], rs.randn(p) * .3))
    et, ct = WeibullModel._simulate_from_eta(lo.dot(D, truth), k, .4,
                                             seed + 2)
    d = np.isfinite(et).astype(np.float64)
    lt = np.log(np.minimum(et, ct))
    return _model(dsn, d, lt, weibull_shape=k), D, d, lt


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_trajectory_matches_host_velocity_verlet(kind):
    k = 1.7
    model, D, d, lt = _survival_data(kind, 3 * VEC_BLOCK + 5, 23, k)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, d, lt, k)
    limit = _stability_limit(D, d, lt, k, scale, pp, q0)
    dt = limit / 4
    print('stability limit', limit)
    want = lo.trajectory(f, dt, 25, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(dt, 25, scale, pp, q0, p0, logp0, grad0)
    assert not want[5] and not got['instability']
    assert got['n_steps'] == want[4] == 25
    for key, ref in (('q', want[0]), ('p', want[1]), ('grad', want[3])):
        print(key, np.abs(got[key] - ref).max() / np.abs(ref).max())
        np.testing.assert_allclose(got[key], ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['logp'], want[2], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['hamiltonian'], [want[6], want[7]],
                               rtol=RTOL, atol=ATOL)
    again = model.hmc_trajectory(dt, 25, scale, pp, q0, p0, logp0, grad0)
    for key in ('q', 'p', 'grad', 'hamiltonian'):
        assert np.array_equal(again[key], got[key])
    assert again['logp'] == got['logp']
    # a tolerance on the Hamiltonian's range that a larger step exceeds:
    # both stop at the same step
    want = lo.trajectory(f, dt * 3, 200, q0, p0, logp0, grad0, tol=.5)
    got = model.hmc_trajectory(dt * 3, 200, scale, pp, q0, p0, logp0, grad0,
                               .5)
    print('small tol: steps', got['n_steps'], want[4])
    assert want[5] and 1 <= want[4] < 200 and np.isfinite(want[2])
    assert got['instability'] and got['n_steps'] == want[4]
    np.testing.assert_allclose(got['q'], want[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['p'], want[1], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_nuts_doublings_match_the_oracle(kind):
    k = 1.7
    model, D, d, lt = _survival_data(kind, 3 * VEC_BLOCK + 5, 23, k)
    oracle = wb.OracleModel(D, d, lt, shape=k)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, d, lt, k)
    limit = _stability_limit(D, d, lt, k, scale, pp, q0)
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
    # a tolerance on the Hamiltonian's range that the steps exceed
    outs = _compare_doublings(*args, limit * .75, [1, -1, 1, 1, -1, 1, 1],
                              1e-3, 7)
    assert outs[-1]['instability_detected']


# ------------------------------------------------------------ whole chains
CHAIN_N, CHAIN_P = 300, 12
CHAIN_ITER = {'hmc': 10, 'nuts': 20}
# A chain multiplies a rounding difference from iteration to iteration (see
# test_hip_negbin.py: the step size follows log10 of the Hamiltonian's error).
# The seeds were chosen on the oracle alone, on the CPU (`seed_search` below):
# the oracle's own chain was run again with its likelihood, its gradient and
# L(k) perturbed by 1e-11 relative and compared with itself at this file's
# tolerance, rtol 1e-6 / atol 1e-9, over every saved parameter.  Every seed
# taken is unchanged at 1e-11.  The rule "at most half of the seeds tried are
# left out" is met in none of the four cases -- most chains of this length
# hang on the last bits of a Hamiltonian -- and 'hmc' has no such seed among
# the first 12 at 20 iterations (the best leaves the tolerance by a factor of
# 18 000), so its chains are 10 iterations long; on the dense design none of
# seeds 0 to 47 is unchanged over even 10 and the search went on to 239.
CHAIN_SEED = {('hmc', 'sparse'): 33, ('hmc', 'dense'): 132,
              ('nuts', 'sparse'): 24, ('nuts', 'dense'): 22}
# On the MI355X the four chains deviate from the driver on the oracle by at
# most 1.3e-10 relative ('hmc' dense 1.3e-10, 'hmc' sparse 5.9e-11, 'nuts'
# dense 1.1e-10, 'nuts' sparse 1.4e-11); the test prints the figure.
# (seeds tried, unchanged at 1e-11, the taken seed's largest deviation in
# units of the tolerance at 1e-11)
SEED_SEARCH = {('hmc', 'sparse'): (48, 1, .23),
               ('hmc', 'dense'): (240, 1, .97),
               ('nuts', 'sparse'): (48, 5, .20),
               ('nuts', 'dense'): (48, 2, .46)}


def _chain_problem(fmt):
    from bayesbridge_amd import WeibullModel
    rs = np.random.RandomState(11)
    if fmt == 'sparse':
        X = sparse.random(CHAIN_N, CHAIN_P, density=.3, format='csr',
                          random_state=rs)
        X.data[:] = 1.
    else:
        X = rs.randn(CHAIN_N, CHAIN_P) * .5
    beta = np.zeros(CHAIN_P)
    beta[:4] = (.8, -.6, .4, -.3)
    eta = -.5 + np.asarray(X.dot(beta)).ravel()
    et, ct = WeibullModel._simulate_from_eta(eta, 1.5, .4, 12)
    return X, et, ct


class _HostDesign:
    """What the Gibbs driver reads of a design, for the oracle chain on a
    machine without a GPU (the choice of seeds)."""
    use_hip, is_sparse, intercept_added = True, False, True

    def __init__(self, X):
        self.shape = (X.shape[0], X.shape[1] + 1)
        self.column_offset = np.asarray(X.mean(axis=0)).ravel()


def _chain(fmt, method, seed, oracle=False, n_iter=None, resume=None,
           perturb=0., host=False, **model_args):
    """`n_iter` Gibbs iterations on the device model, or on the oracle model
    behind the same design object.  The chain starts at given coefficients,
    so no mode search runs; the shape starts at its default, 1."""
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, et, ct = _chain_problem(fmt)
    d = np.isfinite(et).astype(np.float64)
    lt = np.log(np.minimum(et, ct))
    n_iter = n_iter or CHAIN_ITER[method]
    if host:
        dsn = _HostDesign(X)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = RegressionModel(
                (et, ct), X, 'weibull',
                **{'weibull_' + key: a for key, a in model_args.items()})
        dsn = model.design
        assert np.array_equal(model.log_time, lt)
    if oracle:
        D = lo.design(X, True, True, offset=dsn.column_offset)
        model = wb.OracleModel(D, d, lt, design=dsn, perturb=perturb,
                               **model_args)
    prior = RegressionCoefPrior(bridge_exponent=.5, sd_for_intercept=2.,
                                regularizing_slab_size=1.)
    start = wb.newton_mle(lo.design(X), d, lt, 1.)[0]
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


CHAIN_KEYS = ('coef', 'global_scale', 'logp', 'local_scale', 'weibull_shape')


def seed_search(method, fmt, n_iter, seeds=range(48), perturbs=(1e-11,)):
    """The choice of seeds, on the CPU alone: the oracle's own chain against
    itself with its likelihood, its gradient and L(k) perturbed by each of
    `perturbs` relative, at this file's tolerance, over every saved parameter.
    Returns {seed: largest deviation in units of the tolerance}."""
    out = {}
    for seed in seeds:
        base, _ = _chain(fmt, method, seed, oracle=True, host=True,
                         n_iter=n_iter)
        worst = 0.
        for perturb in perturbs:
            moved, _ = _chain(fmt, method, seed, oracle=True, host=True,
                              n_iter=n_iter, perturb=perturb)
            worst = max(worst, max(
                float(np.max(np.abs(moved[key] - base[key])
                             / (ATOL + RTOL * np.abs(base[key]))))
                for key in CHAIN_KEYS))
        out[seed] = worst
    return out



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
    assert samples['coef'].shape == (CHAIN_P + 1, n_iter)
    assert samples['weibull_shape'].shape == (n_iter,)
    assert len(set(samples['weibull_shape'])) == n_iter
    assert info['_markov_chain_state']['weibull_shape'] \
        == samples['weibull_shape'][-1]
    si, wsi = (i['_reg_coef_sampling_info'] for i in (info, winfo))
    assert set(si) == set(wsi) == set(HMC_INFO_KEYS if method == 'hmc'
                                      else NUTS_INFO_KEYS)
    worst = max(float(np.max(np.abs(samples[key] - want[key])
                             / (ATOL + RTOL * np.abs(want[key]))))
                for key in CHAIN_KEYS)
    print('shape', samples['weibull_shape'][[0, -1]], 'n_grad_evals',
          si['n_grad_evals'], 'largest deviation %.3g of the tolerance (rtol '
          '%.0e): %.3g relative' % (worst, RTOL, worst * RTOL))
    for key in CHAIN_KEYS:
        np.testing.assert_allclose(samples[key], want[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)
    for key in si:
        np.testing.assert_allclose(si[key], wsi[key], rtol=RTOL, atol=ATOL,
                                   err_msg=key)
    assert np.all(si['n_grad_evals'] > 1)
    # two halves through gibbs_resume against the straight run
    half = n_iter // 2
    resumed, rinfo = _chain(fmt, method, seed, n_iter=half,
                            resume=n_iter - half)
    assert rinfo['n_iter'] == n_iter
    for key in samples:
        np.testing.assert_allclose(resumed[key], samples[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)
    for key in si:
        np.testing.assert_allclose(rinfo['_reg_coef_sampling_info'][key],
                                   si[key], rtol=RTOL, atol=ATOL, err_msg=key)


def test_fixed_shape_chain_draws_no_uniforms_for_it(monkeypatch):
    """weibull_shape=1.5: samples['weibull_shape'] is constant, the slice
    update never runs, and the chain matches the driver on the oracle with
    the same fixed value."""
    from bayesbridge_amd import bayesbridge
    seed = CHAIN_SEED['nuts', 'dense']
    fixed, info = _chain('dense', 'nuts', seed, n_iter=8, shape=1.5)
    want, _ = _chain('dense', 'nuts', seed, n_iter=8, oracle=True, shape=1.5)
    assert np.all(fixed['weibull_shape'] == 1.5)
    assert info['_markov_chain_state']['weibull_shape'] == 1.5
    for key in CHAIN_KEYS:
        np.testing.assert_allclose(fixed[key], want[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)

    def never(*args, **kw):
        raise AssertionError("the shape is fixed")

    monkeypatch.setattr(bayesbridge, 'update_shape', never)
    again, _ = _chain('dense', 'nuts', seed, n_iter=8, shape=1.5)
    for key in CHAIN_KEYS:
        assert np.array_equal(again[key], fixed[key]), key


def test_default_sampler_mode_search_and_initial_shape():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, et, ct = _chain_problem('dense')
    model = RegressionModel((et, ct), X, 'weibull',
                            weibull_shape_prior={'shape': 3., 'rate': 2.})
    assert model.intercept_added            # added by default, unlike Cox
    assert model.n_obs == CHAIN_N           # the rows stay in their order
    prior = RegressionCoefPrior(bridge_exponent=.5, sd_for_intercept=2.,
                                regularizing_slab_size=1.)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        samples, info = BayesBridge(model, prior).gibbs(
            3, init={'global_scale': .1, 'weibull_shape': 1.4}, seed=1,
            params_to_save=('coef', 'weibull_shape'))
    assert info['coef_sampler_type'] == 'hmc'
    assert info['options']['rng'] == 'reference'
    assert info['_init_optim_info']['is_success']
    assert info['init']['weibull_shape'] == 1.4
    assert set(samples) == {'coef', 'weibull_shape'}
    assert np.all(np.isfinite(samples['coef']))
    assert np.all(samples['weibull_shape'] > 0)
    assert model.shape == samples['weibull_shape'][-1]
    # the search went uphill from its start, at the initial shape
    D = lo.design(X, True, True, offset=model.design.column_offset)
    start = np.zeros(CHAIN_P + 1)
    model.shape = 1.4
    start[0] = model.calc_intercept_mle()
    assert wb.loglik_grad(D, model.event, model.log_time,
                          info['init']['coef'], 1.4)[0] > \
        wb.loglik_grad(D, model.event, model.log_time, start, 1.4)[0]


def test_refusals_are_exceptions():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior, SamplerOptions
    model, D, d, lt = _survival_data('dense64', 100, 20, 1.5)
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
        model.compute_loglik_and_gradient(np.zeros(20))


# ------------------------------------------------------------- prediction
PREDICT_KEYS = ('mean', 'sd', 'lpd', 'loglik_mean', 'loglik_var')
N_DRAW = 7


@lru_cache(maxsize=None)
def _predict_case(n):
    """Rows, times, 7 draws of the coefficients and of the shape; the
    long-double results by their definitions and the errors of the float64
    recurrence (the prediction) and of the float64 two-pass form (the
    survival) against them.  Computed once per n, from the oracle alone."""
    from bayesbridge_amd import WeibullModel
    rs = np.random.RandomState(31 + n)
    X = rs.randn(n, 2) * .5
    truth = np.array([-.4, .5, -.3])
    D = lo.design(X, True, True)
    et, ct = WeibullModel._simulate_from_eta(lo.dot(D, truth), 1.5, .4, n)
    coef = truth[:, None] + rs.randn(3, N_DRAW) * .05
    shape = np.exp(math.log(1.5) + rs.randn(N_DRAW) * .1)
    times = np.array([.05, .5, 1., 2.5, 40.])
    d = np.isfinite(et).astype(np.float64)
    lt = np.log(np.minimum(et, ct))
    eta_ld = np.stack([wb.eta_ld(D, coef[:, s]) for s in range(N_DRAW)],
                      axis=1)
    eta64 = np.stack([lo.dot(D, coef[:, s]) for s in range(N_DRAW)], axis=1)
    want = wb.predict_explicit(eta_ld, shape, d, lt)
    rec = wb.predict_recurrence(eta64, shape, d, lt)
    measured = {key: _rel(rec[key], want[key])
                for key in PREDICT_KEYS + ('mu',)}
    surv = wb.survival(eta_ld, shape, times)
    surv64 = wb.survival(eta64, shape, times, np.float64)
    smeasured = {key: _rel(surv64[key], surv[key])
                 for key in ('mean', 'sd', 'draws')}
    return (X, et, ct, coef, shape, times, want, measured, surv, smeasured)


@pytest.mark.parametrize('n', [VEC_BLOCK + 1, LAP + 1])
def test_predict_and_survival_match_the_long_double_oracle(n):
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    X, et, ct, coef, shape, times, want, measured, surv, smeasured = \
        _predict_case(n)
    dsn = HipDenseDesignMatrix(X, add_intercept=True, center_predictor=True)
    model = RegressionModel((et, ct), dsn, 'weibull')
    got = model.predict(coef, shape, return_draws=True)
    for key in PREDICT_KEYS:
        print('n %6d %-11s oracle f64 vs ext %.2e   device vs ext %.2e   '
              'bound %.2e' % (n, key, measured[key],
                              _rel(got[key], want[key]),
                              _bound(measured[key])))
    for key in PREDICT_KEYS:
        assert got[key].shape == (n,)
        assert _rel(got[key], want[key]) <= _bound(measured[key]), key
    assert got['draws'].shape == (n, N_DRAW)
    assert _rel(got['draws'], want['mu']) <= _bound(measured['mu'])
    lppd = float(np.sum(want['lpd']))
    p_waic = float(np.sum(want['loglik_var']))
    for key, value in (('lppd', lppd), ('p_waic', p_waic),
                       ('waic', -2. * (lppd - p_waic))):
        np.testing.assert_allclose(got[key], value, rtol=1e-12)
    # no result depends on the draws per pass
    for per in (0, 1, 3):
        other = model.predict(coef, shape, return_draws=True,
                              _draws_per_pass=per)
        assert set(other) == set(got)
        for key in got:
            assert np.array_equal(other[key], got[key]), (per, key)
    # a scalar shape is that value for every draw; new rows without an
    # outcome give the medians only, with one the training rows' scores
    one = model.predict(coef, 1.5)
    same = model.predict(coef, np.full(N_DRAW, 1.5))
    for key in one:
        assert np.array_equal(one[key], same[key]), key
    for per in (0, 1, 3):
        new = model.predict(coef, shape, X_new=X, _draws_per_pass=per)
        assert set(new) == {'mean', 'sd'}
        assert np.array_equal(new['mean'], got['mean'])
        assert np.array_equal(new['sd'], got['sd'])
        scored = model.predict(coef, shape, X_new=X, event_time_new=et,
                               censoring_time_new=ct, _draws_per_pass=per)
        for key in PREDICT_KEYS + ('lppd', 'p_waic', 'waic'):
            assert np.array_equal(scored[key], got[key]), key
    for bad in (np.ones(3), -1., np.inf, np.full(N_DRAW, np.nan)):
        with pytest.raises(ValueError):
            model.predict(coef, bad)
    with pytest.raises(ValueError, match='at least 2 draws'):
        model.predict(coef[:, 0], 1.5)
    assert set(model.predict(coef[:, 0], 1.5, X_new=X[:5])) == {'mean', 'sd'}
    # survival: training rows and new rows, any time
    s_train = model.predict_survival(coef, shape, times=times,
                                     return_draws=True)
    for key in ('mean', 'sd'):
        print('n %6d survival %-4s oracle f64 vs ext %.2e   device vs ext '
              '%.2e   bound %.2e' % (n, key, smeasured[key],
                                     _rel(s_train[key], surv[key]),
                                     _bound(smeasured[key])))
    assert np.array_equal(s_train['time'], times)
    for key in ('mean', 'sd'):
        assert s_train[key].shape == (n, len(times))
        assert _rel(s_train[key], surv[key]) <= _bound(smeasured[key]), key
    assert s_train['draws'].shape == (n, len(times), N_DRAW)
    assert _rel(s_train['draws'], surv['draws']) \
        <= _bound(smeasured['draws'])
    s_new = model.predict_survival(coef, shape, X_new=X, times=times)
    assert set(s_new) == {'time', 'mean', 'sd'}
    for key in ('mean', 'sd'):
        assert np.array_equal(s_new[key], s_train[key]), key
    # S decreases in t and lies in [0, 1]; the default grid is the training
    # rows' distinct event times
    assert np.all(np.diff(s_train['mean'], axis=1) < 0)
    assert s_train['mean'].min() >= 0 and s_train['mean'].max() <= 1
    if n < 1000:
        default = model.predict_survival(coef, shape, X_new=X[:3])
        assert np.array_equal(default['time'], np.unique(et[np.isfinite(et)]))
        assert default['mean'].shape == (3, len(default['time']))
    # S at the posterior draws' own median is one half, draw by draw
    half = model.predict_survival(coef[:, :1], shape[:1], X_new=X[:1],
                                  times=[float(got['draws'][0, 0])])
    assert half['mean'][0, 0] == pytest.approx(.5, rel=1e-12)


def test_the_shared_summary_still_refuses_family_4():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    design = HipDenseDesignMatrix(rs.randn(40, 3))
    coef, d = rs.randn(2, 4) * .1, np.ones(40)
    lt = rs.randn(40)
    out = [np.empty(40) for _ in range(5)]
    st = lib.bbx_design_predictive_summary(
        design.handle, 4, 2, _ptr(coef), None, None, _ptr(d), None, None, 0,
        *[_ptr(a) for a in out], None)
    assert st == -1 and 'family 4' in _lib.last_error()
    # the family's own call refuses what it must, with the design usable
    entry = lib.bbx_design_predictive_summary_weibull
    k = np.array([1., 2.])
    for bad_k in (None, np.array([1., 0.]), np.array([1., np.inf])):
        assert entry(design.handle, 2, _ptr(coef), _ptr(bad_k), _ptr(d),
                     _ptr(lt), None, 0, *[_ptr(a) for a in out], None) == -1
        assert 'shape' in _lib.last_error()
    # NULL arrays
    assert entry(design.handle, 2, None, _ptr(k), _ptr(d), _ptr(lt), None, 0,
                 *[_ptr(a) for a in out], None) == -1
    assert 'coef is NULL' in _lib.last_error()
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), _ptr(d), _ptr(lt),
                 None, 0, None, _ptr(out[1]), *[_ptr(a) for a in out[2:]],
                 None) == -1
    assert 'mean is NULL' in _lib.last_error()
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), _ptr(d), _ptr(lt),
                 None, 0, _ptr(out[0]), None, *[_ptr(a) for a in out[2:]],
                 None) == -1
    assert 'sd is NULL' in _lib.last_error()
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), _ptr(d), None, None,
                 0, *[_ptr(a) for a in out], None) == -1
    assert 'together' in _lib.last_error()
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), None, _ptr(lt), None,
                 0, *[_ptr(a) for a in out], None) == -1
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), _ptr(d), _ptr(lt),
                 None, 0, _ptr(out[0]), _ptr(out[1]), None, None, None,
                 None) == -1
    # fewer than 2 draws when scoring; one draw without an outcome is served
    assert entry(design.handle, 1, _ptr(coef), _ptr(k), _ptr(d), _ptr(lt),
                 None, 0, *[_ptr(a) for a in out], None) == -1
    assert 'at least 2 draws' in _lib.last_error()
    assert entry(design.handle, 1, _ptr(coef), _ptr(k), None, None, None, 0,
                 _ptr(out[0]), _ptr(out[1]), None, None, None, None) == 0
    bad_d = np.where(np.arange(40) == 7, 2., d)
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), _ptr(bad_d), _ptr(lt),
                 None, 0, *[_ptr(a) for a in out], None) == -1
    assert 'event[7]' in _lib.last_error()
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), _ptr(d), _ptr(lt),
                 None, -1, *[_ptr(a) for a in out], None) == -1
    assert entry(design.handle, 2, _ptr(coef), _ptr(k), _ptr(d), _ptr(lt),
                 None, 0, *[_ptr(a) for a in out], None) == 0
    assert np.all(np.isfinite(out[2])) and np.all(out[0] > 0)


def test_c_abi_errors_are_status_codes():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    n, p = 50, 4
    design = HipDenseDesignMatrix(rs.randn(n, p))
    P = p + 1
    d, lt = (np.arange(n) % 2).astype(np.float64), rs.randn(n)
    vec, out = rs.randn(P) * .1, np.empty(P)
    ll, cnt = c_double(), c_int()
    null = c_void_p()
    assert lib.bbx_weibull_loglik_grad(null, _ptr(vec), byref(ll), None) < 0
    assert lib.bbx_weibull_set_location(null, _ptr(vec)) < 0
    assert lib.bbx_weibull_set_shape(null, 1.) < 0
    assert lib.bbx_weibull_destroy(null) == 0
    # bad arguments at create
    h = c_void_p()
    assert lib.bbx_weibull_create(design.handle, _ptr(d), _ptr(lt), 1.,
                                  None) < 0
    assert lib.bbx_weibull_create(null, _ptr(d), _ptr(lt), 1., byref(h)) < 0
    assert lib.bbx_weibull_create(design.handle, None, _ptr(lt), 1.,
                                  byref(h)) == -1
    assert 'NULL event' in _lib.last_error()
    assert lib.bbx_weibull_create(design.handle, _ptr(d), None, 1.,
                                  byref(h)) == -1
    assert 'NULL log_time' in _lib.last_error()
    at = np.arange(n)
    for bad_d, bad_lt, bad_k, text in (
            (np.where(at == 7, -1., d), lt, 1., 'event[7]'),
            (np.where(at == 7, .5, d), lt, 1., 'event[7]'),
            (np.where(at == 7, 2., d), lt, 1., 'event[7]'),
            (np.where(at == 7, np.nan, d), lt, 1., 'event[7]'),
            (d, np.where(at == 9, np.inf, lt), 1., 'log_time[9]'),
            (d, np.where(at == 9, -np.inf, lt), 1., 'log_time[9]'),
            (d, np.where(at == 9, np.nan, lt), 1., 'log_time[9]'),
            (d, lt, 0., 'shape'), (d, lt, -1., 'shape'),
            (d, lt, np.inf, 'shape'), (d, lt, np.nan, 'shape')):
        bad_d = np.ascontiguousarray(bad_d)
        bad_lt = np.ascontiguousarray(bad_lt)
        assert lib.bbx_weibull_create(design.handle, _ptr(bad_d),
                                      _ptr(bad_lt), bad_k, byref(h)) == -1
        assert not h.value
        assert text in _lib.last_error()
    assert lib.bbx_weibull_create(design.handle, _ptr(d), _ptr(lt), 2.,
                                  byref(h)) == 0
    # order of calls
    assert lib.bbx_weibull_hessian_matvec(h, _ptr(vec), _ptr(out)) == -5
    assert 'set_location' in _lib.last_error()
    u = rs.rand(1)
    assert lib.bbx_weibull_nuts_doubling(h, .1, 1, 0, _ptr(u), byref(cnt),
                                         byref(cnt), None, None, None) < 0
    assert 'nuts_begin' in _lib.last_error()
    kk, L = np.array([1., 2., 4.]), np.empty(8)
    assert lib.bbx_weibull_shape_loglik(h, None, 3, _ptr(kk), _ptr(L)) == -5
    assert 'cached' in _lib.last_error()
    for n_k in (0, 9, -1):
        assert lib.bbx_weibull_shape_loglik(h, _ptr(vec), n_k, _ptr(kk),
                                            _ptr(L)) == -1
    for bad in (0., -1., np.inf, np.nan):
        bad_kk = np.array([1., bad, 4.])
        assert lib.bbx_weibull_shape_loglik(h, _ptr(vec), 3, _ptr(bad_kk),
                                            _ptr(L)) == -1
        assert 'k[1]' in _lib.last_error()
        assert lib.bbx_weibull_set_shape(h, bad) == -1
    assert lib.bbx_weibull_shape_loglik(h, _ptr(vec), 3, None, _ptr(L)) == -1
    # a refused call with beta cached nothing
    assert lib.bbx_weibull_shape_loglik(h, None, 3, _ptr(kk), _ptr(L)) == -5
    assert lib.bbx_weibull_shape_loglik(h, _ptr(vec), 3, _ptr(kk),
                                        _ptr(L)) == 0
    assert lib.bbx_weibull_shape_loglik(h, None, 3, _ptr(kk), _ptr(L)) == 0
    assert np.all(np.isfinite(L[:3]))
    # the design and the handle work afterwards
    ll0 = c_double()
    assert lib.bbx_weibull_loglik_grad(h, _ptr(vec), byref(ll), _ptr(out)) == 0
    assert np.isfinite(ll.value)
    assert lib.bbx_weibull_set_shape(h, 5.) == 0
    assert lib.bbx_weibull_loglik_grad(h, _ptr(vec), byref(ll0), None) == 0
    assert ll0.value != ll.value
    # use after the design is destroyed
    design.__del__()
    assert lib.bbx_weibull_loglik_grad(h, _ptr(vec), byref(ll), None) < 0
    assert 'destroyed' in _lib.last_error()
    assert lib.bbx_weibull_set_shape(h, 1.) < 0
    assert lib.bbx_weibull_destroy(h) == 0
