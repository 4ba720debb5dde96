"""GPU: case weights in the Cox model (csrc/cox_weighted.hip on
csrc/hamiltonian.hpp) -- the likelihood, its gradient and Hessian matvec
against the NumPy oracle (tests/cox_weighted_oracle.py) on three design types,
at the partition edges of the scans and at one multi-tile size; against the
plain CoxModel with unit weights and, with integer weights, on the replicated
rows; the exact scaling under doubled weights; weights spanning twelve orders
of magnitude and the empty risk-set rule; determinism and the launch count;
the trajectory, No-U-Turn doublings and whole seeded chains against the same
host logic on the oracle; the refusals of the create call.  There is no
reference implementation of this likelihood: the oracle's extended-precision
form is the yardstick, and each comparison first checks on the CPU that the
oracle's own float64 scan form meets the tolerance it holds the device to."""
import math
import warnings
from ctypes import byref, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_cases as cc
import cox_weighted_oracle as cwo
import ham_cabi as hc
import logit_oracle as lo
from test_hip_cox_efron import _betas, _design, _launches, _within

pytestmark = pytest.mark.gpu

# tests/test_hip_cox.py's, for the same quantities against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10
RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance
VALUES = {'dense64': 'normal', 'tiled_binary': 'binary',
          'csr_valued': 'valued'}


def _models(kind, event, cens, X, weights, plain=False):
    """(the weighted model on rows already in order, the oracle's X, idx[, the
    plain model on the same design])."""
    from bayesbridge_amd import RegressionModel
    design, X = _design(kind, X)
    model = RegressionModel((event, cens), design, 'cox', weights=weights)
    assert model.name == 'cox' and model._ham_prefix == 'bbx_coxw_'
    assert model.n_pred == X.shape[1]
    assert np.array_equal(model.weights, weights)
    idx = (model.n_event, model.risk_set_start_index,
           model.risk_set_end_index, model.n_appearance_in_risk_set,
           model.weights)
    if plain:
        other = RegressionModel((event, cens), design, 'cox')
        assert other._ham_prefix == 'bbx_cox_' and other.weights is None
        return model, X, idx, other
    return model, X, idx


def _oracle_ext(X, beta, v, idx, event, cens):
    if X.shape[0] <= cwo.EXPLICIT_MAX_N:
        a = idx[4]
        oll, ograd = cwo.explicit_loglik_grad(X, beta, event, cens, a)
        return oll, ograd, cwo.explicit_hessian_matvec(X, beta, v, event,
                                                       cens, a)
    oll, ograd = cwo.scans_loglik_grad(X, beta, idx, np.longdouble)
    return oll, ograd, cwo.scans_hessian_matvec(X, beta, v, idx,
                                                np.longdouble)


def _rel(got, want):
    return np.abs(np.asarray(got) - want).max() / (np.abs(want).max() or 1.)


def _check_against_oracle(model, X, idx, event, cens, betas, vs):
    """Device == oracle at the tolerances, after the CPU check that the
    oracle's float64 scan form is within them of its extended-precision form
    (the explicit risk-set matrix up to 2049 rows, scans beyond); two calls
    give the same bits."""
    for beta, v in zip(betas, vs):
        oll, ograd, ohv = _oracle_ext(X, beta, v, idx, event, cens)
        assert np.isfinite(oll)
        fll, fgrad = cwo.scans_loglik_grad(X, beta, idx)
        fhv = cwo.scans_hessian_matvec(X, beta, v, idx)
        print('n', X.shape[0], 'oracle f64 vs ext: ll %.2e grad %.2e hess %.2e'
              % (_rel(fll, oll), _rel(fgrad, ograd), _rel(fhv, ohv)))
        assert abs(fll - oll) <= LL_TOL * abs(oll)
        assert _within(fgrad, ograd, GRAD_TOL)
        assert _within(fhv, ohv, HESS_TOL)
        ll, grad = model.compute_loglik_and_gradient(beta)
        hv = model.get_hessian_matvec_operator(beta)(v)
        print('   device vs ext: ll %.2e grad %.2e hess %.2e'
              % (_rel(ll, oll), _rel(grad, ograd), _rel(hv, ohv)))
        assert abs(ll - oll) <= LL_TOL * abs(oll)
        assert _within(grad, ograd, GRAD_TOL)
        assert _within(hv, ohv, HESS_TOL)
        ll2, grad2 = model.compute_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        assert np.array_equal(model.get_hessian_matvec_operator(beta)(v), hv)
        assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
            == (ll, None)
        assert model.hamiltonian_loglik_and_gradient(beta)[0] == ll


def _grid_problem(kind, n, p, seed, n_grid=200, weights='lognormal',
                  plain=False):
    """Sorted rows with times on a grid (events tie, censoring times tie event
    times; no row is censored before the first event, so n rows stay) and
    their weights."""
    from bayesbridge_amd.model import cox_preprocess
    rs = np.random.RandomState(seed)
    X = cc._design(n, p, VALUES[kind], rs, .2 if p <= 20 else .1)
    a = np.exp(rs.randn(n)) if weights == 'lognormal' else weights(rs, n)
    dense = X if kind.startswith('dense') else np.asarray(X.todense())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, X, keep = cox_preprocess(
            *cwo.make_times(dense, seed, n_grid=n_grid), X)
    assert len(keep) == n
    return (event, cens) + _models(kind, event, cens, X, a[keep], plain)


@pytest.mark.parametrize('kind', ['tiled_binary', 'csr_valued', 'dense64'])
def test_likelihood_gradient_hessian_match_the_oracle(kind):
    """2049 rows x 40 columns, weights lognormal(0, 1), times on a 200-point
    grid: tied events, censoring times tied to event times."""
    event, cens, model, X, idx = _grid_problem(kind, 2049, 40, 3)
    assert model.n_obs == 2049 and idx[4].max() / idx[4].min() > 100
    assert np.any(idx[1] != np.arange(idx[0]))
    assert np.intersect1d(event, cens).size
    _check_against_oracle(model, X, idx, event, cens, *_betas(40))


SUBSET = [(1, 0), (2, 0), (2, 1), (1, 2049), (255, 2049), (256, 0), (257, 1),
          (2047, 0), (2048, 1), (2049, 2049)]


@pytest.mark.parametrize('ne,n_cens', SUBSET)
def test_partition_edges(ne, n_cens):
    """SCAN_G = 256 chunks per segment, tiles of 2048: segment lengths at the
    edges, cox_cases' ties across every chunk and tile boundary, weights
    uniform on [0.2, 5].  One event alone with weight 1: every result is
    exactly 0, as the plain model's.  With a weight a it is not: H = a, so
    loglik = -a log a, and w = a - (a (1/a)) a is 0 only up to the rounding
    of 1/a -- the gradient and the Hessian matvec are held to the tolerances
    times the size a |x| (times |u|) of the two terms that cancel."""
    case = cc.cox_case(ne, n_cens, p=3, seed=ne + 7 * n_cens)
    a = np.random.RandomState(ne + n_cens).uniform(.2, 5., ne + n_cens)
    model, X, idx = _models('dense64', case.event_time, case.censoring_time,
                            case.X, a)
    assert model.n_obs == ne + n_cens and model.n_event == ne
    if (ne, n_cens) == (1, 0):
        beta = np.array([.3, -.2, .1])
        unit = _models('dense64', case.event_time, case.censoring_time,
                       case.X, np.ones(1))[0]
        assert unit.compute_loglik_and_gradient(beta)[0] == 0.
        assert not unit.compute_loglik_and_gradient(beta)[1].any()
        assert not unit.get_hessian_matvec_operator(beta)(beta).any()
        assert a[0] != 1.
        ll, grad, hv = _all_three(model, beta, beta)
        want = -a[0] * math.log(a[0])
        assert cwo.explicit_loglik(X, beta, case.event_time,
                                   case.censoring_time, a) \
            == pytest.approx(want, rel=1e-15)
        print('one event: ll', ll, 'want', want, 'grad', grad, 'hess', hv)
        assert abs(ll - want) <= LL_TOL * abs(want)
        size = a[0] * np.abs(X).max()
        assert np.abs(grad).max() <= GRAD_TOL * size
        assert np.abs(hv).max() <= HESS_TOL * size * abs((X @ beta)[0])
        return
    _check_against_oracle(model, X, idx, case.event_time,
                          case.censoring_time, *_betas(3))


def test_multi_tile_chunks():
    """524 289 events + 1 censored row: each of the 256 chunks holds 2049
    elements, one more than a tile."""
    ne, p = 524289, 4
    case = cc.cox_case(ne, 1, p=p, seed=5)
    a = np.exp(np.random.RandomState(5).randn(ne + 1))
    model, X, idx = _models('dense64', case.event_time, case.censoring_time,
                            case.X, a)
    assert cc.chunk_len(ne) == cc.SCAN_TILE + 1
    betas, vs = _betas(p, scales=(.5,))
    _check_against_oracle(model, X, idx, case.event_time,
                          case.censoring_time, betas, vs)


def _all_three(model, beta, v):
    ll, grad = model.compute_loglik_and_gradient(beta)
    return ll, grad, model.get_hessian_matvec_operator(beta)(v)


def test_unit_weights_are_the_plain_model():
    """Weights all 1 on the plain model's design: its values at the
    tolerances.  Non-unit weights: farther than 100 tolerances from them, so
    these tests can see the feature."""
    case = cc.cox_case(1500, 1500, p=12, seed=6)
    beta, v = _betas(12, scales=(.5,))
    beta, v = beta[0], v[0]
    rs = np.random.RandomState(6)
    for a, unit in ((np.ones(3000), True), (np.exp(rs.randn(3000)), False)):
        model, X, idx, plain = _models('dense64', case.event_time,
                                       case.censoring_time, case.X, a, True)
        got, want = _all_three(model, beta, v), _all_three(plain, beta, v)
        d = (abs(got[0] - want[0]) / abs(want[0]), _rel(got[1], want[1]),
             _rel(got[2], want[2]))
        print('unit' if unit else 'lognormal',
              'vs plain: ll %.2e grad %.2e hess %.2e' % d,
              'bit-equal' if d == (0., 0., 0.) else '')
        if unit:
            assert d[0] <= LL_TOL and d[1] <= GRAD_TOL and d[2] <= HESS_TOL
        else:
            assert d[0] > 100 * LL_TOL and d[1] > 100 * GRAD_TOL
            assert d[2] > 100 * HESS_TOL
        _check_against_oracle(model, X, idx, case.event_time,
                              case.censoring_time, [beta], [v])


def test_integer_weights_are_replicated_rows():
    """Weights in {1, 2, 3} on 1500 + 1500 rows against the plain handle on
    the design with row i written a_i times."""
    from bayesbridge_amd import RegressionModel
    case = cc.cox_case(1500, 1500, p=12, seed=7)
    a = np.random.RandomState(7).randint(1, 4, 3000).astype(np.float64)
    assert set(a) == {1., 2., 3.}
    model, X, idx = _models('dense64', case.event_time, case.censoring_time,
                            case.X, a)
    revent, rcens, rX = cwo.replicate(case.event_time, case.censoring_time,
                                      case.X, a)
    plain = RegressionModel((revent, rcens), _design('dense64', rX)[0], 'cox')
    assert plain.n_obs == int(a.sum()) and plain._ham_prefix == 'bbx_cox_'
    assert plain.n_event == int(a[:1500].sum())
    betas, vs = _betas(12)
    for beta, v in zip(betas, vs):
        got, want = _all_three(model, beta, v), _all_three(plain, beta, v)
        print('vs replicated: ll %.2e grad %.2e hess %.2e'
              % (abs(got[0] - want[0]) / abs(want[0]), _rel(got[1], want[1]),
                 _rel(got[2], want[2])))
        assert abs(got[0] - want[0]) <= LL_TOL * abs(want[0])
        assert _within(got[1], want[1], GRAD_TOL)
        assert _within(got[2], want[2], HESS_TOL)
    _check_against_oracle(model, X, idx, case.event_time,
                          case.censoring_time, betas, vs)


@pytest.mark.parametrize('kind', ['dense64', 'tiled_binary'])
def test_doubled_weights_double_every_bit(kind):
    """Every intermediate scales by a power of two: gradient and Hessian
    matvec are bit for bit twice the original; the log-likelihood is
    2 loglik - log 2 . sum_k 2 a_k."""
    event, cens, model, X, idx = _grid_problem(kind, 2049, 20, 11)
    a = idx[4]
    twice = _models(kind, event, cens, X, 2. * a)[0]
    four = _models(kind, event, cens, X, 4. * a)[0]
    for beta, v in zip(*_betas(20)):
        ll, grad, hv = _all_three(model, beta, v)
        ll2, grad2, hv2 = _all_three(twice, beta, v)
        ll4, grad4, hv4 = _all_three(four, beta, v)
        assert np.any(grad != 0) and np.any(hv != 0)
        assert np.array_equal(grad2, 2. * grad) and np.array_equal(hv2, 2. * hv)
        assert np.array_equal(grad4, 4. * grad) and np.array_equal(hv4, 4. * hv)
        want = 2. * ll - math.log(2.) * np.sum(2. * a[:idx[0]])
        print('doubled: ll %.17g want %.17g' % (ll2, want))
        assert abs(ll2 - want) <= LL_TOL * abs(want)
        want = 4. * ll - math.log(4.) * np.sum(4. * a[:idx[0]])
        assert abs(ll4 - want) <= LL_TOL * abs(want)


def test_weights_over_twelve_orders_of_magnitude():
    def wide(rs, n):
        a = 10. ** rs.uniform(-6., 6., n)
        a[:2] = 1e-6, 1e6
        return a
    event, cens, model, X, idx = _grid_problem('dense64', 2049, 20, 12,
                                               weights=wide)
    assert idx[4].min() == 1e-6 and idx[4].max() == 1e6
    betas, vs = _betas(20)
    for beta, v in zip(betas, vs):
        ll, grad, hv = _all_three(model, beta, v)
        assert np.isfinite(ll) and np.all(np.isfinite(grad))
        assert np.all(np.isfinite(hv))
    _check_against_oracle(model, X, idx, event, cens, betas, vs)


def test_underflowing_risk_set_gives_minus_infinity():
    """Where every weighted hazard at risk underflows the handle reports what
    the plain model reports."""
    event, cens, model, X, idx = _grid_problem('dense64', 2000, 20, 9,
                                               n_grid=50)
    beta = np.zeros(20)
    beta[0] = 2000.       # exp(eta - max) underflows for most rows
    assert cwo.scans_loglik_grad(X, beta, idx) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
        == (-np.inf, None)
    from bayesbridge_amd import _lib
    b = np.ascontiguousarray(beta)
    assert _lib.load().bbx_coxw_set_location(
        model.handle, b.ctypes.data_as(c_void_p)) == _lib.ERR_NUMERIC
    with pytest.raises(ValueError, match='Hessian operator'):
        model.get_hessian_matvec_operator(beta)
    # the flags were that evaluation's only
    ll = model.compute_loglik_and_gradient(beta * 0)[0]
    assert abs(ll - cwo.scans_loglik_grad(X, beta * 0, idx)[0]) \
        <= LL_TOL * abs(ll)
    # a trajectory whose first step lands there reports instability
    P = 20
    scale, pp = np.ones(P), np.ones(P)
    f = cwo.precond_f(X, scale, pp, idx)
    q0, p0 = np.zeros(P), beta.copy()
    logp0, grad0 = f(q0)
    want = lo.trajectory(f, 1., 10, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(1., 10, scale, pp, q0, p0, logp0, grad0)
    assert want[5] and want[4] == 1 and want[2] == -np.inf
    assert got['instability'] is True and got['n_steps'] == 1
    assert got['logp'] == -np.inf and got['grad'] is None


def test_launch_count_is_the_plain_handles():
    case = cc.cox_case(900, 400, p=6, seed=8)
    a = np.random.RandomState(8).uniform(.2, 5., 1300)
    model, X, idx, plain = _models('dense64', case.event_time,
                                   case.censoring_time, case.X, a, True)
    counts = _launches(model, case.beta), _launches(plain, case.beta)
    print('launches (weighted, plain): %s' % (counts,))
    assert counts[0] == counts[1] > 6


def _traj_inputs(X, idx, seed=0):
    P = X.shape[1]
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    prior_prec = np.ones(P)
    f = cwo.precond_f(X, scale, prior_prec, idx)
    q0 = rs.randn(P) * .1
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


@pytest.fixture(scope='module')
def traj_problem():
    return {kind: _grid_problem(kind, 2000, 60, 2, n_grid=30)[2:]
            for kind in ('tiled_binary', 'dense64')}


# the stability limit of the dense problem (_stability_limit) is .069; the
# Hamiltonian of one step of .05 already moves by more than the tolerance 100
TRAJ_DT = .02


@pytest.mark.parametrize('n_step', [0, 1, 20])
@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_trajectory_matches_host_velocity_verlet(traj_problem, kind, n_step):
    model, X, idx = traj_problem[kind]
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(X, idx)
    want = lo.trajectory(f, TRAJ_DT, n_step, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(TRAJ_DT, n_step, scale, pp, q0, p0, logp0,
                               grad0)
    assert not want[5] and not got['instability']
    assert got['n_steps'] == want[4] == n_step
    np.testing.assert_allclose(got['q'], want[0], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got['p'], want[1], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got['grad'], want[3], rtol=1e-9, atol=1e-12)
    assert math.isfinite(want[2])
    assert got['logp'] == pytest.approx(want[2], rel=1e-11)
    assert got['hamiltonian'][0] == pytest.approx(want[6], rel=1e-13)
    assert got['hamiltonian'][1] == pytest.approx(want[7], rel=1e-11)
    if n_step == 0:
        assert got['hamiltonian'][0] == got['hamiltonian'][1]
    again = model.hmc_trajectory(TRAJ_DT, n_step, scale, pp, q0, p0, logp0,
                                 grad0)
    for key in ('q', 'p', 'grad', 'hamiltonian'):
        assert np.array_equal(again[key], got[key])


def _stability_limit(X, idx, scale, pp, q0):
    """2 / sqrt(largest curvature of -f at q0), by power iteration on the
    oracle's Hessian."""
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * cwo.scans_hessian_matvec(X, q0 * scale,
                                                       scale * v, idx)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_nuts_doublings_match_the_oracle(kind):
    from test_hip_cox_interval import _compare_doublings
    model, X, idx = _grid_problem(kind, 1000, 20, 12, n_grid=10)[2:]
    oracle = cwo.OracleModel(X, idx)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(X, idx)
    limit = _stability_limit(X, idx, scale, pp, q0)
    print('stability limit', limit)
    args = (model, oracle, scale, pp, q0, p0, logp0, grad0)
    # every height up to 4 in both directions: a step small enough for the
    # 31 steps to make no U-turn
    for first in (1, -1):
        directions = [first * (-1) ** h for h in range(5)]
        outs = _compare_doublings(*args, limit / 200, directions, 100., 5)
        assert [out['height'] for out in outs] == [1, 2, 3, 4, 5]
        assert sum(out['n_steps'] for out in outs) == 31
        assert sum(out['n_uniform'] for out in outs) == 31
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
CHAIN_N, CHAIN_P = 400, 8
# A chain multiplies a rounding difference from iteration to iteration.  The
# seeds are ones at which the oracle's own chain, run again with its
# likelihood and gradient perturbed by 1e-15 relative (a few ulp: what another
# summation order and another exp differ by), agrees with itself to 1e-8 or
# better, three perturbations out of three: the best of seeds 0-11 ('hmc'
# sparse: 0-39) on the CPU, the device not involved (chain_seed_search below:
# 'hmc' sparse 6e-10, dense 2e-9; 'nuts' 9e-10 and 4e-10).
CHAIN_SEED = {('hmc', 'sparse'): 39, ('hmc', 'dense'): 10,
              ('nuts', 'sparse'): 1, ('nuts', 'dense'): 1}


def chain_problem(fmt):
    """Unsorted (event, censoring, X, weights): times on a 10-point grid,
    weights lognormal(0, 1/2)."""
    rs = np.random.RandomState(13)
    if fmt == 'sparse':
        X = sparse.random(CHAIN_N, CHAIN_P, density=.3, format='csr',
                          random_state=rs)
        X.data[:] = 1.
    else:
        X = rs.randn(CHAIN_N, CHAIN_P) * .5
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    event, cens = cwo.make_times(dense, 13, n_grid=10)
    return event, cens, X, np.exp(.5 * rs.randn(CHAIN_N))


def chain_sorted(fmt):
    """(sorted event, censoring, X, idx, the maximum partial-likelihood
    coefficients): the chain starts there, so it has no long transient
    trajectories and no mode search runs."""
    from bayesbridge_amd.model import cox_preprocess
    event, cens, X, a = chain_problem(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, X, keep = cox_preprocess(event, cens, X)
    idx = cwo.index_arrays(event, cens, a[keep])
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    return event, cens, X, idx, cwo.newton_mle(dense, idx)


def _chain(fmt, method, seed, oracle=False, n_iter=12, resume=None):
    from bayesbridge_amd import RegressionModel
    from test_hip_cox_interval import run_chain
    event, cens, X, a = chain_problem(fmt)
    _, _, Xs, idx, start = chain_sorted(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', weights=a)
    assert model._ham_prefix == 'bbx_coxw_' and not model.intercept_added
    # the unsorted rows' weights went with them
    assert np.array_equal(model.weights, idx[4])
    assert not np.array_equal(model.weights, a)
    if oracle:
        model = cwo.OracleModel(Xs, idx, design=model.design)
    return run_chain(model, method, seed, start, n_iter, resume)


@pytest.mark.parametrize('method,fmt', [('hmc', 'dense'), ('hmc', 'sparse'),
                                        ('nuts', 'dense'), ('nuts', 'sparse')])
def test_seeded_chain_matches_the_driver_on_the_oracle(method, fmt):
    from bayesbridge_amd.bayesbridge import HMC_INFO_KEYS, NUTS_INFO_KEYS
    seed = CHAIN_SEED[method, fmt]
    samples, info = _chain(fmt, method, seed)
    want, winfo = _chain(fmt, method, seed, oracle=True)
    assert info['coef_sampler_type'] == method
    assert info['options']['rng'] == 'reference'
    assert set(samples) == {'coef', 'local_scale', 'global_scale', 'logp'}
    assert 'obs_prec' not in info['_markov_chain_state']
    assert samples['coef'].shape == (CHAIN_P, 12)
    si, wsi = (i['_reg_coef_sampling_info'] for i in (info, winfo))
    assert set(si) == set(wsi) == set(HMC_INFO_KEYS if method == 'hmc'
                                      else NUTS_INFO_KEYS)
    steps = 'n_integrator_step' if method == 'hmc' else 'tree_height'
    print(steps, si[steps], 'n_grad_evals', si['n_grad_evals'], 'max rel coef',
          np.max(np.abs(samples['coef'] - want['coef'])
                 / (np.abs(want['coef']) + 1e-3)))
    for key in ('coef', 'global_scale', 'logp', 'local_scale'):
        np.testing.assert_allclose(samples[key], want[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)
    for key in si:
        np.testing.assert_allclose(si[key], wsi[key], rtol=RTOL, atol=ATOL,
                                   err_msg=key)
    assert np.all(si['n_grad_evals'] > 1)
    # two halves through gibbs_resume against the straight run
    resumed, rinfo = _chain(fmt, method, seed, n_iter=6, resume=6)
    assert rinfo['n_iter'] == 12
    for key in samples:
        np.testing.assert_allclose(resumed[key], samples[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)
    for key in si:
        np.testing.assert_allclose(rinfo['_reg_coef_sampling_info'][key],
                                   si[key], rtol=RTOL, atol=ATOL, err_msg=key)


def test_default_sampler_and_mode_search():
    """No sampler named: 'hmc'; no coefficients given: the mode search runs on
    the device likelihood, without obs_prec."""
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    event, cens, X, a = chain_problem('dense')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', weights=a,
                                add_intercept=True)
        assert not model.intercept_added
        samples, info = BayesBridge(
            model, RegressionCoefPrior(bridge_exponent=.5,
                                       regularizing_slab_size=1.)).gibbs(
            3, init={'global_scale': .1}, seed=1)
    assert info['coef_sampler_type'] == 'hmc'
    assert info['_init_optim_info']['is_success']
    assert set(samples) == {'coef', 'global_scale', 'logp'}
    assert np.all(np.isfinite(samples['coef']))
    assert 'obs_prec' not in info['_markov_chain_state']


# ---------------------------------------------------------------- refusals
def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def test_create_refuses_bad_weights_and_index_arrays_with_a_message():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    event, cens, sX, idx, _ = chain_sorted('dense')
    n, ne = len(event), idx[0]
    design = HipDenseDesignMatrix(sX, add_intercept=False)
    names = ('start', 'end', 'n_app', 'weights')
    good = dict(zip(names[:3], (np.ascontiguousarray(v, dtype=np.int32)
                                for v in idx[1:4])))
    good['weights'] = np.ascontiguousarray(idx[4], dtype=np.float64)

    def create(n_event=ne, out=True, dsn=design.handle, **over):
        arrays = dict(good)
        arrays.update(over)
        h = c_void_p()
        st_ = lib.bbx_coxw_create(dsn, n_event,
                                  *[_ptr(arrays[k]) for k in names],
                                  byref(h) if out else None)
        return st_, h, _lib.last_error()

    def changed(name, at, value):
        v = good[name].copy()
        v[at] = value
        return {name: v}

    status, h, _ = create()
    assert status == 0 and h.value
    assert lib.bbx_coxw_destroy(h) == 0
    assert create(out=False)[::2] == (-1, 'NULL output pointer')
    assert create(dsn=None)[::2] == (-1, 'invalid design')
    for name in names[:3]:
        status, h, msg = create(**{name: None})
        assert status == -1 and not h.value and msg == 'NULL index array'
    status, h, msg = create(weights=None)
    assert status == -1 and not h.value and msg == 'NULL weights'
    for bad in (0, -1, n + 1):
        assert create(n_event=bad)[::2] == (-1, 'n_event must be in [1, n]')
    k = ne // 2
    cases = [
        (changed('start', k, -1), 'risk set %d out of range' % k),
        (changed('start', k, k + 1), 'risk set %d out of range' % k),
        (changed('end', k, ne - 2), 'risk set %d out of range' % k),
        (changed('end', k, n), 'risk set %d out of range' % k),
        (changed('n_app', 3, 0), 'n_app[3] outside [1, n_event]'),
        (changed('n_app', 3, ne + 1), 'n_app[3] outside [1, n_event]'),
    ]
    for value in (np.nan, np.inf, -np.inf, 0., -0., -1.5):
        cases.append((changed('weights', 7, value),
                      'weights[7] is not a finite positive number'))
    # the first offending row is the one named
    both = changed('weights', 9, -1.)['weights']
    both[n - 1] = np.nan
    cases.append(({'weights': both},
                  'weights[9] is not a finite positive number'))
    for over, text in cases:
        status, h, msg = create(**over)
        print(text, '->', msg)
        assert status == -1 and not h.value
        assert text in msg, (text, msg)
    # the smallest and the largest finite weights are taken
    tiny = changed('weights', 7, 5e-324)['weights']
    tiny[8] = np.finfo(np.float64).max
    status, h, _ = create(weights=tiny)
    assert status == 0
    assert lib.bbx_coxw_destroy(h) == 0


def test_null_handle_is_refused_by_every_shared_entry_point():
    from bayesbridge_amd import _lib
    calls = hc.Calls(_lib.load(), 'coxw')
    for name in hc.SHARED:
        assert calls.call(name, None) == (
            hc.ERR_INVALID, 'NULL coxw handle'), name
    assert calls.destroy(None) == hc.OK


def chain_seed_search(seeds=range(24), fmts=('sparse', 'dense'),
                      methods=('hmc', 'nuts')):
    """Not a test: prints, for every chain of the table above, the seeds at
    which the oracle's chain agrees with itself under a 1e-15 relative
    perturbation of its likelihood.  CPU only (a stand-in design)."""
    from test_hip_cox_interval import run_chain

    from bayesbridge_amd import HipDesignMatrix

    class Design(HipDesignMatrix):
        intercept_added, shape, device = False, None, 0

        def __init__(self, shape):
            self.shape = shape

    class Perturbed(cwo.OracleModel):
        eps = 0.

        def _f(self, scale, prior_prec):
            base, eps = super()._f(scale, prior_prec), self.eps

            def f(q):
                logp, grad = base(q)
                if grad is None:
                    return logp, grad
                return logp * (1 + eps), grad * (1 - eps)
            return f

    for fmt in fmts:
        _, _, Xs, idx, start = chain_sorted(fmt)
        for method in methods:
            for seed in seeds:
                runs = []
                for eps in (0., 1e-15, -1e-15, 2e-15):
                    model = Perturbed(Xs, idx, design=Design(Xs.shape))
                    model.eps = eps
                    runs.append(run_chain(model, method, seed,
                                          start)[0]['coef'])
                worst = max(np.max(np.abs(r - runs[0])
                                   / (np.abs(runs[0]) + 1e-3))
                            for r in runs[1:])
                print(fmt, method, seed, '%.1e' % worst)
