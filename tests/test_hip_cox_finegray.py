"""GPU: the Fine-Gray competing-risks model (csrc/cox_finegray.hip on
csrc/hamiltonian.hpp) -- the likelihood, its gradient and Hessian matvec
against the NumPy oracle (tests/cox_finegray_oracle.py) on three design types,
at the partition edges of the scans and at one multi-tile size; against the
plain CoxModel where the two likelihoods coincide (no censored rows, no
competing rows) and away from it where they do not; determinism, the empty
risk-set rule and the launch count; the trajectory, No-U-Turn doublings and
whole seeded chains against the same host logic on the oracle; the refusals
of the create call.  The oracle's extended-precision form is the yardstick
(the definition in its docstring, not another package's conventions), and
each comparison first checks on the CPU that the oracle's own float64 scan
form meets the tolerance it holds the device to."""
import math
import warnings
from ctypes import byref, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_cases as cc
import cox_finegray_oracle as cfo
import ham_cabi as hc
import logit_oracle as lo
from test_hip_cox_efron import _betas, _design, _launches, _within

pytestmark = pytest.mark.gpu

# tests/test_hip_cox.py's, for the same quantities against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10
RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance
VALUES = {'dense64': 'normal', 'tiled_binary': 'binary',
          'csr_valued': 'valued'}
INF = float('inf')


def _models(kind, event, cens, comp, X):
    """(the Fine-Gray model on rows already in order, the oracle's X, idx)."""
    from bayesbridge_amd import RegressionModel
    design, X = _design(kind, X)
    model = RegressionModel((event, cens), design, 'cox', competing_time=comp)
    assert model.name == 'cox' and model._ham_prefix == 'bbx_coxfg_'
    assert model.n_pred == X.shape[1] and model.n_obs == len(event)
    assert np.array_equal(model.competing_time, comp)
    return model, X, cfo.model_idx(model)


def _plain_model(event, cens, X):
    """The plain handle on rows it sorts itself (a likelihood does not depend
    on the order of its rows)."""
    from bayesbridge_amd import RegressionModel
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox')
    assert model._ham_prefix == 'bbx_cox_' and model.competing_time is None
    return model


def _oracle_ext(X, beta, v, idx, times):
    if X.shape[0] <= cfo.EXPLICIT_MAX_N:
        W, evrow = cfo.weight_matrix(*times)
        oll, ograd = cfo.explicit_loglik_grad(X, beta, W, evrow)
        return oll, ograd, cfo.explicit_hessian_matvec(X, beta, v, W, evrow)
    oll, ograd = cfo.scans_loglik_grad(X, beta, idx, np.longdouble)
    return oll, ograd, cfo.scans_hessian_matvec(X, beta, v, idx,
                                                np.longdouble)


def _rel(got, want):
    return np.abs(np.asarray(got) - want).max() / (np.abs(want).max() or 1.)


def _all_three(model, beta, v):
    ll, grad = model.compute_loglik_and_gradient(beta)
    return ll, grad, model.get_hessian_matvec_operator(beta)(v)


def _check_against_oracle(model, X, idx, times, betas, vs):
    """Device == oracle at the tolerances, after the CPU check that the
    oracle's float64 scan form is within them of its extended-precision form
    (the explicit weight matrix up to 2049 rows, scans beyond); two calls
    give the same bits."""
    for beta, v in zip(betas, vs):
        oll, ograd, ohv = _oracle_ext(X, beta, v, idx, times)
        assert np.isfinite(oll)
        fll, fgrad = cfo.scans_loglik_grad(X, beta, idx)
        fhv = cfo.scans_hessian_matvec(X, beta, v, idx)
        print('n', X.shape[0], 'oracle f64 vs ext: ll %.2e grad %.2e hess %.2e'
              % (_rel(fll, oll), _rel(fgrad, ograd), _rel(fhv, ohv)))
        assert abs(fll - oll) <= LL_TOL * abs(oll)
        assert _within(fgrad, ograd, GRAD_TOL)
        assert _within(fhv, ohv, HESS_TOL)
        ll, grad, hv = _all_three(model, beta, v)
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


def _grid_times(dense, seed, n_grid, fracs):
    """cfo.make_times with one of the earliest rows made an event, so that no
    row is censored before the first event and every row stays."""
    event, cens, comp = cfo.make_times(dense, seed, n_grid=n_grid, fracs=fracs)
    T = np.minimum(np.minimum(event, cens), comp)
    i = int(np.argmin(T))
    event[i], cens[i], comp[i] = T[i], INF, INF
    return event, cens, comp


def _grid_problem(kind, n, p, seed, n_grid=200, fracs=(1 / 3, 1 / 3)):
    """Sorted rows with times on a grid (times of all three kinds tie):
    (times, model, X, idx)."""
    from bayesbridge_amd.model import cox_preprocess_finegray
    rs = np.random.RandomState(seed)
    X = cc._design(n, p, VALUES[kind], rs, .2 if p <= 20 else .1)
    dense = X if kind.startswith('dense') else np.asarray(X.todense())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, comp, X, keep, _, _ = cox_preprocess_finegray(
            *_grid_times(dense, seed, n_grid, fracs), X)
    assert len(keep) == n
    return ((event, cens, comp),) + _models(kind, event, cens, comp, X)


@pytest.mark.parametrize('kind', ['tiled_binary', 'csr_valued', 'dense64'])
def test_likelihood_gradient_hessian_match_the_oracle(kind):
    """2049 rows x 40 columns, times on a 200-point grid, about a third each
    of events, competing events and censored rows."""
    times, model, X, idx = _grid_problem(kind, 2049, 40, 3)
    assert model.n_obs == 2049
    for count in (idx[0], len(idx[5]), 2049 - idx[0] - len(idx[5])):
        assert 600 < count < 770
    assert idx[6].min() < .25 and idx[7].max() > 4.      # G far from 1
    assert np.intersect1d(times[0], times[1]).size
    assert np.intersect1d(times[0], times[2]).size
    _check_against_oracle(model, X, idx, times, *_betas(40))


EDGES = (1, 2, 255, 256, 257, 2047, 2048, 2049)
BLOCKS = [(L, 3, 2, 'mixed') for L in EDGES] \
    + [(3, L, 2, 'mixed') for L in EDGES] \
    + [(2, 3, L, 'mixed') for L in EDGES] \
    + [(300, 0, 200, 'mixed'), (300, 200, 0, 'mixed'),
       (257, 300, 5, 'before'), (257, 300, 5, 'after'),
       (2, 2049, 0, 'before'), (2049, 2, 0, 'after')]


@pytest.mark.parametrize('ne,n_comp,n_cens,where', BLOCKS)
def test_partition_edges(ne, n_comp, n_cens, where):
    """SCAN_G = 256 chunks per segment, tiles of 2048: the three segment
    lengths (all rows, the competing rows, the events) at the edges; no
    competing rows (the second risk segment is not launched), no censored
    rows, every competing row before the first event (p_i = 0: in every risk
    set by its weight alone) and every one after the last (in every risk set
    with weight 1)."""
    event, cens, comp, X = cfo.blocks_case(ne, n_comp, n_cens, p=3,
                                           seed=ne + 7 * n_comp + 13 * n_cens,
                                           where=where)
    model, X, idx = _models('dense64', event, cens, comp, X)
    assert model.n_event == ne and len(idx[5]) == n_comp
    assert model.n_obs == ne + n_comp + n_cens
    if where == 'before':
        assert np.all(idx[4][idx[5]] == 0) and np.all(idx[3] == n_comp)
    if where == 'after':
        assert np.all(idx[4][idx[5]] == ne) and not np.any(idx[3])
    _check_against_oracle(model, X, idx, (event, cens, comp), *_betas(3))


def test_multi_tile_chunks():
    """524 289 rows, a third of each kind: each of the 256 chunks of the row
    scan holds 2049 elements, one more than a tile."""
    n, p = 524289, 4
    times, model, X, idx = _grid_problem('dense64', n, p, 5, n_grid=5000)
    assert cc.chunk_len(n) == cc.SCAN_TILE + 1
    assert idx[0] > 150000 and len(idx[5]) > 150000
    betas, vs = _betas(p, scales=(.5,))
    _check_against_oracle(model, X, idx, times, betas, vs)


def _compare(got, want):
    d = (abs(got[0] - want[0]) / abs(want[0]), _rel(got[1], want[1]),
         _rel(got[2], want[2]))
    print('vs plain: ll %.2e grad %.2e hess %.2e' % d)
    return d


def test_without_censored_rows_it_is_the_plain_handle_on_recoded_rows():
    """G = 1: every competing row stays in every later risk set with weight 1,
    which is the plain likelihood with the competing rows censored after the
    last event."""
    times, model, X, idx = _grid_problem('dense64', 3000, 12, 6, n_grid=100,
                                         fracs=(.5, 0.))
    event, cens, comp = times
    assert len(idx[5]) > 1000 and np.all(idx[6] == 1.) and np.all(idx[7] == 1.)
    recoded = np.where(np.isfinite(comp), event[np.isfinite(event)].max() + 1.,
                       INF)
    plain = _plain_model(event, recoded, X)
    assert plain.n_obs == 3000 and plain.n_event == model.n_event
    for beta, v in zip(*_betas(12)):
        d = _compare(_all_three(model, beta, v), _all_three(plain, beta, v))
        assert d[0] <= LL_TOL and d[1] <= GRAD_TOL and d[2] <= HESS_TOL
    _check_against_oracle(model, X, idx, times, *_betas(12))


def test_without_competing_rows_it_is_the_plain_handle():
    times, model, X, idx = _grid_problem('dense64', 3000, 12, 7, n_grid=100,
                                         fracs=(0., .5))
    event, cens, comp = times
    assert len(idx[5]) == 0 and idx[6].min() < .5
    plain = _plain_model(event, cens, X)
    assert plain.n_obs == 3000
    for beta, v in zip(*_betas(12)):
        d = _compare(_all_three(model, beta, v), _all_three(plain, beta, v))
        assert d[0] <= LL_TOL and d[1] <= GRAD_TOL and d[2] <= HESS_TOL


def test_censoring_at_the_competing_event_is_another_likelihood():
    """With real censoring and competing rows the model is farther than 100
    tolerances from the plain handle that censors at the competing event, so
    these tests can see the feature."""
    times, model, X, idx = _grid_problem('dense64', 3000, 12, 8, n_grid=100)
    event, cens, comp = times
    plain = _plain_model(event, np.minimum(cens, comp), X)
    assert plain.n_event == model.n_event
    for beta, v in zip(*_betas(12)):
        d = _compare(_all_three(model, beta, v), _all_three(plain, beta, v))
        assert d[0] > 100 * LL_TOL and d[1] > 100 * GRAD_TOL
        assert d[2] > 100 * HESS_TOL
    _check_against_oracle(model, X, idx, times, *_betas(12))


def test_underflowing_risk_set_gives_minus_infinity():
    """Where every hazard at risk underflows the handle reports what the plain
    model reports, for that evaluation only."""
    times, model, X, idx = _grid_problem('dense64', 2000, 20, 9, n_grid=50)
    beta = np.zeros(20)
    beta[0] = 2000.       # exp(eta - max) underflows for most rows
    assert cfo.scans_loglik_grad(X, beta, idx) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
        == (-np.inf, None)
    from bayesbridge_amd import _lib
    b = np.ascontiguousarray(beta)
    assert _lib.load().bbx_coxfg_set_location(
        model.handle, b.ctypes.data_as(c_void_p)) == _lib.ERR_NUMERIC
    with pytest.raises(ValueError, match='Hessian operator'):
        model.get_hessian_matvec_operator(beta)
    # the flags were that evaluation's only
    zero = np.zeros(20)
    ll, grad = model.compute_loglik_and_gradient(zero)
    oll, ograd = cfo.scans_loglik_grad(X, zero, idx)
    assert abs(ll - oll) <= LL_TOL * abs(oll)
    assert _within(grad, ograd, GRAD_TOL)
    assert np.all(np.isfinite(model.get_hessian_matvec_operator(zero)(b)))
    # a trajectory whose first step lands there reports instability
    P = 20
    scale, pp = np.ones(P), np.ones(P)
    f = cfo.precond_f(X, scale, pp, idx)
    q0, p0 = np.zeros(P), beta.copy()
    logp0, grad0 = f(q0)
    want = lo.trajectory(f, 1., 10, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(1., 10, scale, pp, q0, p0, logp0, grad0)
    assert want[5] and want[4] == 1 and want[2] == -np.inf
    assert got['instability'] is True and got['n_steps'] == 1
    assert got['logp'] == -np.inf and got['grad'] is None


def test_launch_count_is_the_plain_handles():
    times, model, X, idx = _grid_problem('dense64', 1300, 6, 8, n_grid=40)
    event, cens, comp = times
    plain = _plain_model(event, np.minimum(cens, comp), X)
    beta = _betas(6)[0][0]
    counts = _launches(model, beta), _launches(plain, beta)
    print('launches (fine-gray, plain): %s' % (counts,))
    assert counts[0] == counts[1] > 6
    # and without competing rows, where one risk segment is not launched
    times, model, X, idx = _grid_problem('dense64', 1300, 6, 8, n_grid=40,
                                         fracs=(0., .5))
    assert _launches(model, beta) == counts[1]


def _traj_inputs(X, idx, seed=0):
    P = X.shape[1]
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    prior_prec = np.ones(P)
    f = cfo.precond_f(X, scale, prior_prec, idx)
    q0 = rs.randn(P) * .1
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


@pytest.fixture(scope='module')
def traj_problem():
    return {kind: _grid_problem(kind, 2000, 60, 2, n_grid=30)[1:]
            for kind in ('tiled_binary', 'dense64')}


# well inside the stability limit of both problems (_stability_limit: .13
# dense, .43 binary): 20 steps move the Hamiltonian by less than 1
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
        hv = pp * v - scale * cfo.scans_hessian_matvec(X, q0 * scale,
                                                       scale * v, idx)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_nuts_doublings_match_the_oracle(kind):
    from test_hip_cox_interval import _compare_doublings
    model, X, idx = _grid_problem(kind, 1000, 20, 12, n_grid=10)[1:]
    oracle = cfo.OracleModel(X, idx)
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
# better, three perturbations out of three: the best of seeds 0-23 on the CPU,
# the device not involved (chain_seed_search below: 'hmc' sparse 3e-10, dense
# 1e-9; 'nuts' 1e-10 and 2e-10).
CHAIN_SEED = {('hmc', 'sparse'): 18, ('hmc', 'dense'): 13,
              ('nuts', 'sparse'): 17, ('nuts', 'dense'): 10}


def chain_problem(fmt):
    """Unsorted (event, censoring, competing, X): times on a 10-point grid."""
    rs = np.random.RandomState(13)
    if fmt == 'sparse':
        X = sparse.random(CHAIN_N, CHAIN_P, density=.3, format='csr',
                          random_state=rs)
        X.data[:] = 1.
    else:
        X = rs.randn(CHAIN_N, CHAIN_P) * .5
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    return cfo.make_times(dense, 13, n_grid=10) + (X,)


def chain_sorted(fmt):
    """(sorted times, X, idx, the maximum partial-likelihood coefficients):
    the chain starts there, so it has no long transient trajectories and no
    mode search runs."""
    from bayesbridge_amd.model import (cox_finegray_risk_sets,
                                       cox_preprocess_finegray)
    event, cens, comp, X = chain_problem(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, comp, X, keep, g, r = cox_preprocess_finegray(
            event, cens, comp, X)
    idx = cox_finegray_risk_sets(event, cens, comp) + (g, r)
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    return (event, cens, comp), X, idx, cfo.newton_mle(dense, idx)


def _chain(fmt, method, seed, oracle=False, n_iter=12, resume=None):
    from bayesbridge_amd import RegressionModel
    from test_hip_cox_interval import run_chain
    event, cens, comp, X = chain_problem(fmt)
    times, Xs, idx, start = chain_sorted(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', competing_time=comp)
    assert model._ham_prefix == 'bbx_coxfg_' and not model.intercept_added
    # the unsorted rows were sorted, and G is the full data's
    assert np.array_equal(model.competing_time, times[2])
    assert not np.array_equal(model.competing_time, comp)
    for got, want in zip(cfo.model_idx(model), idx):
        assert np.array_equal(got, want)
    if oracle:
        model = cfo.OracleModel(Xs, idx, design=model.design)
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
    event, cens, comp, X = chain_problem('dense')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', competing_time=comp,
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


def test_a_prebuilt_design_must_be_in_order():
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    event, cens, comp, X = chain_problem('dense')
    design = HipDenseDesignMatrix(X, add_intercept=False)
    with pytest.raises(ValueError, match="Fine-Gray model's order"):
        RegressionModel((event, cens), design, 'cox', competing_time=comp)


# ---------------------------------------------------------------- refusals
def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def test_create_refuses_bad_arrays_with_a_message():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    times, sX, idx, _ = chain_sorted('dense')
    n, ne, nc = len(times[0]), idx[0], len(idx[5])
    design = HipDenseDesignMatrix(sX, add_intercept=False)
    ints = ('evrow', 'a', 'b', 'p', 'comp_row')
    good = {k: np.ascontiguousarray(v, dtype=np.int32)
            for k, v in zip(ints, idx[1:6])}
    good['event_g'] = np.ascontiguousarray(idx[6], dtype=np.float64)
    good['comp_rinv'] = np.ascontiguousarray(idx[7], dtype=np.float64)
    order = ('evrow', 'a', 'b', 'p', 'n_comp', 'comp_row', 'event_g',
             'comp_rinv')

    def create(n_event=ne, n_comp=nc, out=True, dsn=design.handle, **over):
        arrays = dict(good)
        arrays.update(over)
        h = c_void_p()
        args = [n_comp if k == 'n_comp' else _ptr(arrays[k]) for k in order]
        st_ = lib.bbx_coxfg_create(dsn, n_event, *args,
                                   byref(h) if out else None)
        return st_, h, _lib.last_error()

    def changed(name, at, value):
        v = good[name].copy()
        v[at] = value
        return {name: v}

    status, h, _ = create()
    assert status == 0 and h.value
    assert lib.bbx_coxfg_destroy(h) == 0
    assert create(out=False)[::2] == (-1, 'NULL output pointer')
    assert create(dsn=None)[::2] == (-1, 'invalid design')
    for name in ints:
        status, h, msg = create(**{name: None})
        assert status == -1 and not h.value and msg == 'NULL index array'
    for name in ('event_g', 'comp_rinv'):
        status, h, msg = create(**{name: None})
        assert status == -1 and not h.value and msg == 'NULL factor array'
    for bad in (0, -1, n + 1):
        assert create(n_event=bad)[::2] == (-1, 'n_event must be in [1, n]')
    for bad in (-1, n - ne + 1):
        assert create(n_comp=bad)[::2] == (
            -1, 'n_comp must be in [0, n - n_event]')
    k, j = ne // 2, nc // 2
    row = int(good['comp_row'][j])
    cases = [
        (changed('evrow', k, -1), 'evrow[%d] outside [0, n)' % k),
        (changed('evrow', k, n), 'evrow[%d] outside [0, n)' % k),
        (changed('evrow', k, good['evrow'][k - 1]),
         'evrow[%d] is not increasing' % k),
        (changed('a', k, -1), 'a[%d] outside [0, evrow[k]]' % k),
        (changed('a', k, good['evrow'][k] + 1),
         'a[%d] outside [0, evrow[k]]' % k),
        (changed('a', k, good['a'][k - 1] - 1), 'a[%d] is decreasing' % k),
        (changed('b', k, good['b'][k] + 1),
         'b[%d] is not the number of competing rows before a[k]' % k),
        (changed('b', k, nc + 1),
         'b[%d] is not the number of competing rows before a[k]' % k),
        (changed('b', k, -1),
         'b[%d] is not the number of competing rows before a[k]' % k),
        (changed('p', row, -1), 'p[%d] outside [0, n_event]' % row),
        (changed('p', row, ne + 1), 'p[%d] outside [0, n_event]' % row),
        (changed('p', int(good['evrow'][0]), 0),
         'p[%d] outside [1, n_event]' % good['evrow'][0]),
        (changed('p', n - 1, good['p'][n - 2] - 1), 'p[%d] is decreasing'
         % (n - 1)),
        (changed('comp_row', j, -1), 'comp_row[%d] outside [0, n)' % j),
        (changed('comp_row', j, n), 'comp_row[%d] outside [0, n)' % j),
        (changed('comp_row', j, good['comp_row'][j - 1]),
         'comp_row[%d] is not increasing' % j),
    ]
    # a competing row that is an event row: the event between two of them
    between = [(i, int(e)) for i in range(1, nc) for e in good['evrow']
               if good['comp_row'][i - 1] < e < good['comp_row'][i]]
    i, e = between[0]
    cases.append((changed('comp_row', i, e),
                  'comp_row[%d] is an event row' % i))
    for value in (np.nan, np.inf, -np.inf, 0., -0., -.5, 1.5):
        cases.append((changed('event_g', 7, value),
                      'event_g[7] is not in (0, 1]'))
    for value in (np.nan, np.inf, -np.inf, 0., .5, -2.):
        cases.append((changed('comp_rinv', 7, value),
                      'comp_rinv[7] is not a finite number >= 1'))
    # the first offender is the one named
    both = changed('comp_rinv', 9, .5)['comp_rinv']
    both[nc - 1] = np.nan
    cases.append(({'comp_rinv': both},
                  'comp_rinv[9] is not a finite number >= 1'))
    for over, text in cases:
        status, h, msg = create(**over)
        print(text, '->', msg)
        assert status == -1 and not h.value
        assert text in msg, (text, msg)
    # the ends of the ranges are taken; without competing rows the two arrays
    # of theirs may be NULL
    edge_g = changed('event_g', 7, 5e-324)['event_g']
    edge_g[8] = 1.
    edge_r = changed('comp_rinv', 7, np.finfo(np.float64).max)['comp_rinv']
    edge_r[8] = 1.
    status, h, _ = create(event_g=edge_g, comp_rinv=edge_r)
    assert status == 0
    assert lib.bbx_coxfg_destroy(h) == 0
    status, h, msg = create(n_comp=0, comp_row=None, comp_rinv=None,
                            b=np.zeros(ne, dtype=np.int32),
                            p=np.maximum(good['p'], 1))
    assert status == 0, msg
    assert lib.bbx_coxfg_destroy(h) == 0


def test_null_handle_is_refused_by_every_shared_entry_point():
    from bayesbridge_amd import _lib
    calls = hc.Calls(_lib.load(), 'coxfg')
    for name in hc.SHARED:
        assert calls.call(name, None) == (
            hc.ERR_INVALID, 'NULL coxfg handle'), name
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

    class Perturbed(cfo.OracleModel):
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
        _, Xs, idx, start = chain_sorted(fmt)
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
