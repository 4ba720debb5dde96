"""GPU: Efron's tied event times in the Cox model (csrc/cox_efron.hip on
csrc/hamiltonian.hpp) -- the likelihood, its gradient and Hessian matvec
against the NumPy oracle (tests/cox_efron_oracle.py) on four design types, at
the partition edges of the scans with tie groups across them, and on edge
data; against the plain CoxModel with and without ties; the launch count; the
empty risk-set rule; the trajectory, No-U-Turn doublings and whole seeded
chains against the same host logic on the oracle; the refusals of the create
call.  There is no reference implementation of this likelihood: the oracle's
extended-precision form is the yardstick, and each comparison first checks on
the CPU that the oracle's own float64 scan form meets the tolerance it holds
the device to."""
import warnings
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_cases as cc
import cox_efron_oracle as ceo
import ham_cabi as hc
import logit_oracle as lo

pytestmark = pytest.mark.gpu

# tests/test_hip_cox.py's, for the same quantities against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10
RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance
VALUES = {'dense64': 'normal', 'dense32': 'normal', 'tiled_binary': 'binary',
          'csr_valued': 'valued'}


def _design(kind, X):
    """(design, the matrix the oracle uses).  As test_hip_cox_edges._model:
    sparse designs go through the raw CSR path and dense ones with a constant
    column through the device-array path, which keep constant columns (one or
    two rows make every column constant)."""
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if kind in ('dense64', 'dense32'):
        dtype = 'float32' if kind == 'dense32' else 'float64'
        if dtype == 'float32':
            X = X.astype(np.float32).astype(np.float64)
        if np.any(np.var(X, axis=0) < X.shape[0] * 2. ** -52):
            import torch
            t = torch.from_numpy(np.ascontiguousarray(X)).cuda()
            design = HipDenseDesignMatrix.from_device_array(
                X.shape[0], X.shape[1], t.data_ptr(), add_intercept=False,
                in_dtype='float64', storage_dtype=dtype)
            torch.cuda.synchronize()
        else:
            design = HipDenseDesignMatrix(X, add_intercept=False,
                                          storage_dtype=dtype)
        return design, X
    X = sparse.csr_matrix(X)
    X.sort_indices()
    storage = 'csr' if kind == 'csr_valued' else 'tiled'
    return HipSparseDesignMatrix.from_csr_arrays(
        X.shape, X.indptr, X.indices, X.data, add_intercept=False,
        storage=storage), X


def _models(kind, event, cens, X, plain=False):
    """(the Efron model on rows already in order, the oracle's X, idx[, the
    plain model on the same design])."""
    from bayesbridge_amd import RegressionModel
    design, X = _design(kind, X)
    model = RegressionModel((event, cens), design, 'cox', ties='efron')
    assert model.name == 'cox' and model._ham_prefix == 'bbx_coxef_'
    assert model.n_pred == X.shape[1]
    idx = (model.n_event, model.risk_set_start_index,
           model.risk_set_end_index, model.n_appearance_in_risk_set,
           model.tie_group_size)
    if plain:
        other = RegressionModel((event, cens), design, 'cox')
        assert other._ham_prefix == 'bbx_cox_'
        return model, X, idx, other
    return model, X, idx


def _with_groups(case, groups):
    """The case with events a .. b-1 tied, for every (a, b): distinct times
    elsewhere.  The censoring times stay (none is below the first event)."""
    t = np.arange(1., case.n_event + 1.)
    for a, b in groups:
        t[a:b] = t[a]
    return case._replace(event_time=np.concatenate(
        (t, case.event_time[case.n_event:])))


def _straddling_groups(ne, width):
    """Tie groups of `width` events, one across each chunk or tile boundary of
    the event scans (forward and reversed) that the one before leaves room
    for."""
    groups = []
    for b in cc.event_boundaries(ne):
        a = max(int(b) - width // 2, 0)
        e = min(a + width, ne)
        if e - a >= 2 and a < b < e and (not groups or a >= groups[-1][1]):
            groups.append((a, e))
    return groups


def _within(got, want, tol):
    return np.all(np.abs(np.asarray(got) - want) <= tol * np.abs(want).max())


def _oracle_ext(X, beta, v, idx, event, cens):
    if X.shape[0] <= ceo.EXPLICIT_MAX_N:
        oll, ograd = ceo.explicit_loglik_grad(X, beta, event, cens)
        return oll, ograd, ceo.explicit_hessian_matvec(X, beta, v, event,
                                                       cens)
    oll, ograd = ceo.scans_loglik_grad(X, beta, idx, np.longdouble)
    return oll, ograd, ceo.scans_hessian_matvec(X, beta, v, idx,
                                                np.longdouble)


def _check_against_oracle(model, X, idx, event, cens, betas, vs):
    """Device == oracle at the tolerances, after the CPU check that the
    oracle's float64 scan form is within them of its extended-precision form
    (the explicit loop up to 2049 rows, scans beyond); two calls give the
    same bits."""
    for beta, v in zip(betas, vs):
        oll, ograd, ohv = _oracle_ext(X, beta, v, idx, event, cens)
        assert np.isfinite(oll)
        fll, fgrad = ceo.scans_loglik_grad(X, beta, idx)
        fhv = ceo.scans_hessian_matvec(X, beta, v, idx)

        def rel(ll, grad, hv):
            return (abs(ll - oll) / (abs(oll) or 1.),
                    np.abs(grad - ograd).max() / (np.abs(ograd).max() or 1.),
                    np.abs(hv - ohv).max() / (np.abs(ohv).max() or 1.))

        print('n', X.shape[0], 'oracle f64 vs ext: ll %.2e grad %.2e hess %.2e'
              % rel(fll, fgrad, fhv))
        assert abs(fll - oll) <= LL_TOL * abs(oll)
        assert _within(fgrad, ograd, GRAD_TOL)
        assert _within(fhv, ohv, HESS_TOL)
        ll, grad = model.compute_loglik_and_gradient(beta)
        hv = model.get_hessian_matvec_operator(beta)(v)
        print('   device vs ext: ll %.2e grad %.2e hess %.2e'
              % rel(ll, grad, hv))
        assert abs(ll - oll) <= LL_TOL * abs(oll)
        assert _within(grad, ograd, GRAD_TOL)
        assert _within(hv, ohv, HESS_TOL)
        ll2, grad2 = model.compute_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        assert np.array_equal(model.get_hessian_matvec_operator(beta)(v), hv)
        assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
            == (ll, None)
        assert model.hamiltonian_loglik_and_gradient(beta)[0] == ll


def _betas(p, seed=1, scales=(.1, 1.)):
    rs = np.random.RandomState(seed)
    return [rs.randn(p) * s for s in scales], [rs.randn(p) for _ in scales]


@pytest.mark.parametrize('kind', ['tiled_binary', 'csr_valued', 'dense64',
                                  'dense32'])
def test_likelihood_gradient_hessian_match_the_oracle(kind):
    """2049 rows on a 12-point grid of times: tie groups a hundred deep,
    censoring times tied to event times."""
    n, p = 2049, 40
    X = cc._design(n, p, VALUES[kind], np.random.RandomState(3), .1)
    dense = X if kind.startswith('dense') else np.asarray(X.todense())
    from bayesbridge_amd.model import cox_preprocess
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, X, _ = cox_preprocess(*ceo.grid_times(dense, 3, 12), X)
    model, X, idx = _models(kind, event, cens, X)
    assert idx[4].min() > 20 and len(np.unique(idx[4])) > 5
    assert np.intersect1d(event, cens).size
    _check_against_oracle(model, X, idx, event, cens, *_betas(p))


SUBSET = [(1, 0), (2, 0), (2, 1), (1, 2049), (255, 2049), (256, 0), (257, 1),
          (2047, 0), (2048, 1), (2049, 2049)]


@pytest.mark.parametrize('width', [2, 7])
@pytest.mark.parametrize('ne,n_cens', SUBSET)
def test_partition_edges_with_straddling_tie_groups(ne, n_cens, width):
    """SCAN_G = 256 chunks per segment, tiles of 2048: segment lengths at the
    edges, a tie group of `width` across every chunk and tile boundary of the
    event scans.  One event alone: every result is exactly 0."""
    case = cc.cox_case(ne, n_cens, p=3, seed=ne + 7 * n_cens)
    groups = _straddling_groups(ne, width)
    case = _with_groups(case, groups)
    model, X, idx = _models('dense64', case.event_time, case.censoring_time,
                            case.X)
    assert model.n_obs == ne + n_cens
    if ne > width:
        assert groups and idx[4].max() == width
        bounds = set(cc.event_boundaries(ne))
        assert all(any(a < b < e for b in bounds) for a, e in groups)
    if (ne, n_cens) == (1, 0):
        beta = np.array([.3, -.2, .1])
        assert model.compute_loglik_and_gradient(beta)[0] == 0.
        assert not model.compute_loglik_and_gradient(beta)[1].any()
        assert not model.get_hessian_matvec_operator(beta)(beta).any()
        return
    _check_against_oracle(model, X, idx, case.event_time,
                          case.censoring_time, *_betas(3))


@pytest.mark.parametrize('kind', ['dense64', 'tiled_binary'])
def test_one_tie_group_of_all_events(kind):
    case = cc.cox_case(700, 300, p=10, values=VALUES[kind], seed=2)
    case = _with_groups(case, [(0, 700)])
    model, X, idx = _models(kind, case.event_time, case.censoring_time,
                            case.X)
    assert np.all(idx[4] == 700) and np.all(idx[1] == 0)
    _check_against_oracle(model, X, idx, case.event_time,
                          case.censoring_time, *_betas(10))


def test_last_tie_group_with_nothing_else_at_risk():
    """No censored rows and the last 9 events tied: R = 0 for that group, and
    phi = a T with nothing subtracted."""
    case = _with_groups(cc.cox_case(600, 0, p=5, seed=4), [(591, 600),
                                                            (100, 103)])
    model, X, idx = _models('dense64', case.event_time, case.censoring_time,
                            case.X)
    assert np.all(idx[4][591:] == 9) and np.all(idx[2] == 599)
    _check_against_oracle(model, X, idx, case.event_time,
                          case.censoring_time, *_betas(5))


def test_multi_tile_chunks_with_ties_of_three():
    """524 289 events: each of the 256 chunks holds 2049 elements, one more
    than a tile; groups of three from row 1 on, so that one lies across the
    first tile boundary (2048) and the first chunk boundary (2049)."""
    ne, p = 524289, 4
    case = cc.cox_case(ne, 1, p=p, seed=5)
    # a group of 7 and one of 2 across the tile boundaries of chunks 1 and 2
    special = [(4094, 4101), (6145, 6147)]
    assert all(a < b * 2049 + 2048 < e for b, (a, e) in enumerate(special, 1))
    groups = [(a, min(a + 3, ne)) for a in range(1, ne, 3)]
    groups = [g for g in groups
              if not any(g[0] < e and a < g[1] for a, e in special)] + special
    case = _with_groups(case, groups)
    model, X, idx = _models('dense64', case.event_time, case.censoring_time,
                            case.X)
    assert cc.chunk_len(ne) == cc.SCAN_TILE + 1
    assert np.all(idx[4][7000:-2] == 3) and idx[1][2049] == 2047
    assert idx[4][4097] == 7 and idx[4][6146] == 2
    betas, vs = _betas(p, scales=(.5,))
    _check_against_oracle(model, X, idx, case.event_time,
                          case.censoring_time, betas, vs)


def test_against_the_plain_handle_with_and_without_ties():
    """No ties: the plain handle's values at the tolerances (another order of
    the same sums, so not bit for bit).  With ties: farther than 100
    tolerances from them, so these tests can see the feature."""
    base = cc.cox_case(1500, 1500, p=12, seed=6)
    beta, v = _betas(12, scales=(.5,))
    beta, v = beta[0], v[0]
    for groups, tied in (([], False),
                         ([(a, a + 5) for a in range(0, 1500, 5)], True)):
        case = _with_groups(base, groups)
        model, X, idx, plain = _models('dense64', case.event_time,
                                       case.censoring_time, case.X, True)
        assert (idx[4].max() > 1) == tied
        ll, grad = model.compute_loglik_and_gradient(beta)
        pll, pgrad = plain.compute_loglik_and_gradient(beta)
        hv = model.get_hessian_matvec_operator(beta)(v)
        phv = plain.get_hessian_matvec_operator(beta)(v)
        d = (abs(ll - pll) / abs(pll),
             np.abs(grad - pgrad).max() / np.abs(pgrad).max(),
             np.abs(hv - phv).max() / np.abs(phv).max())
        print('tied' if tied else 'no ties',
              'vs plain: ll %.2e grad %.2e hess %.2e' % d)
        if tied:
            assert ll > pll
            assert d[0] > 100 * LL_TOL and d[1] > 100 * GRAD_TOL
            assert d[2] > 100 * HESS_TOL
        else:
            assert d[0] <= LL_TOL and d[1] <= GRAD_TOL and d[2] <= HESS_TOL
        _check_against_oracle(model, X, idx, case.event_time,
                              case.censoring_time, [beta], [v])


def _launches(model, beta):
    from bayesbridge_amd import _lib
    lib = _lib.load()
    lib.bbx_launch_count.restype = c_uint64
    before = lib.bbx_launch_count()
    model.compute_loglik_and_gradient(beta)
    return lib.bbx_launch_count() - before


def test_launch_count_is_the_plain_handles():
    base = cc.cox_case(900, 400, p=6, seed=8)
    beta = base.beta
    counts = []
    for groups in ([], [(0, 900)]):
        case = _with_groups(base, groups)
        model, X, idx, plain = _models('dense64', case.event_time,
                                       case.censoring_time, case.X, True)
        assert np.all(idx[4] == (900 if groups else 1))
        counts.append((_launches(model, beta), _launches(plain, beta)))
    print('launches (efron, plain): no ties %s, all tied %s' % tuple(counts))
    assert counts[0][0] == counts[0][1] == counts[1][0] == counts[1][1] > 6


def test_steep_hazards_with_ties_stay_finite():
    """cox_cases.steep_case with every second pair of events tied: hazards
    that fall by e^7 from row to row in bursts.  Every phi of the oracle is
    positive, so the device is finite (a phi formed as a difference from the
    total would be 0 for the late events)."""
    case = cc.steep_case(4099, 1)
    case = _with_groups(case, [(a, a + 2) for a in range(0, 4098, 4)])
    model, X, idx = _models('dense64', case.event_time, case.censoring_time,
                            case.X)
    assert idx[4].max() == 2
    phi = ceo.phi_ext(X, case.beta, idx)
    assert np.all(phi > 0) and phi.max() / phi.min() > 1e30
    ll, grad = model.compute_loglik_and_gradient(case.beta)
    oll, ograd = ceo.scans_loglik_grad(X, case.beta, idx, np.longdouble)
    print('steep: device vs ext ll %.2e' % (abs(ll - oll) / abs(oll)))
    assert np.isfinite(ll) and np.all(np.isfinite(grad))
    assert abs(ceo.scans_loglik_grad(X, case.beta, idx)[0] - oll) \
        <= LL_TOL * abs(oll)
    assert abs(ll - oll) <= LL_TOL * abs(oll)
    hv = model.get_hessian_matvec_operator(case.beta)(np.array([.7, -1.1]))
    assert np.all(np.isfinite(hv))


def _grid_problem(kind, n, p, seed, n_grid=10):
    from bayesbridge_amd.model import cox_preprocess
    X = cc._design(n, p, VALUES[kind], np.random.RandomState(seed), .2)
    dense = X if kind.startswith('dense') else np.asarray(X.todense())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, X, _ = cox_preprocess(
            *ceo.grid_times(dense, seed, n_grid), X)
    return _models(kind, event, cens, X)


def test_underflowing_risk_set_gives_minus_infinity():
    """Where every hazard at risk underflows the handle reports what the
    plain model reports."""
    model, X, idx = _grid_problem('dense64', 2000, 20, 9, n_grid=50)
    beta = np.zeros(20)
    beta[0] = 2000.       # exp(eta - max) underflows for most rows
    assert ceo.scans_loglik_grad(X, beta, idx) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
        == (-np.inf, None)
    from bayesbridge_amd import _lib
    b = np.ascontiguousarray(beta)
    assert _lib.load().bbx_coxef_set_location(
        model.handle, b.ctypes.data_as(c_void_p)) == _lib.ERR_NUMERIC
    with pytest.raises(ValueError, match='Hessian operator'):
        model.get_hessian_matvec_operator(beta)
    # the flags were that evaluation's only
    ll = model.compute_loglik_and_gradient(beta * 0)[0]
    assert abs(ll - ceo.scans_loglik_grad(X, beta * 0, idx)[0]) \
        <= LL_TOL * abs(ll)
    # a trajectory whose first step lands there reports instability
    P = 20
    scale, pp = np.ones(P), np.ones(P)
    f = ceo.precond_f(X, scale, pp, idx)
    q0, p0 = np.zeros(P), beta.copy()
    logp0, grad0 = f(q0)
    want = lo.trajectory(f, 1., 10, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(1., 10, scale, pp, q0, p0, logp0, grad0)
    assert want[5] and want[4] == 1 and want[2] == -np.inf
    assert got['instability'] is True and got['n_steps'] == 1
    assert got['logp'] == -np.inf and got['grad'] is None


def _traj_inputs(X, idx, seed=0):
    P = X.shape[1]
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    prior_prec = np.ones(P)
    f = ceo.precond_f(X, scale, prior_prec, idx)
    q0 = rs.randn(P) * .1
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


@pytest.fixture(scope='module')
def traj_problem():
    return {kind: _grid_problem(kind, 2000, 60, 2, n_grid=30)
            for kind in ('tiled_binary', 'dense64')}


@pytest.mark.parametrize('n_step', [0, 1, 20])
@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_trajectory_matches_host_velocity_verlet(traj_problem, kind, n_step):
    import math
    model, X, idx = traj_problem[kind]
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(X, idx)
    want = lo.trajectory(f, .05, n_step, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(.05, n_step, scale, pp, q0, p0, logp0, grad0)
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
    again = model.hmc_trajectory(.05, n_step, scale, pp, q0, p0, logp0, grad0)
    for key in ('q', 'p', 'grad', 'hamiltonian'):
        assert np.array_equal(again[key], got[key])


def _stability_limit(X, idx, scale, pp, q0):
    """2 / sqrt(largest curvature of -f at q0), by power iteration on the
    oracle's Hessian."""
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * ceo.scans_hessian_matvec(X, q0 * scale,
                                                       scale * v, idx)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_nuts_doublings_match_the_oracle(kind):
    from test_hip_cox_interval import _compare_doublings
    model, X, idx = _grid_problem(kind, 1000, 20, 12)
    oracle = ceo.OracleModel(X, idx)
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
# better, three perturbations out of three: the best of seeds 0-9 ('hmc' dense:
# 0-23) on the CPU, the device not involved (chain_seed_search below: 'hmc'
# sparse 7e-10, dense 4e-9; 'nuts' 3e-10 and 3e-10).
CHAIN_SEED = {('hmc', 'sparse'): 7, ('hmc', 'dense'): 14,
              ('nuts', 'sparse'): 8, ('nuts', 'dense'): 1}


def chain_problem(fmt):
    """Unsorted (event, censoring, X): times on a 10-point grid."""
    rs = np.random.RandomState(13)
    if fmt == 'sparse':
        X = sparse.random(CHAIN_N, CHAIN_P, density=.3, format='csr',
                          random_state=rs)
        X.data[:] = 1.
    else:
        X = rs.randn(CHAIN_N, CHAIN_P) * .5
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    event, cens = ceo.grid_times(dense, 13, 10)
    return event, cens, X


def chain_sorted(fmt):
    """(sorted event, censoring, X, idx, the maximum partial-likelihood
    coefficients): the chain starts there, so it has no long transient
    trajectories and no mode search runs."""
    from bayesbridge_amd.model import cox_preprocess
    event, cens, X = chain_problem(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        event, cens, X, _ = cox_preprocess(event, cens, X)
    idx = ceo.index_arrays(event, cens)
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    return event, cens, X, idx, ceo.newton_mle(dense, idx)


def _chain(fmt, method, seed, oracle=False, n_iter=12, resume=None):
    from bayesbridge_amd import RegressionModel
    from test_hip_cox_interval import run_chain
    event, cens, X = chain_problem(fmt)
    _, _, Xs, idx, start = chain_sorted(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', ties='efron')
    assert model._ham_prefix == 'bbx_coxef_' and not model.intercept_added
    assert np.array_equal(model.tie_group_size, idx[4]) and idx[4].min() > 5
    if oracle:
        model = ceo.OracleModel(Xs, idx, design=model.design)
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
    event, cens, X = chain_problem('dense')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', ties='efron',
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


def test_create_refuses_bad_index_arrays_with_a_message():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    event, cens, sX, idx, _ = chain_sorted('dense')
    n, ne = len(event), idx[0]
    design = HipDenseDesignMatrix(sX, add_intercept=False)
    names = ('start', 'end', 'n_app')
    good = dict(zip(names, (np.ascontiguousarray(v, dtype=np.int32)
                            for v in idx[1:4])))

    def create(n_event=ne, out=True, dsn=design.handle, **over):
        arrays = dict(good)
        arrays.update(over)
        h = c_void_p()
        st_ = lib.bbx_coxef_create(dsn, n_event,
                                   *[_ptr(arrays[k]) for k in names],
                                   byref(h) if out else None)
        return st_, h, _lib.last_error()

    def changed(name, at, value):
        v = good[name].copy()
        v[at] = value
        return {name: v}

    status, h, _ = create()
    assert status == 0 and h.value
    assert lib.bbx_coxef_destroy(h) == 0
    assert create(out=False)[::2] == (-1, 'NULL output pointer')
    assert create(dsn=None)[::2] == (-1, 'invalid design')
    for name in names:
        status, h, msg = create(**{name: None})
        assert status == -1 and not h.value and msg == 'NULL index array'
    for bad in (0, -1, n + 1):
        assert create(n_event=bad)[::2] == (-1, 'n_event must be in [1, n]')
    start, end, n_app = (good[k] for k in names)
    # k: the second event of the second tie group; its group starts at s > 0
    s = int(start[start > 0][0])
    k = s + 1
    assert start[k] == s and start[s - 1] == 0 and s >= 3
    last = ne - 1
    assert ne <= end[last - 1] < n - 1
    i = int(np.flatnonzero(n_app < ne)[0])
    cases = [
        (changed('start', k, -1), 'start[%d] outside [0, k]' % k),
        (changed('start', k, k + 1), 'start[%d] outside [0, k]' % k),
        (changed('start', k, 0), 'start[%d] is decreasing' % k),
        # in range and not decreasing, but inside a group
        (changed('start', s - 1, 1),
         'start[%d] is not the first row of a contiguous tie group' % (s - 1)),
        (changed('end', k, ne - 2), 'end[%d] outside [n_event - 1, n)' % k),
        (changed('end', k, n), 'end[%d] outside [n_event - 1, n)' % k),
        (changed('end', last, end[last - 1] + 1),
         'end[%d] is increasing' % last),
        (changed('n_app', 3, 0), 'n_app[3] outside [1, n_event]'),
        (changed('n_app', 3, ne + 1), 'n_app[3] outside [1, n_event]'),
        (changed('n_app', i, s + 1),
         'n_app[%d] does not end on a tie-group boundary' % i),
    ]
    for over, text in cases:
        status, h, msg = create(**over)
        print(text, '->', msg)
        assert status == -1 and not h.value
        assert text in msg, (text, msg)
    # the handle made from the good arrays still computes
    status, h, _ = create()
    assert status == 0
    assert lib.bbx_coxef_destroy(h) == 0


def test_null_handle_is_refused_by_every_shared_entry_point():
    from bayesbridge_amd import _lib
    calls = hc.Calls(_lib.load(), 'coxef')
    for name in hc.SHARED:
        assert calls.call(name, None) == (
            hc.ERR_INVALID, 'NULL coxef handle'), name
    assert calls.destroy(None) == hc.OK


def chain_seed_search(seeds=range(24)):
    """Not a test: prints, for every chain of the table above, the seeds at
    which the oracle's chain agrees with itself under a 1e-15 relative
    perturbation of its likelihood.  CPU only (a stand-in design)."""
    from test_hip_cox_interval import run_chain

    from bayesbridge_amd import HipDesignMatrix

    class Design(HipDesignMatrix):
        intercept_added, shape, device = False, None, 0

        def __init__(self, shape):
            self.shape = shape

    class Perturbed(ceo.OracleModel):
        eps = 0.

        def _f(self, scale, prior_prec):
            base, eps = super()._f(scale, prior_prec), self.eps

            def f(q):
                logp, grad = base(q)
                if grad is None:
                    return logp, grad
                return logp * (1 + eps), grad * (1 - eps)
            return f

    for fmt in ('sparse', 'dense'):
        _, _, Xs, idx, start = chain_sorted(fmt)
        for method in ('hmc', 'nuts'):
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
