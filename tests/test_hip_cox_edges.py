"""GPU: the Cox likelihood kernels (csrc/cox.hip) at the edges of their
scans' partition, against the extended-precision reference of
tests/cox_oracle.py with its componentwise error bound.

Each scan cuts a segment into SCAN_G = 256 chunks of ceil(len / 256) elements
and scans a chunk in tiles of 2048.  The cases (tests/cox_cases.py) put
segment lengths at 256 L +- 1, at one and two tiles per chunk, ties across
every chunk and tile boundary, censored times tied to event times, one
censored row (end_k == ne), and hot rows at the boundaries.  Tolerances are
cox_oracle.EDGE_TOL times the bound; the sensitivity controls show that a
row lost from a risk set, or the censored prefix dropped at end_k == ne, lies
more than 100 tolerances away."""
import math

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_cases as cc
import cox_oracle as co

pytestmark = pytest.mark.gpu

TOL = co.EDGE_TOL
LENGTHS = [1, 2, 255, 256, 257, 2047, 2048, 2049]      # 2049 = 256 * 8 + 1
SIZES = ([(ne, nc) for ne in LENGTHS for nc in [0] + LENGTHS]
         + [(3, 0)])
SUBSET = [(1, 0), (2, 1), (3, 0), (255, 2049), (257, 1), (2048, 0),
          (2049, 256), (256, 2047)]
VALUES = {'dense64': 'normal', 'dense32': 'normal', 'tiled_binary': 'binary',
          'csr_valued': 'valued', 'mixed': 'mixed'}


def _model(kind, case):
    """A device Cox model on the case's rows (already in order) and the
    matrix the reference uses.  Sparse designs go through the raw CSR path,
    which keeps constant columns (n = 1 makes every column constant, and so
    do identical hot rows at n <= 3); dense ones with a constant column go
    through the device-array path, which keeps them too."""
    from bayesbridge_amd import (HipDenseDesignMatrix, HipSparseDesignMatrix,
                                 RegressionModel)
    X = case.X
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
    else:
        X = sparse.csr_matrix(X)
        X.sort_indices()
        storage = 'csr' if kind == 'csr_valued' else 'tiled'
        design = HipSparseDesignMatrix.from_csr_arrays(
            X.shape, X.indptr, X.indices, X.data, add_intercept=False,
            storage=storage)
    model = RegressionModel((case.event_time, case.censoring_time), design,
                            'cox')
    assert model.n_pred == X.shape[1]
    return model, X, (model.n_event, model.risk_set_start_index,
                      model.risk_set_end_index, model.n_appearance_in_risk_set)


def _hot_case(ne, n_cens, values, p=6):
    """Hot rows at a boundary of the event scans (or row 0), at the first
    censored row and at a boundary of the censored scan."""
    b = cc.event_boundaries(ne)
    hot = [b[len(b) // 2] if len(b) else 0]
    if n_cens:
        hot.append(ne)
        cb = cc.scan_starts(n_cens)
        if len(cb):
            hot.append(ne + cb[len(cb) // 2])
    return cc.cox_case(ne, n_cens, p=p, values=values, hot=hot,
                       seed=ne + 7 * n_cens)


def _within(got, want, bound):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    return bool(np.all(np.abs(got - want) <= TOL * bound))


def _check(model, X, risk, betas, v_seed=1):
    """loglik, gradient, the loglik_only path, the Hessian matvec after
    set_location, and bitwise repeats.  Returns the last (loglik, grad)."""
    rs = np.random.RandomState(v_seed)
    for beta in betas:
        ll, grad = model.compute_loglik_and_gradient(beta)
        el, eg, lb, gb = co.loglik_grad_ext(X, beta, *risk)
        assert math.isfinite(el)
        assert abs(ll - el) <= TOL * lb, (ll, el, lb)
        assert _within(grad, eg, gb), np.max(np.abs(grad - eg) / gb)
        lo, none = model.compute_loglik_and_gradient(beta, loglik_only=True)
        assert none is None and lo == ll
        v = rs.randn(len(beta))
        hv = model.get_hessian_matvec_operator(beta)(v)
        eh, hb = co.hessian_matvec_ext(X, beta, v, *risk)
        assert _within(hv, eh, hb), np.max(np.abs(hv - eh) / hb)
        ll2, grad2 = model.compute_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        hv2 = model.get_hessian_matvec_operator(beta)(v)
        assert np.array_equal(hv2, hv)
    return ll, grad


def _sensitivity(X, risk, beta, got, case):
    """The device's result is farther than 100 tolerances from the
    reference with a hot boundary row dropped from its risk sets, and (where
    some risk set ends at the first censored row) with end_k > ne in place
    of end_k >= ne."""
    want = co.loglik_grad_ext(X, beta, *risk)
    assert co.distance_in_tolerances(got, want) <= 1.
    far = co.distance_in_tolerances(
        got, co.loglik_grad_ext(X, beta, *risk, drop=case.hot[0]))
    assert far > 100., far
    if np.any(risk[2] == risk[0]):
        far = co.distance_in_tolerances(
            got, co.loglik_grad_ext(X, beta, *risk, strict_end=True))
        assert far > 100., far


@pytest.mark.parametrize('ne,n_cens', SIZES)
@pytest.mark.parametrize('kind', ['dense64', 'tiled_binary'])
def test_partition_edges(kind, ne, n_cens):
    case = _hot_case(ne, n_cens, VALUES[kind])
    model, X, risk = _model(kind, case)
    betas = [case.beta * .2, case.beta]
    ll, grad = _check(model, X, risk, betas)
    if kind == 'dense64' and (ne, n_cens) != (1, 0):
        _sensitivity(X, risk, betas[-1], (ll, grad), case)


@pytest.mark.parametrize('ne,n_cens', SUBSET)
@pytest.mark.parametrize('kind', ['csr_valued', 'dense32', 'mixed'])
def test_partition_edges_other_designs(kind, ne, n_cens):
    case = _hot_case(ne, n_cens, VALUES[kind], p=10)
    model, X, risk = _model(kind, case)
    _check(model, X, risk, [case.beta * .2, case.beta])


EVENT_HEAVY = [('dense64', 524288, 0), ('dense64', 524289, 1),
               ('dense64', 1048577, 524289), ('tiled_binary', 524289, 1),
               ('tiled_binary', 1048577, 524289)]


@pytest.mark.parametrize('kind,ne,n_cens', EVENT_HEAVY)
def test_event_heavy_multi_tile(kind, ne, n_cens):
    """Event chunks of exactly one tile (524 288 events) and of one tile
    plus one element or more: the carries of the reversed suffix scan and of
    the cumsums of 1/H and z."""
    assert cc.chunk_len(ne) >= cc.SCAN_TILE
    case = _hot_case(ne, n_cens, VALUES[kind], p=4 if kind == 'dense64'
                     else 40)
    model, X, risk = _model(kind, case)
    ll, grad = _check(model, X, risk, [case.beta])
    if kind == 'dense64':
        _sensitivity(X, risk, case.beta, (ll, grad), case)


def test_steep_hazards_across_tiles():
    """test_hip_cox.py's steep hazards at scale: 1/H spans > 1e30 across the
    tiles of the cumsum of 1/H and jumps by > 2^53 within a thread's eight
    elements at tile and chunk boundaries."""
    case = cc.steep_case(1048577, 1)
    model, X, risk = _model('dense64', case)
    _check(model, X, risk, [case.beta])


# -- trajectories ------------------------------------------------------------

def _traj_check(got, want, n_step):
    assert got['n_steps'] == want[3]
    assert got['instability'] == want[4]
    np.testing.assert_allclose(got['q'], want[0], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got['p'], want[1], rtol=1e-9, atol=1e-12)
    if math.isfinite(want[2]):
        assert got['logp'] == pytest.approx(want[2], rel=1e-11)
    else:
        assert got['logp'] == want[2] and got['grad'] is None
    assert got['hamiltonian'][0] == pytest.approx(want[5], rel=1e-13)
    assert got['hamiltonian'][1] == pytest.approx(want[6], rel=1e-11)


def _run_traj(model, X, risk, dt, n_step, tol=100., inputs=None):
    from test_hip_cox import _traj_inputs
    f, scale, pp, q0, p0, logp0, grad0 = inputs or _traj_inputs(model, X,
                                                                risk)
    with np.errstate(all='ignore'):
        want = co.trajectory(f, dt, n_step, q0, p0, logp0, grad0, tol=tol)
    got = model.hmc_trajectory(dt, n_step, scale, pp, q0, p0, logp0, grad0,
                               hamiltonian_tol=tol)
    return got, want


@pytest.mark.parametrize('kind', ['csr_valued', 'dense32', 'mixed'])
def test_trajectory_other_designs(kind):
    from test_hip_cox import _cox_data
    model, X, risk = _cox_data(kind, 3000, 100)
    got, want = _run_traj(model, X, risk, .05, 25)
    assert not want[4] and want[3] == 25
    _traj_check(got, want, 25)


def test_trajectory_event_heavy_multi_tile():
    """12 steps on 524 289 events (two tiles per event chunk); at this n the
    host loop is stable up to dt ~ .001."""
    case = _hot_case(524289, 1, 'normal', p=4)
    model, X, risk = _model('dense64', case)
    got, want = _run_traj(model, X, risk, .0005, 12)
    assert not want[4] and want[3] == 12
    _traj_check(got, want, 12)


@pytest.mark.parametrize('n_step', [0, 1])
def test_trajectory_zero_and_one_step(n_step):
    from test_hip_cox import _cox_data
    model, X, risk = _cox_data('dense64', 3000, 100)
    got, want = _run_traj(model, X, risk, .05, n_step)
    assert want[3] == n_step
    _traj_check(got, want, n_step)
    if n_step == 0:
        assert got['hamiltonian'][0] == got['hamiltonian'][1]


@pytest.mark.parametrize('kind', ['tiled_binary', 'csr_valued'])
def test_trajectory_instability_stop(kind):
    from test_hip_cox import _cox_data
    model, X, risk = _cox_data(kind, 3000, 100)
    got, want = _run_traj(model, X, risk, 3., 200)
    assert want[4] and got['instability']
    assert got['n_steps'] == want[3] < 200


def test_trajectory_stops_at_a_zero_risk_set_sum_after_step_one():
    """Row 0 (the first event) alone carries column 0, so beta_0 = q_0 moves
    by p_0 = 200 per step (its gradient is ~e^-400) from 400: at step 2,
    eta_0 - eta_i = 800 and exp underflows for every later risk set: H_1 ==
    0, logp = -inf.  (Step 1, at 600, stays clear of subnormal hazards.)  A
    huge hamiltonian_tol leaves that as the only stop."""
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    n = 40
    rs = np.random.RandomState(3)
    X = np.column_stack((np.eye(n)[0], rs.randn(n) * .1))
    event_time = np.arange(1., n + 1.)
    model = RegressionModel((event_time, np.full(n, np.inf)),
                            HipDenseDesignMatrix(X, add_intercept=False),
                            'cox')
    risk = (model.n_event, model.risk_set_start_index,
            model.risk_set_end_index, model.n_appearance_in_risk_set)
    scale = np.ones(2)
    pp = np.full(2, 1e-8)
    f = co.precond_f(X, scale, pp, risk)
    q0 = np.array([400., 0.])
    p0 = np.array([200., .1])
    logp0, grad0 = f(q0)
    got, want = _run_traj(model, X, risk, 1., 10, tol=1e300,
                          inputs=(f, scale, pp, q0, p0, logp0, grad0))
    assert want[4] and want[2] == -np.inf and want[3] == 2
    _traj_check(got, want, 10)
