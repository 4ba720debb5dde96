"""GPU: the Cox model in counting-process form (csrc/cox_interval.hip on
csrc/hamiltonian.hpp) -- the likelihood, its gradient and Hessian matvec
against the NumPy oracle (tests/cox_interval_oracle.py) on three design types,
at the partition edges of the scans and on edge data; against the plain
CoxModel where no row enters late; under episode splitting; the empty
risk-set rule; the trajectory, No-U-Turn doublings and whole seeded chains
against the same host logic on the oracle; the refusals.  There is no
reference implementation of this likelihood: the oracle's extended-precision
form is the yardstick, and each comparison first checks on the CPU that the
oracle's own float64 two-scan form meets the tolerance it holds the device to.
"""
import warnings
from ctypes import byref, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_interval_oracle as cio
import cox_oracle as co
import logit_oracle as lo

pytestmark = pytest.mark.gpu

# tests/test_hip_cox.py's, for the same quantities against its oracle
LL_TOL, GRAD_TOL, HESS_TOL = 1e-11, 1e-11, 1e-10
RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance


def _matrix(kind, n, p, seed):
    from bayesbridge_amd import simulate
    rs = np.random.RandomState(seed)
    if kind == 'tiled_binary':
        return simulate.simulate_binary_csr_fast(n, p, .1, seed=seed)
    if kind == 'csr_valued':
        return sparse.random(n, p, density=.1, format='csr', random_state=rs)
    return rs.randn(n, p)


def _design(kind, X):
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if kind == 'tiled_binary':
        return HipSparseDesignMatrix(X, add_intercept=False, storage='tiled')
    if kind == 'csr_valued':
        return HipSparseDesignMatrix(X, add_intercept=False, storage='csr')
    return HipDenseDesignMatrix(X, add_intercept=False)


def _model(kind, entry, event, cens, X):
    """(device model on sorted rows, sorted X, the oracle's index arrays,
    sorted (entry, event, censoring))."""
    from bayesbridge_amd import RegressionModel
    from bayesbridge_amd.model import cox_preprocess_interval
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        entry, event, cens, X, _ = cox_preprocess_interval(entry, event, cens,
                                                           X)
    model = RegressionModel((event, cens), _design(kind, X), 'cox',
                            entry_time=entry)
    assert model.name == 'cox' and model._ham_prefix == 'bbx_coxcp_'
    idx = (model.n_event, model.event_row, model.risk_set_start_index,
           model.risk_set_entry_index, model.n_event_by_exit,
           model.n_event_by_entry, model.entry_order)
    return model, X, idx, (entry, event, cens)


def _problem(kind, n, p, seed=0, **kw):
    X = _matrix(kind, n, p, seed)
    return _model(kind, *cio.make_times(X, seed, **kw), X)


def _keep_every_row(entry, event, cens):
    """The same times with every row in some risk set, so that the row count
    is the one a case is about: a row censored before the first event is
    censored at it, and a censored row with no event while it is at risk is
    at risk from the start."""
    ev = np.sort(event[np.isfinite(event)])
    cens = np.where(np.isinf(event) & (cens < ev[0]), ev[0], cens)
    x = np.minimum(event, cens)
    at_risk = np.searchsorted(ev, x, side='right') \
        > np.searchsorted(ev, entry, side='right')
    return np.where(at_risk, entry, -np.inf), event, cens


def _within(got, want, tol, scale=None):
    scale = np.abs(want).max() if scale is None else scale
    return np.all(np.abs(np.asarray(got) - want) <= tol * scale)


def _check_against_oracle(model, X, idx, times, betas, vs, scales=False):
    """Device == oracle at the tolerances, after the CPU check that the
    oracle's float64 two-scan form is within them of its extended-precision
    form (explicit matrix up to 2049 rows, scans beyond); two calls give the
    same bits.  scales: the tolerances refer to the sizes of the summed terms
    (cio.term_scales), for data on which the results cancel to ~0."""
    n = X.shape[0]
    if n <= cio.EXPLICIT_MAX_N:
        mask, evrow = cio.risk_matrix(*times)
        assert np.array_equal(evrow, idx[1])
    for beta, v in zip(betas, vs):
        if n <= cio.EXPLICIT_MAX_N:
            oll, ograd = cio.explicit_loglik_grad(X, beta, mask, evrow)
            ohv = cio.explicit_hessian_matvec(X, beta, v, mask, evrow)
        else:
            oll, ograd = cio.scans_loglik_grad(X, beta, idx, np.longdouble)
            ohv = cio.scans_hessian_matvec(X, beta, v, idx, np.longdouble)
        assert np.isfinite(oll)
        sl, sg, sh = (abs(oll), None, None)
        if scales:
            sl, sg, sh = cio.term_scales(X, beta, v, idx)
            sg, sh = sg.max(), sh.max()
        fll, fgrad = cio.scans_loglik_grad(X, beta, idx)
        fhv = cio.scans_hessian_matvec(X, beta, v, idx)
        print('n', n, 'E/H up to %.3g' % cio.cancellation(X, beta, idx),
              'oracle f64 vs ext: ll %.2e grad %.2e hess %.2e' % (
                  abs(fll - oll) / (sl or 1.),
                  np.abs(fgrad - ograd).max() / (sg or np.abs(ograd).max()),
                  np.abs(fhv - ohv).max() / (sh or np.abs(ohv).max())))
        assert abs(fll - oll) <= LL_TOL * sl
        assert _within(fgrad, ograd, GRAD_TOL, sg)
        assert _within(fhv, ohv, HESS_TOL, sh)
        ll, grad = model.compute_loglik_and_gradient(beta)
        hv = model.get_hessian_matvec_operator(beta)(v)
        print('   device vs ext: ll %.2e grad %.2e hess %.2e' % (
            abs(ll - oll) / (sl or 1.),
            np.abs(grad - ograd).max() / (sg or np.abs(ograd).max()),
            np.abs(hv - ohv).max() / (sh or np.abs(ohv).max())))
        assert abs(ll - oll) <= LL_TOL * sl
        assert _within(grad, ograd, GRAD_TOL, sg)
        assert _within(hv, ohv, HESS_TOL, sh)
        ll2, grad2 = model.compute_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        assert np.array_equal(model.get_hessian_matvec_operator(beta)(v), hv)
        assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
            == (ll, None)
        assert model.hamiltonian_loglik_and_gradient(beta)[0] == ll


def _betas(p, seed=1, scales=(.1, 1.)):
    rs = np.random.RandomState(seed)
    return [rs.randn(p) * s for s in scales], [rs.randn(p) for _ in scales]


@pytest.mark.parametrize('kind', ['tiled_binary', 'csr_valued', 'dense64'])
def test_likelihood_gradient_hessian_match_the_oracle(kind):
    n, p = 2049, 40
    model, X, idx, times = _problem(kind, n, p, seed=3)
    assert np.isfinite(times[0]).sum() > n // 4       # real delayed entry
    assert np.sum(idx[3] < X.shape[0]) > idx[0] // 2  # most H_k subtract
    _check_against_oracle(model, X, idx, times, *_betas(p))


def test_tied_times_match_the_oracle():
    """Event times tied with each other, with censoring times (inside the
    risk set) and with entry times (outside it)."""
    model, X, idx, times = _problem('dense64', 700, 10, seed=4, ties=True)
    entry, event, cens = times
    ev = event[np.isfinite(event)]
    assert len(np.unique(ev)) < len(ev)
    assert np.intersect1d(ev, cens).size and np.intersect1d(ev, entry).size
    _check_against_oracle(model, X, idx, times, *_betas(10))


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257])
def test_partition_edges_of_the_scans(n, monkeypatch):
    """SCAN_G = 256 chunks per segment: empty chunks (n < 256) and one element
    per chunk; n = 1 is a single event (every result is exactly 0), n = 2 one
    event and one censored row."""
    from bayesbridge_amd import design_matrix
    # the columns of one or two rows can be "constant", and the design classes
    # drop constant columns as hand-made intercepts: keep them
    monkeypatch.setattr(design_matrix, 'remove_intercept_indicator',
                        lambda X: X)
    rs = np.random.RandomState(n)
    X = rs.randn(n, 3)
    if n <= 2:
        entry = np.array([-np.inf, .5])[:n]
        event = np.array([1., np.inf])[:n]
        cens = np.array([np.inf, 2.])[:n]
    else:
        entry, event, cens = _keep_every_row(
            *cio.make_times(X, n, censor_frac=.3))
    model, X, idx, times = _model('dense64', entry, event, cens, X)
    assert model.n_obs == n
    _check_against_oracle(model, X, idx, times, *_betas(3), scales=n == 1)
    if n == 1:
        beta = np.array([.3, -.2, .1])
        assert model.compute_loglik_and_gradient(beta)[0] == 0.
        assert not model.compute_loglik_and_gradient(beta)[1].any()


def test_a_chunk_that_crosses_a_tile():
    """524 289 rows: each of the 256 chunks holds 2049 elements, one more than
    a tile of SCAN_BLOCK x SCAN_E = 2048."""
    n, p = 524289, 8
    X = np.random.RandomState(7).randn(n, p)
    entry, event, cens = _keep_every_row(*cio.make_times(X, 7))
    model, X, idx, times = _model('dense64', entry, event, cens, X)
    assert model.n_obs == n and np.sum(idx[3] < n) > 1000
    betas, vs = _betas(p, scales=(.5,))
    _check_against_oracle(model, X, idx, times, betas, vs)


def _edge(case, n=300, p=4):
    rs = np.random.RandomState(11)
    X = rs.randn(n, p)
    x = np.cumsum(rs.uniform(.5, 1.5, n))          # distinct exit times
    if case == 'late_entry':
        # every row enters after the exit of the row before it: F is as large
        # as E, less one term, until the end.  (A censored row would be in no
        # risk set.)
        entry = np.concatenate(([-np.inf], (x[:-1] + x[1:]) / 2))
        cens = np.zeros(n, dtype=bool)
    elif case == 'late_entry_pairs':
        # ... after the exit of the row two before it: less two terms
        entry = np.concatenate(([-np.inf] * 2, (x[:-2] + x[1:-1]) / 2))
        cens = rs.rand(n) < .3
        cens[0] = False
    elif case == 'all_tied':
        x = np.where(rs.rand(n) < .5, 5., 5. + rs.rand(n))
        entry = np.where(rs.rand(n) < .5, 5. * rs.rand(n), -np.inf)
        cens = x > 5.
        cens[:20] = True               # some censored at the event time
    else:
        assert case == 'events_only'
        entry = np.where(rs.rand(n) < .6, x * rs.rand(n), -np.inf)
        cens = np.zeros(n, dtype=bool)
    event = np.where(cens, np.inf, x)
    censoring = np.where(cens, x, np.inf)
    return entry, event, censoring, X


@pytest.mark.parametrize('case', ['late_entry', 'late_entry_pairs',
                                  'all_tied', 'events_only'])
def test_edge_data(case):
    """late_entry: every risk set is a single row, so the likelihood is 0 for
    every beta and each result is a sum of terms that cancel: the tolerances
    there refer to the size of those terms (cio.term_scales)."""
    entry, event, cens, X = _edge(case)
    model, X, idx, times = _model('dense64', entry, event, cens, X)
    n = X.shape[0]
    if case == 'late_entry':
        assert np.all(idx[4] - idx[5] == 1) and model.n_event > 150
        # E - F leaves one term of many
        assert np.array_equal(idx[3][:-1] - idx[2][:-1],
                              np.ones(model.n_event - 1))
    if case == 'late_entry_pairs':
        assert np.max(idx[3] - idx[2]) == 2 and np.any(np.isinf(times[1]))
    if case == 'all_tied':
        assert model.n_event > 100
        assert len(np.unique(times[1][np.isfinite(times[1])])) == 1
        assert np.any(times[2] == 5.)
    if case == 'events_only':
        assert model.n_event == n == 300
    # E / H grows with the spread of eta where a risk set is one or two rows
    # of hundreds: coefficients at which the float64 oracle keeps the
    # tolerances
    _check_against_oracle(model, X, idx, times,
                          *_betas(X.shape[1], scales=(.05, .2)),
                          scales=case == 'late_entry')


def test_without_delayed_entry_it_is_the_plain_model():
    """entry = -inf everywhere: loglik, gradient and Hessian matvec of the
    plain CoxModel on the same rows (in its own order), at the tolerances."""
    from bayesbridge_amd import RegressionModel
    n, p = 3000, 30
    X = _matrix('dense64', n, p, 5)
    entry, event, cens = cio.make_times(X, 5, entry_frac=0.)
    assert np.all(entry == -np.inf)
    model, Xs, idx, times = _model('dense64', entry, event, cens, X)
    assert np.all(idx[3] == Xs.shape[0]) and np.all(idx[5] == 0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = RegressionModel((event, cens), X, 'cox')
    assert plain._ham_prefix == 'bbx_cox_' and plain.n_obs == model.n_obs
    for beta, v in zip(*_betas(p)):
        ll, grad = model.compute_loglik_and_gradient(beta)
        pll, pgrad = plain.compute_loglik_and_gradient(beta)
        hv = model.get_hessian_matvec_operator(beta)(v)
        phv = plain.get_hessian_matvec_operator(beta)(v)
        print('vs plain: ll %.2e grad %.2e hess %.2e' % (
            abs(ll - pll) / abs(pll),
            np.abs(grad - pgrad).max() / np.abs(pgrad).max(),
            np.abs(hv - phv).max() / np.abs(phv).max()))
        assert abs(ll - pll) <= LL_TOL * abs(pll)
        assert _within(grad, pgrad, GRAD_TOL)
        assert _within(hv, phv, HESS_TOL)
    _check_against_oracle(model, Xs, idx, times, *_betas(p))


def test_steep_hazards_without_delayed_entry_subtract_nothing():
    """The data of test_hip_cox.py's
    test_steep_hazards_keep_every_prefix_of_the_scans: relative hazards that
    fall by e^7 from one event to the next.  A risk-set sum formed as a
    difference from the total would be 0 or negative for the late events;
    without delayed entry nothing is subtracted, and loglik is finite."""
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    n = 96
    X = np.column_stack((-7. * np.arange(n),
                         np.random.RandomState(5).randn(n)))
    event_time = np.arange(1., n + 1.)
    censoring_time = np.full(n, np.inf)
    design = HipDenseDesignMatrix(X, add_intercept=False)
    model = RegressionModel((event_time, censoring_time), design, 'cox',
                            entry_time=np.full(n, -np.inf))
    plain = RegressionModel((event_time, censoring_time), design, 'cox')
    beta = np.array([1., .3])
    ll, grad = model.compute_loglik_and_gradient(beta)
    pll, pgrad = plain.compute_loglik_and_gradient(beta)
    assert np.isfinite(ll) and np.isfinite(pll)
    assert abs(ll - pll) <= LL_TOL * abs(pll)
    assert _within(grad, pgrad, 1e-10)       # test_hip_cox.py's, on this data
    v = np.array([.7, -1.1])
    hv = model.get_hessian_matvec_operator(beta)(v)
    phv = plain.get_hessian_matvec_operator(beta)(v)
    assert _within(hv, phv, 1e-9)


def test_episode_splitting_leaves_the_likelihood_unchanged():
    """Every row cut at a random interior time into two rows with the same
    covariates, the event on the second."""
    n, p = 1500, 12
    X = _matrix('dense64', n, p, 6)
    entry, event, cens = cio.make_times(X, 6)
    model, _, _, _ = _model('dense64', entry, event, cens, X)
    rs = np.random.RandomState(8)
    x = np.minimum(event, cens)
    lower = np.where(np.isfinite(entry), entry, 0.)
    cut = lower + (x - lower) * rs.uniform(.05, .95, n)
    assert np.all((entry < cut) & (cut < x))
    entry2 = np.concatenate((entry, cut))
    event2 = np.concatenate((np.full(n, np.inf), event))
    cens2 = np.concatenate((cut, cens))
    split, _, _, _ = _model('dense64', entry2, event2, cens2,
                            np.vstack((X, X)))
    assert split.n_event == model.n_event and split.n_obs > 1.5 * model.n_obs
    for beta, v in zip(*_betas(p)):
        ll, grad = model.compute_loglik_and_gradient(beta)
        sll, sgrad = split.compute_loglik_and_gradient(beta)
        hv = model.get_hessian_matvec_operator(beta)(v)
        shv = split.get_hessian_matvec_operator(beta)(v)
        print('split vs uncut: ll %.2e grad %.2e hess %.2e' % (
            abs(sll - ll) / abs(ll),
            np.abs(sgrad - grad).max() / np.abs(grad).max(),
            np.abs(shv - hv).max() / np.abs(hv).max()))
        assert abs(sll - ll) <= LL_TOL * abs(ll)
        assert _within(sgrad, grad, GRAD_TOL)
        assert _within(shv, hv, HESS_TOL)


def test_empty_risk_set_sum_gives_minus_infinity():
    model, X, idx, times = _problem('dense64', 2000, 20, seed=9)
    beta = np.zeros(20)
    beta[0] = 2000.       # exp(eta - max) underflows for most rows
    assert cio.scans_loglik_grad(X, beta, idx) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
        == (-np.inf, None)
    with pytest.raises(ValueError, match='Hessian operator'):
        model.get_hessian_matvec_operator(beta)
    # the flags were that evaluation's only
    ll = model.compute_loglik_and_gradient(beta * 0)[0]
    assert abs(ll - cio.scans_loglik_grad(X, beta * 0, idx)[0]) \
        <= LL_TOL * abs(ll)
    # a trajectory whose first step lands there reports instability
    P = 20
    scale, pp = np.ones(P), np.ones(P)
    f = cio.precond_f(X, scale, pp, idx)
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
    f = cio.precond_f(X, scale, prior_prec, idx)
    q0 = rs.randn(P) * .1
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_trajectory_matches_host_velocity_verlet(kind):
    model, X, idx, _ = _problem(kind, 2000, 60, seed=2)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(X, idx)
    want = lo.trajectory(f, .05, 25, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(.05, 25, scale, pp, q0, p0, logp0, grad0)
    assert not want[5] and not got['instability']
    assert got['n_steps'] == want[4] == 25
    np.testing.assert_allclose(got['q'], want[0], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got['p'], want[1], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got['grad'], want[3], rtol=1e-9, atol=1e-12)
    assert got['logp'] == pytest.approx(want[2], rel=1e-11)
    assert got['hamiltonian'][0] == pytest.approx(want[6], rel=1e-13)
    assert got['hamiltonian'][1] == pytest.approx(want[7], rel=1e-11)
    again = model.hmc_trajectory(.05, 25, scale, pp, q0, p0, logp0, grad0)
    for key in ('q', 'p', 'grad', 'hamiltonian'):
        assert np.array_equal(again[key], got[key])


def test_trajectory_stops_where_the_host_loop_stops():
    """A step size far past the stability limit: the integrator diverges and
    the device stops at the host loop's step."""
    model, X, idx, _ = _problem('dense64', 2000, 60, seed=2)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(X, idx)
    with np.errstate(all='ignore'):
        want = lo.trajectory(f, 3., 200, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(3., 200, scale, pp, q0, p0, logp0, grad0)
    assert want[5] and got['instability']
    assert got['n_steps'] == want[4] < 200


def _stability_limit(X, idx, scale, pp, q0):
    """2 / sqrt(largest curvature of -f at q0), by power iteration on the
    oracle's Hessian."""
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * cio.scans_hessian_matvec(X, q0 * scale,
                                                       scale * v, idx)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


def _compare_doublings(model, oracle, scale, pp, q0, p0, logp0, grad0, dt,
                       directions, tol, seed):
    """The same doublings on the device and on the oracle, with the same
    uniforms: integers exact, states at the Hamiltonian tolerance."""
    joint = logp0 - .5 * np.dot(p0, p0)
    rs = np.random.RandomState(seed)
    for m in (model, oracle):
        m.nuts_begin(scale, pp, q0, p0, logp0, grad0, joint, joint - 1., tol)
    outs = []
    for height, direction in enumerate(directions):
        uniforms = rs.rand(2 ** height)
        with np.errstate(all='ignore'):
            want = oracle.nuts_doubling(dt, direction, height, uniforms)
        got = model.nuts_doubling(dt, direction, height, uniforms)
        print('height', height, 'dir', direction, got)
        for key in want:
            if isinstance(want[key], float):
                np.testing.assert_allclose(got[key], want[key], rtol=RTOL,
                                           atol=ATOL, err_msg=key)
            else:
                assert got[key] == want[key], (key, got, want)
        q, logp, grad = model.nuts_sample()
        wq, wlogp, wgrad = oracle.nuts_sample()
        np.testing.assert_allclose(q, wq, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(logp, wlogp, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(grad, wgrad, rtol=RTOL, atol=ATOL)
        outs.append(got)
        if got['u_turn_detected'] or got['instability_detected']:
            break
    return outs


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_nuts_doublings_match_the_oracle(kind):
    model, X, idx, _ = _problem(kind, 1000, 20, seed=12)
    oracle = cio.OracleModel(X, idx)
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
CHAIN_N, CHAIN_P = 300, 10
# A chain multiplies a rounding difference from iteration to iteration.  The
# seeds are ones at which the oracle's own chain, run again with its
# likelihood and gradient perturbed by 1e-15 relative (a few ulp: what another
# summation order and another exp differ by), agrees with itself to 1e-8 or
# better, three perturbations out of three: the best of seeds 0-23 on the
# CPU, the device not involved ('hmc' sparse 9e-10, dense 8e-9; 'nuts' 2e-10
# and 4e-10).
CHAIN_SEED = {('hmc', 'sparse'): 0, ('hmc', 'dense'): 15,
              ('nuts', 'sparse'): 12, ('nuts', 'dense'): 16}


def chain_problem(fmt):
    rs = np.random.RandomState(13)
    if fmt == 'sparse':
        X = sparse.random(CHAIN_N, CHAIN_P, density=.3, format='csr',
                          random_state=rs)
        X.data[:] = 1.
    else:
        X = rs.randn(CHAIN_N, CHAIN_P) * .5
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    entry, event, cens = cio.make_times(dense, 13)
    return entry, event, cens, X


def chain_sorted(fmt):
    """(sorted entry, event, censoring, X, index arrays, the maximum
    partial-likelihood coefficients): the chain starts there, so it has no
    long transient trajectories and no mode search runs."""
    from bayesbridge_amd.model import (cox_interval_risk_sets,
                                       cox_preprocess_interval)
    entry, event, cens, X = chain_problem(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        entry, event, cens, X, _ = cox_preprocess_interval(entry, event, cens,
                                                           X)
    idx = cox_interval_risk_sets(entry, event, cens)
    dense = np.asarray(X.todense()) if fmt == 'sparse' else X
    return entry, event, cens, X, idx, cio.newton_mle(dense, idx)


def run_chain(model, method, seed, start, n_iter=12, resume=None):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    prior = RegressionCoefPrior(bridge_exponent=.5, regularizing_slab_size=1.)
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


def _chain(fmt, method, seed, oracle=False, n_iter=12, resume=None):
    from bayesbridge_amd import RegressionModel
    entry, event, cens, X = chain_problem(fmt)
    _, _, _, Xs, idx, start = chain_sorted(fmt)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', entry_time=entry)
    assert model._ham_prefix == 'bbx_coxcp_' and not model.intercept_added
    if oracle:
        model = cio.OracleModel(Xs, idx, design=model.design)
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
    entry, event, cens, X = chain_problem('dense')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((event, cens), X, 'cox', entry_time=entry,
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
def test_refusals_are_exceptions():
    from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,
                                 RegressionModel)
    from bayesbridge_amd.model import CoxModel
    entry, event, cens, X = chain_problem('dense')
    n = len(event)
    strata = np.arange(n) % 2
    with pytest.raises(ValueError, match='strata'):
        RegressionModel((event, cens, strata), X, 'cox', entry_time=entry)
    se, st, sc, sX, idx, _ = chain_sorted('dense')
    design = HipDenseDesignMatrix(sX, add_intercept=False)
    with pytest.raises(ValueError, match='strata'):
        CoxModel(st, sc, design, strata=np.zeros(len(st)), entry_time=se)
    for family, outcome in (('linear', event), ('logit', np.ones(n)),
                            ('poisson', np.ones(n))):
        with pytest.raises(ValueError, match="family='cox' only"):
            RegressionModel(outcome, X, family, entry_time=entry)
    # a prebuilt design must be in the model's order, without an intercept
    with pytest.raises(ValueError, match='order'):
        RegressionModel((event, cens), HipDenseDesignMatrix(
            X, add_intercept=False), 'cox', entry_time=entry)
    with pytest.raises(ValueError, match='intercept'):
        RegressionModel((st, sc), HipDenseDesignMatrix(sX), 'cox',
                        entry_time=se)
    with pytest.raises(ValueError, match='strictly before'):
        RegressionModel((st, sc), design, 'cox',
                        entry_time=np.where(np.arange(len(st)) == 3, np.inf,
                                            se))
    model = RegressionModel((st, sc), design, 'cox', entry_time=se)
    bridge = BayesBridge(model)
    with pytest.raises(ValueError):
        bridge.gibbs(1, options={'rng': 'device'})
    with pytest.raises(ValueError):
        bridge.gibbs_batch([0, 1], 1)
    with pytest.raises(ValueError):
        bridge.gibbs_multichain(2, 1)
    with pytest.warns(UserWarning, match='Will use HMC instead'):
        _, info = bridge.gibbs(1, seed=0, coef_sampler_type='cg',
                               init={'coef': np.zeros(CHAIN_P),
                                     'global_scale': .1})
    assert info['coef_sampler_type'] == 'hmc'     # as the plain Cox model
    with pytest.raises(ValueError):
        model.compute_loglik_and_gradient(np.zeros(CHAIN_P + 1))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def test_create_refuses_bad_index_arrays_with_a_message():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    se, st, sc, sX, idx, _ = chain_sorted('dense')
    n, ne = len(st), idx[0]
    design = HipDenseDesignMatrix(sX, add_intercept=False)
    names = ('evrow', 'a', 'b', 'p', 'q', 'entry_perm')
    good = dict(zip(names, (np.ascontiguousarray(v, dtype=np.int32)
                            for v in idx[1:])))

    def create(n_event=ne, out=True, dsn=design.handle, **over):
        arrays = dict(good)
        arrays.update(over)
        h = c_void_p()
        st_ = lib.bbx_coxcp_create(dsn, n_event,
                                   *[_ptr(arrays[k]) for k in names],
                                   byref(h) if out else None)
        return st_, h, _lib.last_error()

    def changed(name, at, value):
        v = good[name].copy()
        v[at] = value
        return {name: v}

    status, h, _ = create()
    assert status == 0 and h.value
    assert lib.bbx_coxcp_destroy(h) == 0
    assert create(out=False)[::2] == (-1, 'NULL output pointer')
    assert create(dsn=None)[::2] == (-1, 'invalid design')
    for name in names:
        status, h, msg = create(**{name: None})
        assert status == -1 and not h.value and msg == 'NULL index array'
    for bad in (0, -1, n + 1):
        assert create(n_event=bad)[::2] == (-1, 'n_event must be in [1, n]')
    k, last = ne // 2, ne - 1
    swapped = good['entry_perm'].copy()
    swapped[5] = swapped[6]
    perm = good['entry_perm']
    assert good['a'][last - 1] >= 1 and good['b'][last - 1] >= 1
    assert good['p'][n - 2] >= 2 and good['q'][perm[n - 2]] > 0
    cases = [
        (changed('evrow', k, n), 'evrow[%d] outside [0, n)' % k),
        (changed('evrow', k, -1), 'evrow[%d] outside [0, n)' % k),
        (changed('evrow', k, good['evrow'][k - 1]),
         'evrow[%d] is not increasing' % k),
        (changed('a', k, -1), 'a[%d] outside [0, evrow[k]]' % k),
        (changed('a', k, good['evrow'][k] + 1),
         'a[%d] outside [0, evrow[k]]' % k),
        (changed('a', last, good['a'][last - 1] - 1),
         'a[%d] is decreasing' % last),
        (changed('b', k, n + 1), 'b[%d] outside [0, n]' % k),
        (changed('b', k, -1), 'b[%d] outside [0, n]' % k),
        (changed('b', last, good['b'][last - 1] - 1),
         'b[%d] is decreasing' % last),
        (changed('b', 0, good['a'][0]), 'risk set 0 is empty'),
        ({'entry_perm': swapped}, 'entry_perm is not a permutation'),
        (changed('entry_perm', 7, n), 'entry_perm is not a permutation'),
        (changed('entry_perm', 7, -1), 'entry_perm is not a permutation'),
        (changed('p', 3, 0), 'p[3] outside [1, n_event]'),
        (changed('p', 3, ne + 1), 'p[3] outside [1, n_event]'),
        (changed('p', n - 1, good['p'][n - 2] - 1),
         'p[%d] is decreasing' % (n - 1)),
        (changed('q', 3, -1), 'q[3] outside [0, p[i])'),
        (changed('q', 3, good['p'][3]), 'q[3] outside [0, p[i])'),
        # in range, but out of step with the entry order
        (changed('q', perm[n - 1], 0),
         'q[entry_perm[%d]] is decreasing in entry order' % (n - 1)),
    ]
    for over, text in cases:
        status, h, msg = create(**over)
        print(text, '->', msg)
        assert status == -1 and not h.value
        assert text in msg, (text, msg)
    # the handle made from the good arrays still computes
    status, h, _ = create()
    assert status == 0
    assert lib.bbx_coxcp_destroy(h) == 0
