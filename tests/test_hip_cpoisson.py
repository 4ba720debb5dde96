"""GPU: the conditional Poisson model (csrc/cpoisson.hip on
csrc/hamiltonian.hpp) -- the likelihood, its gradient and Hessian matvec
against the NumPy oracle (tests/cpoisson_oracle.py) on stratum layouts that
reach every seam of the segmented log-sum-exp passes, against the stratified
Cox handle where the two likelihoods coincide, the per-stratum shift, the
launch count, the trajectory against a host velocity Verlet, No-U-Turn
doublings against tests/nuts_oracle.py, whole seeded chains against the same
driver on the oracle model, the refusals and one statistical check.  There is
no reference implementation of this family: the oracle is the yardstick
throughout (tests/test_cpoisson_host_logic.py pins it on the CPU).

The passes cut the row range [0, n) into G = CP_G chunks of C = ceil(n / G)
rows, scanned in tiles of T = CP_TILE rows."""
import os
import re
import warnings
from ctypes import byref, c_double, c_int, c_uint64, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cpoisson_oracle as cpo
import logit_oracle as lo
from conftest import ROOT

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance
ERR_INVALID, ERR_STATE = -1, -5


def _constant(name, src='cpoisson.hip'):
    text = open(os.path.join(ROOT, 'bayes-bridge_amd', 'csrc', src)).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))


G, T = _constant('CP_G'), _constant('CP_TILE')
EDGE_SIZES = [2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1]


def _chunk(n):
    return -(-n // G)


def _seam_sizes(n=None):
    """Stratum sizes for n = G * 274 rows (C = 274): two shuffled rounds of
    EDGE_SIZES, a filler that ends on a chunk edge, a run of strata of 2 to 3
    rows, one stratum over ~73 chunks, another run of tiny ones, and a last
    stratum that ends the rows."""
    n = G * 274 if n is None else n
    C = _chunk(n)
    assert C * G == n
    rs = np.random.RandomState(11)
    sizes = [int(s) for s in rs.permutation(EDGE_SIZES * 2)]
    sizes.append(-int(np.sum(sizes)) % C + C)        # next boundary: C * j
    assert int(np.sum(sizes)) % C == 0
    sizes += [int(s) for s in rs.randint(2, 4, 300)] + [20000] \
        + [int(s) for s in rs.randint(2, 4, 300)]
    sizes.append(n - int(np.sum(sizes)))
    assert sizes[-1] > T
    return sizes


def _tile_sizes():
    """n = G * 2344: chunks of two tiles.  The first boundary on a tile edge
    inside chunk 0 (row T), strata of T - 1 and T + 1 rows, later boundaries
    on chunk edges (2344 = 8 * 293)."""
    C = T + 296
    n = G * C
    sizes = [T, C - T, T - 1, T + 1, 2 * C - 2 * T]
    rest = n - int(np.sum(sizes))
    assert rest % 293 == 0 and C % 293 == 0
    return sizes + [293] * (rest // 293)


LAYOUTS = {
    'pairs': lambda: [2] * 3000,
    'seams': _seam_sizes,
    'one': lambda: [6000],
    'tiles': _tile_sizes,
    'small': lambda: [2, 3, 7, 63, 64, 65, 255, 256, 257, 40, 2, 900],
}


def _device_design(kind, X, center):
    """A device design without an intercept column on rows already in order,
    and the oracle's design tuple."""
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if kind in ('dense64', 'dense32'):
        dtype = 'float32' if kind == 'dense32' else 'float64'
        dsn = HipDenseDesignMatrix(X, add_intercept=False,
                                   center_predictor=center,
                                   storage_dtype=dtype)
        if kind == 'dense32':
            # float32 storage holds the CENTRED entries rounded to float32
            if center:
                X = X - dsn.column_offset
            X = X.astype(np.float32).astype(np.float64)
            return dsn, lo.design(X, False, False)
    else:
        storage = 'csr' if kind == 'csr_valued' else 'tiled'
        X = sparse.csr_matrix(X)
        dsn = HipSparseDesignMatrix(X, add_intercept=False,
                                    center_predictor=center, storage=storage)
    assert dsn.shape == X.shape and not dsn.intercept_added
    return dsn, lo.design(X, center, False,
                          offset=dsn.column_offset if center else None)


def _values(kind, n, p, seed):
    rs = np.random.RandomState(seed + 100)
    if kind in ('dense64', 'dense32'):
        return rs.randn(n, p)
    mask = (rs.rand(n, p) < .3) * 1.
    if kind == 'tiled_binary':
        return mask
    X = mask * rs.randn(n, p)
    if kind == 'mixed':
        X[:, :p // 2] = mask[:, :p // 2]
    return X


def _counts(rs, sptr, rate):
    """Counts with a positive total in every stratum."""
    y = rs.poisson(rate).astype(np.float64)
    total = np.add.reduceat(y, sptr[:-1])
    y[sptr[:-1][total == 0]] = 1.
    return y


def _outcome(D, sizes, exposure, seed):
    """Counts simulated with a baseline rate per stratum, the exposure
    (or None), the labels and the stratum pointer."""
    sptr = cpo.stratum_ptr_of(sizes)
    n = int(sptr[-1])
    rs = np.random.RandomState(seed + 1)
    e = rs.uniform(.5, 2., n) if exposure else None
    alpha = np.repeat(rs.randn(len(sizes)) * 2., sizes)
    beta = rs.randn(D[0].shape[1]) * .3
    rate = np.exp(np.clip(alpha, -3., 3.) + lo.dot(D, beta))
    y = _counts(rs, sptr, rate * (e if exposure else 1.))
    return y, e, np.repeat(np.arange(len(sizes)), sizes), sptr


def _data(kind, sizes, p, exposure=True, center=True, seed=0):
    """A device model, the oracle's design, the counts, the offset and the
    stratum pointer."""
    from bayesbridge_amd import RegressionModel
    n = int(np.sum(sizes))
    dsn, D = _device_design(kind, _values(kind, n, p, seed), center)
    y, e, lab, sptr = _outcome(D, sizes, exposure, seed)
    model = RegressionModel((y, e, lab), dsn, 'poisson')
    assert model.name == 'poisson' and model.design is dsn
    assert model._ham_prefix == 'bbx_cpoisson_'
    assert np.array_equal(model.stratum_ptr, sptr)
    return model, D, y, (np.log(e) if exposure else np.zeros(n)), sptr


def _check(model, D, y, o, sptr, scales=(.3, 2.)):
    """loglik, gradient, loglik_only, the Hessian matvec after set_location
    and bitwise repeats, at two scales of beta."""
    P = model.n_pred
    rs = np.random.RandomState(1)
    for scale in scales:
        beta, v = rs.randn(P) * scale, rs.randn(P)
        ll, grad = model.compute_loglik_and_gradient(beta)
        oll, ograd = cpo.loglik_grad(D, y, o, sptr, beta)
        print('beta scale', scale, 'loglik', ll, oll,
              'grad max|d| %.2e of %.3g' % (np.abs(grad - ograd).max(),
                                            np.abs(ograd).max()))
        assert np.isfinite(oll) and oll <= 0.
        np.testing.assert_allclose(ll, oll, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(grad, ograd, rtol=RTOL, atol=ATOL)
        ll2, grad2 = model.compute_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        hv = model.get_hessian_matvec_operator(beta)(v)
        ohv = cpo.hessian_matvec(D, y, o, sptr, beta, v)
        print('   hessian max|d| %.2e of %.3g' % (np.abs(hv - ohv).max(),
                                                  np.abs(ohv).max()))
        np.testing.assert_allclose(hv, ohv, rtol=RTOL, atol=ATOL)
        hv2 = model.get_hessian_matvec_operator(beta)(v)
        assert np.array_equal(hv2, hv)
    ll, none = model.compute_loglik_and_gradient(beta, loglik_only=True)
    assert none is None and ll == ll2
    assert model.hamiltonian_loglik_and_gradient(beta)[0] == ll2


def test_layouts_reach_the_seams_they_claim():
    sizes = LAYOUTS['seams']()
    n = int(np.sum(sizes))
    C = _chunk(n)
    assert n == G * 274 and C == 274 and min(sizes) >= 2
    bounds = np.cumsum(sizes)
    assert bounds[-1] == n                       # the last stratum ends the rows
    assert np.sum(bounds[:-1] % C == 0) >= 1     # a boundary on a chunk edge
    assert set(EDGE_SIZES) <= set(sizes)
    big = sizes.index(20000)
    assert 20000 > 70 * C                        # one stratum over many chunks
    assert max(sizes[big - 300:big]) <= 3 and max(sizes[big + 1:big + 301]) <= 3
    # strata inside one chunk, across one edge and the tile-sized ones across
    # several
    start = bounds - np.asarray(sizes)
    crossed = (bounds - 1) // C - start // C
    assert (crossed == 0).any() and (crossed == 1).any() and (crossed > 5).any()
    sizes = LAYOUTS['tiles']()
    n = int(np.sum(sizes))
    C = _chunk(n)
    assert C * G == n and T < C <= 2 * T         # every chunk runs two tiles
    bounds = np.cumsum(sizes)
    assert bounds[0] == T and np.sum(bounds[:-1] % C == 0) > 100
    assert {T - 1, T, T + 1} <= set(sizes)
    # 'pairs' and 'one' leave the last chunks empty: 6000 rows, C = 24
    assert _chunk(6000) * 250 == 6000


@pytest.mark.parametrize('exposure', [True, False])
@pytest.mark.parametrize('shape', ['pairs', 'seams', 'one'])
@pytest.mark.parametrize('kind', ['dense64', 'tiled_binary'])
def test_likelihood_gradient_hessian_match_the_oracle(kind, shape, exposure):
    args = _data(kind, LAYOUTS[shape](), 6, exposure=exposure,
                 seed=len(shape) + exposure)
    assert (args[3] != 0).any() == exposure
    _check(*args)


def test_chunks_of_two_tiles():
    """n = 600 064: every chunk of the passes runs two tiles, stratum
    boundaries on a tile edge and on chunk edges -- the carry from tile to
    tile, which no smaller n reaches."""
    _check(*_data('dense64', LAYOUTS['tiles'](), 3, seed=5), scales=(.3,))


@pytest.mark.parametrize('center', [True, False])
@pytest.mark.parametrize('kind', ['csr_valued', 'dense32', 'mixed'])
def test_other_designs(kind, center):
    _check(*_data(kind, LAYOUTS['small'](), 10, center=center, seed=3))


@pytest.mark.parametrize('shape', ['matched', 'seams'])
def test_agrees_with_the_stratified_cox_handle(shape):
    """One case per stratum, unit exposure: the conditional likelihood of the
    case's row is the stratified Cox partial likelihood of an event at time 1
    whose risk set is its whole stratum (the others censored at time 2)."""
    from bayesbridge_amd import RegressionModel
    if shape == 'matched':
        sizes = [int(s) for s in
                 np.random.RandomState(0).randint(2, 10, 800)]
        assert set(sizes) == set(range(2, 10))
    else:
        sizes = LAYOUTS['seams']()
    sptr = cpo.stratum_ptr_of(sizes)
    n, p = int(sptr[-1]), 6
    dsn, D = _device_design('dense64', _values('dense64', n, p, 7), False)
    y = np.zeros(n)
    y[sptr[:-1]] = 1.                            # the case: first in its stratum
    lab = np.repeat(np.arange(len(sizes)), sizes)
    et = np.where(y == 1., 1., np.inf)
    ct = np.where(y == 1., np.inf, 2.)
    model = RegressionModel((y, None, lab), dsn, 'poisson')
    cox = RegressionModel((et, ct, lab), dsn, 'cox')
    assert cox.strata is not None and cox.design is model.design
    rs = np.random.RandomState(2)
    for scale in (.3, 2.):
        beta, v = rs.randn(p) * scale, rs.randn(p)
        ll, grad = model.compute_loglik_and_gradient(beta)
        cl, cgrad = cox.compute_loglik_and_gradient(beta)
        print('loglik', ll, cl, 'grad max|d| %.2e'
              % np.abs(grad - cgrad).max())
        np.testing.assert_allclose(ll, cl, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(grad, cgrad, rtol=RTOL, atol=ATOL)
        hv = model.get_hessian_matvec_operator(beta)(v)
        ch = cox.get_hessian_matvec_operator(beta)(v)
        np.testing.assert_allclose(hv, ch, rtol=RTOL, atol=ATOL)
        oll, ograd = cpo.loglik_grad(D, y, np.zeros(n), sptr, beta)
        np.testing.assert_allclose(ll, oll, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(grad, ograd, rtol=RTOL, atol=ATOL)


def test_the_shift_is_per_stratum():
    """Two strata whose eta differ by 800 through an indicator column and a
    third whose own eta spreads over 900: finite, equal to the oracle -- and
    not finite under a likelihood with one global max, which sees every exp
    of the lower strata as 0."""
    from bayesbridge_amd import RegressionModel
    sizes = [300, 500, 200]
    sptr = cpo.stratum_ptr_of(sizes)
    n = int(sptr[-1])
    lab = np.repeat(np.arange(3), sizes)
    rs = np.random.RandomState(6)
    spread = np.where(lab == 2, rs.rand(n), 0.)
    spread[sptr[2]], spread[sptr[3] - 1] = 0., 1.
    X = np.column_stack((rs.randn(n, 3), (lab == 1) * 1., spread))
    dsn, D = _device_design('dense64', X, False)
    y = _counts(rs, sptr, np.full(n, 1.5))
    e = rs.uniform(.5, 2., n)
    o = np.log(e)
    model = RegressionModel((y, e, lab), dsn, 'poisson')
    beta = np.array([.3, -.5, .2, 800., 900.])
    eta = lo.dot(D, beta)
    assert eta[lab == 1].min() - eta[lab == 0].max() > 780
    assert np.ptp(eta[lab == 2]) > 800
    ll, grad = model.compute_loglik_and_gradient(beta)
    oll, ograd = cpo.loglik_grad(D, y, o, sptr, beta)
    assert np.isfinite(ll) and np.isfinite(oll) and np.all(np.isfinite(grad))
    np.testing.assert_allclose(ll, oll, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, ograd, rtol=RTOL, atol=ATOL)
    mutant = cpo.loglik_grad_global_max(D, y, o, sptr, beta)
    print('device', ll, 'oracle', oll, 'global-max mutant', mutant[0])
    assert not np.isfinite(mutant[0]) or abs(mutant[0] - ll) > 1e3 * abs(ll)
    v = rs.randn(5)
    hv = model.get_hessian_matvec_operator(beta)(v)
    assert np.all(np.isfinite(hv))
    np.testing.assert_allclose(
        hv, cpo.hessian_matvec(D, y, o, sptr, beta, v), rtol=RTOL, atol=ATOL)
    # a NaN comes out as a NaN, and the next evaluation is clean
    bad = beta * .001
    bad[1] = np.nan
    assert np.isnan(model.compute_loglik_and_gradient(bad)[0])
    ll2, grad2 = model.compute_loglik_and_gradient(beta)
    assert ll2 == ll and np.array_equal(grad2, grad)


def _launches(model, beta):
    from bayesbridge_amd import _lib
    lib = _lib.load()
    lib.bbx_launch_count.restype = c_uint64
    before = lib.bbx_launch_count()
    model.compute_loglik_and_gradient(beta)
    return lib.bbx_launch_count() - before


def test_launch_count_does_not_depend_on_the_strata():
    many = _data('dense64', LAYOUTS['pairs'](), 6)[0]
    one = _data('dense64', LAYOUTS['one'](), 6)[0]
    beta = np.random.RandomState(1).randn(6) * .3
    a, b = _launches(many, beta), _launches(one, beta)
    assert a == b > 0, (a, b)
    assert _launches(many, beta) == a


# ------------------------------------------------------------- trajectories
def _traj_inputs(D, y, o, sptr, seed=0):
    """f of the preconditioned coordinates and a start next to the maximum of
    the likelihood (test_hip_poisson._traj_inputs)."""
    P = D[0].shape[1]
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    prior_prec = np.ones(P)
    f = cpo.precond_f(D, y, o, sptr, scale, prior_prec)
    q0 = cpo.newton_mle(D, y, o, sptr)[0] / scale + rs.randn(P) * .02
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


def _stability_limit(D, y, o, sptr, scale, pp, q0):
    """2 / sqrt(largest curvature of -f at q0), by power iteration on the
    oracle's Hessian."""
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * cpo.hessian_matvec(D, y, o, sptr, q0 * scale,
                                                 scale * v)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


TRAJ_SIZES = [2, 3, 7, 63, 64, 65, 255, 256, 257, 40, 2, 100]


@pytest.fixture(scope='module', params=['tiled_binary', 'dense64'])
def traj(request):
    model, D, y, o, sptr = _data(request.param, TRAJ_SIZES, 10, seed=4)
    inputs = _traj_inputs(D, y, o, sptr)
    limit = _stability_limit(D, y, o, sptr, inputs[1], inputs[2], inputs[3])
    return model, cpo.OracleModel(D, y, o, sptr), inputs, limit


@pytest.mark.parametrize('n_step', [0, 1, 25])
def test_trajectory_matches_host_velocity_verlet(traj, n_step):
    model, _, (f, scale, pp, q0, p0, logp0, grad0), limit = traj
    dt = limit / 4
    want = lo.trajectory(f, dt, n_step, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(dt, n_step, scale, pp, q0, p0, logp0, grad0)
    assert not want[5] and not got['instability']
    assert got['n_steps'] == want[4] == n_step
    for key, ref in (('q', want[0]), ('p', want[1]), ('grad', want[3])):
        np.testing.assert_allclose(got[key], ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['logp'], want[2], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['hamiltonian'], [want[6], want[7]],
                               rtol=RTOL, atol=ATOL)
    again = model.hmc_trajectory(dt, n_step, scale, pp, q0, p0, logp0, grad0)
    for key in ('q', 'p', 'grad', 'hamiltonian'):
        assert np.array_equal(again[key], got[key])
    assert again['logp'] == got['logp']


def test_trajectory_stops_where_the_host_stops(traj):
    """A tolerance on the Hamiltonian's range that the steps of the stable
    trajectory exceed after a few of them (the oracle stops at step 2 on the
    binary design and at step 4 on the dense one): both stop at the same
    step, and the next evaluation is clean."""
    model, _, (f, scale, pp, q0, p0, logp0, grad0), limit = traj
    tol = .3
    want = lo.trajectory(f, limit / 4, 200, q0, p0, logp0, grad0, tol=tol)
    got = model.hmc_trajectory(limit / 4, 200, scale, pp, q0, p0, logp0,
                               grad0, tol)
    print('small tol: steps', got['n_steps'], want[4])
    assert want[5] and 2 <= want[4] < 200 and np.isfinite(want[2])
    assert got['instability'] and got['n_steps'] == want[4]
    np.testing.assert_allclose(got['q'], want[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got['p'], want[1], rtol=RTOL, atol=ATOL)
    ll, grad = model.compute_loglik_and_gradient(q0 * scale)
    np.testing.assert_allclose(ll + np.sum(-pp * q0 ** 2) / 2, logp0,
                               rtol=RTOL, atol=ATOL)


def _compare_doublings(model, oracle, scale, pp, q0, p0, logp0, grad0, dt,
                       directions, tol, seed):
    """The same doublings on the device and on the oracle, with the same
    uniforms; returns the device's outputs (test_hip_poisson's)."""
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


def test_nuts_doublings_match_the_oracle(traj):
    model, oracle, (f, scale, pp, q0, p0, logp0, grad0), limit = traj
    args = (model, oracle, scale, pp, q0, p0, logp0, grad0)
    # every height up to 4 in both directions: a step small enough for the
    # 31 steps to make no U-turn
    for first in (1, -1):
        directions = [first * (-1) ** h for h in range(5)]
        outs = _compare_doublings(*args, limit / 40, directions, 100., 5)
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
    # the flags were the doubling's only
    beta = q0 * scale
    np.testing.assert_allclose(
        model.compute_loglik_and_gradient(beta)[0],
        oracle.compute_loglik_and_gradient(beta)[0], rtol=RTOL)


# ------------------------------------------------------------ whole chains
CHAIN_STRATA, CHAIN_P = 60, 12
# The rule written above CHAIN_SEED in test_hip_poisson.py: the seeds are
# ones at which the oracle's own chain, run again with its likelihood and
# gradient perturbed by 1e-15 relative (random signs), agrees with itself to
# 1e-7 or better, three times out of three.  Searched on the CPU on the oracle
# model alone, from seed 0 upwards; the worst relative difference of the three
# runs over coef, logp and the scales: 'hmc' dense 4.5e-8 at seed 15 (seeds
# 0-14: 2.2e-7 to 1.8e-2), 'hmc' sparse 3.5e-8 at seed 8 (seeds 0-7: 6.7e-7
# to 3.5e-2), 'nuts' dense 1.9e-9 and sparse 4.8e-9 at seed 0.
CHAIN_SEED = {('hmc', 'sparse'): 8, ('hmc', 'dense'): 15,
              ('nuts', 'sparse'): 0, ('nuts', 'dense'): 0}


def _chain_problem(fmt):
    """About 300 rows in 60 strata of 3 to 7, p = 12."""
    rs = np.random.RandomState(11)
    sizes = rs.randint(3, 8, CHAIN_STRATA)
    sptr = cpo.stratum_ptr_of(sizes)
    n = int(sptr[-1])
    if fmt == 'sparse':
        X = sparse.random(n, CHAIN_P, density=.3, format='csr',
                          random_state=rs)
        X.data[:] = 1.
    else:
        X = rs.randn(n, CHAIN_P) * .5
    beta = np.zeros(CHAIN_P)
    beta[:4] = (.8, -.6, .4, -.3)
    e = rs.uniform(.5, 2., n)
    alpha = np.repeat(rs.randn(CHAIN_STRATA), sizes)
    y = _counts(rs, sptr, e * np.exp(alpha + np.asarray(X.dot(beta)).ravel()))
    return X, y, e, np.repeat(np.arange(CHAIN_STRATA), sizes), sptr


def _chain_start(fmt):
    """The conditional maximum-likelihood coefficients (Newton iterations on
    the oracle): a chain started there has no long transient trajectories."""
    X, y, e, lab, sptr = _chain_problem(fmt)
    return cpo.newton_mle(lo.design(X, True, False), y, np.log(e), sptr)[0]


def _chain(fmt, method, seed, oracle=False, n_iter=12, resume=None,
           design=None, wrap=None):
    """`n_iter` Gibbs iterations on the device model, or on the oracle model
    behind the same design object (`design`: a stand-in for it, for runs
    without a device; `wrap`: applied to the oracle model).  The chain starts
    at given coefficients, so no mode search runs."""
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, y, e, lab, sptr = _chain_problem(fmt)
    if design is None:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = RegressionModel((y, e, lab), X, 'poisson')
        # nothing was sorted or dropped
        assert np.array_equal(model.y, y) and not model.intercept_added
        design = model.design
        offset = design.column_offset
    else:
        offset = None
    if oracle:
        D = lo.design(X, True, False, offset=offset)
        model = cpo.OracleModel(D, y, np.log(e), sptr, design=design)
        if wrap:
            model = wrap(model)
    prior = RegressionCoefPrior(bridge_exponent=.5,
                                regularizing_slab_size=1.)
    init = {'coef': _chain_start(fmt), 'global_scale': .1}
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
    """No sampler named: 'hmc'; no coefficients given: the L-BFGS-B mode
    search runs on the device likelihood, without obs_prec or intercept."""
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, y, e, lab, sptr = _chain_problem('dense')
    model = RegressionModel((y, e, lab), X, 'poisson')
    assert not model.intercept_added and model.n_pred == CHAIN_P
    D = lo.design(X, True, False, offset=model.design.column_offset)
    prior = RegressionCoefPrior(bridge_exponent=.5,
                                regularizing_slab_size=1.)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        samples, info = BayesBridge(model, prior).gibbs(
            3, init={'global_scale': .1}, seed=1)
    assert info['coef_sampler_type'] == 'hmc'
    assert info['options']['rng'] == 'reference'
    assert info['_init_optim_info']['is_success']
    assert set(samples) == {'coef', 'global_scale', 'logp'}
    assert np.all(np.isfinite(samples['coef']))
    assert info['_init_optim_info']['n_iter'] > 0
    # the search went uphill from its start (all coefficients 0)
    assert cpo.loglik_grad(D, y, np.log(e), sptr, info['init']['coef'])[0] > \
        cpo.loglik_grad(D, y, np.log(e), sptr, np.zeros(CHAIN_P))[0]
    assert 'obs_prec' not in info['_markov_chain_state']


# ---------------------------------------------------------------- refusals
def test_refusals_are_exceptions():
    """test_hip_poisson.py's refusals on a stratified model."""
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior, SamplerOptions
    model = _data('dense64', [4] * 25, 20)[0]
    bridge = BayesBridge(model, RegressionCoefPrior(bridge_exponent=.5))
    init = {'global_scale': .1}
    for method in ('cg', 'cholesky', 'woodbury'):
        with pytest.raises(ValueError):
            bridge.gibbs(2, init=init, seed=0, coef_sampler_type=method)
        with pytest.raises(ValueError):
            bridge.gibbs(2, init=init, seed=0, options=SamplerOptions(method))
    with pytest.raises(ValueError):
        bridge.gibbs(2, init=init, seed=0, options={'rng': 'device'})
    with pytest.raises(ValueError, match="'cg'"):
        bridge.gibbs_batch([0, 1], 2, init=init)
    with pytest.raises(ValueError, match="'cg'"):
        bridge.gibbs_batch([0, 1], 2, init=init,
                           options={'coef_sampler_type': 'hmc'})
    with pytest.raises(ValueError, match="'cg' only"):
        bridge.gibbs_multichain(2, 2, init=init)
    rs = np.random.RandomState(2)
    op = model.get_hessian_matvec_operator(rs.randn(20) * .1)
    op(rs.randn(20))
    model.get_hessian_matvec_operator(rs.randn(20) * .1)
    with pytest.raises(RuntimeError, match='location has moved'):
        op(rs.randn(20))
    with pytest.raises(ValueError):
        model.compute_loglik_and_gradient(np.zeros(19))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def test_c_abi_errors_are_status_codes():
    """Every refusal is an argument check made before any launch."""
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    lib.bbx_launch_count.restype = c_uint64
    rs = np.random.RandomState(0)
    n, p = 50, 4
    design = HipDenseDesignMatrix(rs.randn(n, p), add_intercept=False)
    y, o = np.ones(n), np.full(n, .5)
    sptr = np.arange(0, n + 1, 5, dtype=np.int64)
    ns = len(sptr) - 1
    vec, out = rs.randn(p) * .1, np.empty(p)
    ll, k = c_double(), c_int()
    null = c_void_p()
    before = lib.bbx_launch_count()
    # NULL handle
    assert lib.bbx_cpoisson_loglik_grad(null, _ptr(vec), byref(ll), None) < 0
    assert lib.bbx_cpoisson_set_location(null, _ptr(vec)) < 0
    assert lib.bbx_cpoisson_hessian_matvec(null, _ptr(vec), _ptr(out)) < 0
    assert lib.bbx_cpoisson_nuts_sample(null, None, byref(ll), None) < 0
    assert lib.bbx_cpoisson_destroy(null) == 0

    def create(y_, o_, ns_, sptr_, design_=design.handle):
        h = c_void_p()
        arrays = [None if a is None else np.ascontiguousarray(a)
                  for a in (y_, o_, sptr_)]
        st = lib.bbx_cpoisson_create(design_, _ptr(arrays[0]),
                                     _ptr(arrays[1]), ns_, _ptr(arrays[2]),
                                     byref(h))
        assert (st == 0) == bool(h.value)
        return st, _lib.last_error(), h

    # NULL pointers
    assert lib.bbx_cpoisson_create(design.handle, _ptr(y), _ptr(o), ns,
                                   _ptr(sptr), None) == ERR_INVALID
    assert 'output' in _lib.last_error()
    assert create(y, o, ns, sptr, null)[0] == ERR_INVALID
    st, msg, _ = create(None, o, ns, sptr)
    assert st == ERR_INVALID and 'NULL y' in msg
    st, msg, _ = create(y, o, ns, None)
    assert st == ERR_INVALID and 'NULL stratum_ptr' in msg
    at = np.arange(n)
    for bad_y, bad_o, name in (
            (np.where(at == 7, -1., y), o, 'y[7]'),
            (np.where(at == 7, np.nan, y), o, 'y[7]'),
            (np.where(at == 7, np.inf, y), o, 'y[7]'),
            (y, np.where(at == 9, np.inf, o), 'log_exposure[9]'),
            (y, np.where(at == 9, -np.inf, o), 'log_exposure[9]'),
            (y, np.where(at == 9, np.nan, o), 'log_exposure[9]')):
        st, msg, _ = create(bad_y, bad_o, ns, sptr)
        assert st == ERR_INVALID and name in msg, (name, st, msg)

    def changed(index, value):
        s = sptr.copy()
        s[index] = value
        return s

    for bad, name in ((changed(0, 1), 'stratum_ptr[0]'),
                      (changed(ns, n - 1), 'stratum_ptr[n_strata]'),
                      (changed(ns, n + 1), 'stratum 9'),
                      (changed(3, sptr[2]), 'stratum 2'),     # an empty one
                      (changed(3, sptr[4] + 1), 'stratum 3')):
        st, msg, _ = create(y, o, ns, bad)
        assert st == ERR_INVALID and name in msg and 'stratum_ptr' in msg, \
            (name, st, msg)
    assert create(y, o, 0, sptr)[0] == ERR_INVALID
    assert 'n_strata' in _lib.last_error()
    # a stratum whose counts sum to 0
    st, msg, _ = create(np.where((at >= 10) & (at < 15), 0., y), o, ns, sptr)
    assert st == ERR_INVALID and 'stratum 2' in msg and 'sum to 0' in msg
    assert lib.bbx_launch_count() == before
    # no offset: log_exposure = NULL
    st, _, h0 = create(y, None, ns, sptr)
    assert st == 0
    st, _, h = create(y, o, ns, sptr)
    assert st == 0
    ll0 = c_double()
    assert lib.bbx_cpoisson_loglik_grad(h0, _ptr(vec), byref(ll0), None) == 0
    assert lib.bbx_cpoisson_destroy(h0) == 0
    # order of calls
    assert lib.bbx_cpoisson_hessian_matvec(h, _ptr(vec),
                                           _ptr(out)) == ERR_STATE
    assert 'set_location' in _lib.last_error()
    u = rs.rand(1)
    assert lib.bbx_cpoisson_nuts_doubling(h, .1, 1, 0, _ptr(u), byref(k),
                                          byref(k), None, None,
                                          None) == ERR_STATE
    assert 'nuts_begin' in _lib.last_error()
    assert lib.bbx_cpoisson_nuts_sample(h, None, byref(ll), None) == ERR_STATE
    assert lib.bbx_cpoisson_hmc_trajectory(
        h, .1, -1, _ptr(vec), _ptr(vec), _ptr(vec), _ptr(vec), 0., _ptr(vec),
        100., None, None, None, None, None, None, None) == ERR_INVALID
    assert lib.bbx_cpoisson_loglik_grad(h, _ptr(vec), byref(ll),
                                        _ptr(out)) == 0
    # a constant offset cancels inside every stratum
    assert np.isfinite(ll.value) and ll.value <= 0.
    np.testing.assert_allclose(ll.value, ll0.value, rtol=1e-12)
    # use after the design is destroyed
    design.__del__()
    assert lib.bbx_cpoisson_loglik_grad(h, _ptr(vec), byref(ll),
                                        None) == ERR_STATE
    assert 'destroyed' in _lib.last_error()
    assert lib.bbx_cpoisson_destroy(h) == 0


# ------------------------------------------------------- statistical check
def _stat_problem():
    """About 200 strata of 2 to 6 rows, p = 6, with stratum baselines
    alpha_s ~ N(0, 2^2) which the model never sees."""
    rs = np.random.RandomState(21)
    sizes = rs.randint(2, 7, 200)
    sptr = cpo.stratum_ptr_of(sizes)
    n = int(sptr[-1])
    X = rs.randn(n, 6) * .5
    truth = np.array([.6, -.4, .3, 0., -.2, .1])
    alpha = np.repeat(rs.randn(200) * 2., sizes)
    y = rs.poisson(np.exp(alpha + X.dot(truth))).astype(np.float64)
    return X, y, np.repeat(np.arange(200), sizes), truth


def _stat_chain(BayesBridge, RegressionCoefPrior, model):
    prior = RegressionCoefPrior(bridge_exponent=2.,
                                _global_scale_parametrization='raw')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            samples, _ = BayesBridge(model, prior).gibbs(
                500, n_burnin=100, seed=3, coef_sampler_type='nuts',
                init={'coef': np.zeros(6), 'global_scale': 100.},
                options={'global_scale_update': None})
    assert samples['coef'].shape == (6, 400)
    return samples


def test_posterior_mean_is_near_the_conditional_mle():
    """Unit exposure, a Gaussian prior (bridge exponent 2) of fixed, large
    scale: the posterior is close to the conditional likelihood, so each
    posterior mean lies within 5 posterior sd of the conditional
    maximum-likelihood estimate (Newton iterations on the oracle).  The
    factory drops the strata without a count."""
    # The same chain (seed 3, 500 'nuts' iterations, 100 of them burn-in) on
    # cpoisson_oracle.OracleModel alone, on the CPU: 642 of the 776 rows are
    # kept, the largest deviation is 0.112 posterior sd (the others 0.023 to
    # 0.048); the estimate lies within 0.68 of its own standard errors of
    # the simulation's coefficients.
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel, cpoisson_preprocess
    X, y, lab, truth = _stat_problem()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((y, None, lab), X, 'poisson')
        ys, _, labs, Xs, keep = cpoisson_preprocess(y, None, lab, X)
    assert model.n_obs == len(keep) < len(y)
    D = lo.design(Xs, True, False, offset=model.design.column_offset)
    mle, cov = cpo.newton_mle(D, ys, np.zeros(len(ys)), model.stratum_ptr)
    samples = _stat_chain(BayesBridge, RegressionCoefPrior, model)
    mean, sd = samples['coef'].mean(axis=1), samples['coef'].std(axis=1)
    dev = np.abs(mean - mle) / sd
    print('mle', mle, 'posterior mean', mean, 'sd', sd, 'deviation', dev)
    assert np.all(np.abs(truth - mle) < 5 * np.sqrt(np.diag(cov)))
    assert dev.max() < 5.
