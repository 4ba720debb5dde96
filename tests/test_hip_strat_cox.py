"""GPU: the stratified Cox partial likelihood on the device
(csrc/cox_strat.hpp, bbx_cox_create_stratified) against the sum-over-strata
oracle of tests/strat_cox_oracle.py, under the bounds test_hip_cox_edges.py
applies to the unstratified handle (cox_oracle.EDGE_TOL times the
extended-precision reference's componentwise bound; the trajectory bounds of
its _traj_check).

The segmented scans run over the row range [0, n) (forward, and reversed)
and the event range [0, n_event), each cut into SCAN_G = 256 chunks of C =
ceil(len / 256) elements scanned in tiles of T = 2048.  The shapes put
stratum boundaries on chunk edges (and, at n > 256 T, on tile edges), strata
of 1 .. T + 1 rows, strata of events only, a stratum whose events all tie,
one stratum over many chunks between runs of tiny ones, 3000 matched pairs,
and a single stratum."""
import math
import warnings
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import cox_oracle as co
import nuts_oracle as no
import strat_cox_oracle as so
from test_hip_cox_edges import TOL, _traj_check, _within

pytestmark = pytest.mark.gpu

G, T = 256, 2048                     # SCAN_G, SCAN_TILE
ERR_INVALID = -1
EDGE_SIZES = [1, 2, 3, 7, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1]


def _chunk(n):
    return -(-n // G)


def _design(kind, X):
    """A device design on rows already in order and the matrix the oracle
    uses (test_hip_cox_edges._model's construction)."""
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if kind in ('dense64', 'dense32'):
        dtype = 'float32' if kind == 'dense32' else 'float64'
        if dtype == 'float32':
            X = X.astype(np.float32).astype(np.float64)
        return HipDenseDesignMatrix(X, add_intercept=False,
                                    storage_dtype=dtype), X
    S = sparse.csr_matrix(X)
    S.sort_indices()
    storage = 'csr' if kind == 'csr_valued' else 'tiled'
    return HipSparseDesignMatrix.from_csr_arrays(
        S.shape, S.indptr, S.indices, S.data, add_intercept=False,
        storage=storage), X


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


def _model(kind, et, ct, lab, p, seed=0):
    from bayesbridge_amd import RegressionModel
    design, X = _design(kind, _values(kind, len(et), p, seed))
    model = RegressionModel((et, ct, lab), design, 'cox')
    assert model.n_pred == p and model.strata is not None
    return model, X, so.split(et, ct, lab)


def _betas(p, seed=1):
    rs = np.random.RandomState(seed)
    return [np.zeros(p), rs.randn(p) * .3, rs.randn(p) * 2.]


def _check(model, X, pieces, betas, v_seed=1):
    """test_hip_cox_edges._check on the stratified oracle: loglik, gradient,
    loglik_only, the Hessian matvec after set_location, bitwise repeats."""
    rs = np.random.RandomState(v_seed)
    worst = 0.
    for beta in betas:
        ll, grad = model.compute_loglik_and_gradient(beta)
        el, eg, lb, gb = so.loglik_grad_ext(X, beta, pieces)
        assert math.isfinite(el)
        print('loglik', ll, el, 'err / bound', abs(ll - el) / lb,
              'grad err / bound', np.max(np.abs(grad - eg) / gb))
        assert abs(ll - el) <= TOL * lb, (ll, el, lb)
        assert _within(grad, eg, gb), np.max(np.abs(grad - eg) / gb)
        worst = max(worst, co.distance_in_tolerances((ll, grad),
                                                     (el, eg, lb, gb)))
        lo, none = model.compute_loglik_and_gradient(beta, loglik_only=True)
        assert none is None and lo == ll
        v = rs.randn(len(beta))
        hv = model.get_hessian_matvec_operator(beta)(v)
        eh, hb = so.hessian_matvec_ext(X, beta, v, pieces)
        print('hessian err / bound', np.max(np.abs(hv - eh) / hb))
        assert _within(hv, eh, hb), np.max(np.abs(hv - eh) / hb)
        ll2, grad2 = model.compute_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        hv2 = model.get_hessian_matvec_operator(beta)(v)
        assert np.array_equal(hv2, hv)
    assert worst <= 1.
    return ll, grad


def _pairs(n_pair, seed=0):
    """1:1 matched sets: one event, one row censored at or after it."""
    rs = np.random.RandomState(seed)
    t = np.round(rs.exponential(1., n_pair) + .1, 1)
    c = np.round(t + rs.exponential(1., n_pair), 1)      # some tie with t
    et = np.column_stack((t, np.full(n_pair, np.inf))).ravel()
    ct = np.column_stack((np.full(n_pair, np.inf), c)).ravel()
    return et, ct, np.repeat(np.arange(n_pair), 2)


def _seam_layout(n=70144):
    """Stratum sizes for n = 256 * 274 rows (C = 274): two shuffled rounds of
    EDGE_SIZES, a filler that ends on a chunk edge, a run of tiny strata, one
    stratum over ~73 chunks, another run of tiny ones, and a last stratum
    that ends the rows.  Returns (sizes, only_events, all_tied)."""
    C = _chunk(n)
    assert C * G == n
    rs = np.random.RandomState(11)
    sizes = list(rs.permutation(EDGE_SIZES * 2))
    used = int(np.sum(sizes))
    sizes.append(-used % C + C)                  # next boundary: C * j
    assert int(np.sum(sizes)) % C == 0
    tiny = list(rs.randint(1, 4, 300))
    sizes += tiny + [20000] + list(rs.randint(1, 4, 300))
    sizes.append(n - int(np.sum(sizes)))
    assert sizes[-1] > T
    where = {s: [i for i, x in enumerate(sizes) if x == s] for s in set(sizes)}
    only_events = [where[1][0], where[64][0], where[T][0], where[3][1]]
    all_tied = [where[257][0], where[7][1], where[2][2]]
    return sizes, only_events, all_tied


CASES = {}


def _case(name):
    """(event_time, censoring_time, labels) of a named shape, built once."""
    if name not in CASES:
        if name == 'pairs':
            CASES[name] = _pairs(3000)
        elif name == 'seams':
            sizes, only_events, all_tied = _seam_layout()
            CASES[name] = so.make_strata(
                sizes, 1, seed=2, only_events=only_events, all_tied=all_tied,
                shuffle=False)[:3]
        elif name == 'small':
            sizes = [1, 2, 3, 7, 63, 64, 65, 255, 256, 257, 40, 1, 2, 900]
            CASES[name] = so.make_strata(sizes, 1, seed=3, only_events=[0, 4],
                                         all_tied=[5])[:3]
        elif name == 'one':
            et, ct, _ = so.make_strata([6000], 1, seed=4)[:3]
            CASES[name] = (et, ct, np.full(6000, 'all'))
        elif name == 'tiles':
            # n = 256 * 2344: chunks of two tiles.  Strata of T - 1, T, T + 1
            # and 293 rows; the first boundary on a tile edge inside chunk 0
            # (row T), later ones on chunk edges (2344 = 8 * 293)
            n = G * 2344
            sizes = [T, 2344 - T, T - 1, T + 1, 2 * 2344 - 2 * T]
            sizes += [293] * ((n - int(np.sum(sizes))) // 293)
            assert int(np.sum(sizes)) == n
            CASES[name] = so.make_strata(sizes, 1, seed=5, only_events=[2],
                                         all_tied=[3], shuffle=False)[:3]
    return CASES[name]


def test_seam_layout_reaches_every_seam():
    """The 'seams' rows: boundaries on chunk edges of the forward row scan,
    strata inside one chunk, across one edge and across many."""
    et, ct, lab = _case('seams')
    n = len(et)
    C = _chunk(n)
    assert n == 70144 and C == 274
    bounds = np.flatnonzero(lab[1:] != lab[:-1]) + 1
    assert np.any(bounds % C == 0)
    size = np.diff(np.concatenate(([0], bounds, [n])))
    assert set(EDGE_SIZES) <= set(size.tolist())
    big = np.argmax(size == 20000)
    assert np.all(size[big - 300:big] <= 3) and np.all(size[big + 1:big + 301]
                                                       <= 3)
    ev = np.isfinite(et)
    per = [(ev[a:b], et[a:b]) for a, b in zip(
        np.concatenate(([0], bounds)), np.concatenate((bounds, [n])))]
    assert sum(np.all(e) for e, _ in per) >= 4          # events only
    assert sum(len(t) > 2 and np.sum(e) > 2 and len(np.unique(t[e])) == 1
               for e, t in per) >= 2                     # all events tied


@pytest.mark.parametrize('shape', ['pairs', 'seams', 'one'])
@pytest.mark.parametrize('kind', ['dense64', 'tiled_binary'])
def test_likelihood_gradient_hessian_match_the_oracle(kind, shape):
    et, ct, lab = _case(shape)
    p = 6
    model, X, pieces = _model(kind, et, ct, lab, p)
    _check(model, X, pieces, _betas(p))


@pytest.mark.parametrize('kind', ['csr_valued', 'dense32', 'mixed'])
def test_other_designs(kind):
    et, ct, lab = _case('small')
    model, X, pieces = _model(kind, et, ct, lab, 10)
    _check(model, X, pieces, _betas(10)[1:2])


def test_chunks_of_two_tiles():
    """n = 600 064: every chunk of the row scans runs two tiles, stratum
    boundaries on a tile edge and on chunk edges -- the carry from tile to
    tile, which no smaller n reaches."""
    et, ct, lab = _case('tiles')
    assert _chunk(len(et)) > T
    bounds = np.flatnonzero(lab[1:] != lab[:-1]) + 1
    assert bounds[0] == T and np.any(bounds % _chunk(len(et)) == 0)
    model, X, pieces = _model('dense64', et, ct, lab, 3)
    _check(model, X, pieces, _betas(3)[1:2])


def test_single_stratum_equals_the_unstratified_handle():
    """One label for all rows: the stratified path against the oracle and
    against the unstratified handle on the same rows, under the same bound."""
    from bayesbridge_amd import RegressionModel
    et, ct, lab = _case('one')
    p = 6
    model, X, pieces = _model('dense64', et, ct, lab, p)
    plain = RegressionModel((et, ct), _design('dense64', X)[0], 'cox')
    assert plain.strata is None
    rs = np.random.RandomState(1)
    for beta in _betas(p):
        el, eg, lb, gb = so.loglik_grad_ext(X, beta, pieces)
        ll, grad = model.compute_loglik_and_gradient(beta)
        pl, pgrad = plain.compute_loglik_and_gradient(beta)
        print('stratified - plain: loglik', abs(ll - pl) / lb, 'grad',
              np.max(np.abs(grad - pgrad) / gb), '(in bounds)')
        assert abs(ll - el) <= TOL * lb and abs(pl - el) <= TOL * lb
        assert abs(ll - pl) <= TOL * lb
        assert _within(grad, pgrad, gb) and _within(grad, eg, gb)
        v = rs.randn(p)
        eh, hb = so.hessian_matvec_ext(X, beta, v, pieces)
        hv = model.get_hessian_matvec_operator(beta)(v)
        ph = plain.get_hessian_matvec_operator(beta)(v)
        print('hessian', np.max(np.abs(hv - ph) / hb))
        assert _within(hv, eh, hb) and _within(hv, ph, hb)


def test_the_shift_is_per_stratum():
    """Two strata whose eta differ by 800 through an intercept-like column:
    finite, equal to the oracle -- and infinitely far from a likelihood with
    one global max, which sees H_k == 0 in the lower stratum."""
    et, ct, lab = so.make_strata([300, 500], 1, seed=6, shuffle=False)[:3]
    rs = np.random.RandomState(6)
    X = np.column_stack((rs.randn(len(et), 3), (lab == 1) * 1.))
    from bayesbridge_amd import RegressionModel
    model = RegressionModel((et, ct, lab), _design('dense64', X)[0], 'cox')
    pieces = so.split(et, ct, lab)
    beta = np.array([.3, -.5, .2, 800.])
    eta = X @ beta
    assert eta[lab == 1].min() - eta[lab == 0].max() > 780
    ll, grad = model.compute_loglik_and_gradient(beta)
    want = so.loglik_grad_ext(X, beta, pieces)
    assert math.isfinite(ll) and math.isfinite(want[0])
    assert co.distance_in_tolerances((ll, grad), want) <= 1.
    mutant = so.loglik_grad_global_max(X, beta, pieces)
    assert mutant[0] == -math.inf
    assert co.distance_in_tolerances((ll, grad), (mutant[0], mutant[1], 0.,
                                                  None)) == math.inf
    v = rs.randn(4)
    hv = model.get_hessian_matvec_operator(beta)(v)
    eh, hb = so.hessian_matvec_ext(X, beta, v, pieces)
    assert _within(hv, eh, hb)


def _underflow_model():
    """test_hip_cox_edges' zero risk-set sum inside the first of two strata:
    row 0 alone carries column 0."""
    from bayesbridge_amd import RegressionModel
    n, m = 40, 20
    rs = np.random.RandomState(3)
    X = np.column_stack((np.eye(n + m)[0], rs.randn(n + m) * .1))
    et = np.concatenate((np.arange(1., n + 1.), np.arange(1., m + 1.)))
    ct = np.full(n + m, np.inf)
    lab = np.repeat([0, 1], [n, m])
    model = RegressionModel((et, ct, lab), _design('dense64', X)[0], 'cox')
    return model, X, so.split(et, ct, lab)


def test_zero_risk_set_sum_in_one_stratum():
    from bayesbridge_amd import _lib
    model, X, pieces = _underflow_model()
    beta = np.array([800., 0.])
    assert so.loglik_grad(X, beta, pieces) == (-math.inf, None)
    assert model.compute_loglik_and_gradient(beta) == (-math.inf, None)
    st = _lib.load().bbx_cox_set_location(model.handle,
                                          beta.ctypes.data_as(c_void_p))
    assert st == _lib.ERR_NUMERIC and 'risk-set sum' in _lib.last_error()
    with pytest.raises(ValueError, match='Hessian operator'):
        model.get_hessian_matvec_operator(beta)
    assert math.isfinite(model.compute_loglik_and_gradient(beta * .5)[0])


def test_trajectory_stops_at_a_zero_risk_set_sum_after_step_one():
    """As test_hip_cox_edges' test of this name: beta_0 = 400, 600, 800; at
    step 2 every later risk set of stratum 0 sums to 0."""
    model, X, pieces = _underflow_model()
    scale, pp = np.ones(2), np.full(2, 1e-8)
    f = so.precond_f(X, scale, pp, pieces)
    q0, p0 = np.array([400., 0.]), np.array([200., .1])
    logp0, grad0 = f(q0)
    with np.errstate(all='ignore'):
        want = co.trajectory(f, 1., 10, q0, p0, logp0, grad0, tol=1e300)
    got = model.hmc_trajectory(1., 10, scale, pp, q0, p0, logp0, grad0,
                               hamiltonian_tol=1e300)
    assert want[4] and want[2] == -np.inf and want[3] == 2
    _traj_check(got, want, 10)


def _launches(model, beta):
    from bayesbridge_amd import _lib
    lib = _lib.load()
    lib.bbx_launch_count.restype = c_uint64
    before = lib.bbx_launch_count()
    model.compute_loglik_and_gradient(beta)
    return lib.bbx_launch_count() - before


def test_launch_count_does_not_depend_on_the_strata():
    et, ct, lab = _case('pairs')
    p = 6
    many, X, _ = _model('dense64', et, ct, lab, p)
    one_t, one_c, _ = so.make_strata([len(et)], 1, seed=4)[:3]
    one = _model('dense64', one_t, one_c, np.zeros(len(et)), p)[0]
    beta = _betas(p)[1]
    a, b = _launches(many, beta), _launches(one, beta)
    assert a == b > 0, (a, b)
    assert _launches(many, beta) == a


def _traj_inputs(X, pieces, seed=0):
    P = X.shape[1]
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    pp = np.ones(P)
    f = so.precond_f(X, scale, pp, pieces)
    q0, p0 = rs.randn(P) * .1, rs.randn(P)
    return (f, scale, pp, q0, p0) + f(q0)


@pytest.fixture(scope='module')
def small():
    et, ct, lab = _case('small')
    return _model('dense64', et, ct, lab, 20)


@pytest.mark.parametrize('n_step', [0, 1, 64])
def test_trajectory_matches_host_velocity_verlet(small, n_step):
    model, X, pieces = small
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(X, pieces)
    want = co.trajectory(f, .02, n_step, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(.02, n_step, scale, pp, q0, p0, logp0, grad0)
    assert not want[4] and want[3] == n_step
    _traj_check(got, want, n_step)


def test_nuts_doublings_match_the_restatement(small):
    """nuts_begin and doublings to height 3 against tests/nuts_oracle.py on
    the stratified f (test_hip_nuts.py's comparison and bounds)."""
    from bayesbridge_amd import nuts
    from test_hip_nuts import ATOL, RTOL
    model, X, pieces = small
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(X, pieces, seed=2)
    np.random.seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        q, info = nuts.generate_next_state(model, .01, q0, scale, pp, p=p0,
                                           max_height=3)
    np.random.seed(9)
    wq, want = no.generate_next_state(f, .01, q0, logp0, grad0, p=p0,
                                      max_height=3)
    assert info['tree_height'] == want['tree_height'] == 3
    assert info['n_grad_evals'] == want['n_grad_evals'] + 1
    assert info['n_uniform'] == want['n_uniform']
    for key in ('u_turn_detected', 'instability_detected',
                'last_doubling_rejected'):
        assert info[key] == want[key]
    np.testing.assert_allclose(q, wq, rtol=RTOL, atol=ATOL)
    for key in ('ave_accept_prob', 'ave_hamiltonian_error'):
        assert info[key] == pytest.approx(want[key], rel=1e-9)


@pytest.mark.parametrize('method', ['hmc', 'nuts'])
def test_seeded_chain(method):
    """Raw (shuffled, with an eventless stratum) input through
    RegressionModel and BayesBridge.gibbs: shapes, finiteness, the same seed
    twice, and every kept logp against the host's log-posterior on the
    stratified oracle (bayesbridge.py:480-511), to the rel 1e-10 of
    test_hip_fullsize.py."""
    from bayesbridge_amd import (BayesBridge, RegressionCoefPrior,
                                 RegressionModel)
    from bayesbridge_amd.model import cox_preprocess_stratified
    rs = np.random.RandomState(8)
    n, p = 600, 8
    X = rs.randn(n, p)
    lab = rs.randint(0, 40, n).astype(str)
    event = np.round(rs.exponential(np.exp(-X[:, 0] * .5)), 2) + .01
    cens = np.round(rs.exponential(1.5, n), 2) + .01
    censored = cens < event
    event[censored], cens[~censored] = np.inf, np.inf
    event[lab == '7'], cens[lab == '7'] = np.inf, 1.     # no event: dropped
    prior = RegressionCoefPrior(bridge_exponent=.5, regularizing_slab_size=1.,
                                _global_scale_parametrization='raw')
    runs = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        et, ct, st, Xs, keep = cox_preprocess_stratified(event, cens, lab, X)
        for _ in range(2):
            model = RegressionModel((event, cens, lab), X, 'cox')
            samples, info = BayesBridge(model, prior).gibbs(
                8, seed=0, init={'global_scale': .1},
                coef_sampler_type=method, params_to_save='all')
            runs.append(samples)
    assert info['coef_sampler_type'] == method
    assert model.n_obs == len(keep) < n and not np.any(st == '7')
    samples = runs[0]
    assert samples['coef'].shape == (p, 8) and samples['logp'].shape == (8,)
    assert samples['global_scale'].shape == (8,)
    for key in ('coef', 'local_scale', 'global_scale', 'logp'):
        assert np.all(np.isfinite(samples[key]))
        np.testing.assert_array_equal(samples[key], runs[1][key])
    pieces = so.split(et, ct, st)
    # the model centres no column of a Cox design away: eta = X beta up to a
    # constant per column, which every stratum's likelihood ignores
    for k in range(8):
        coef, g = samples['coef'][:, k], samples['global_scale'][k]
        ll, _ = so.loglik_grad(Xs, coef, pieces)
        want = ll - .5 * np.sum((coef / 1.) ** 2) - p * math.log(g) \
            - np.sum(np.abs(coef / g) ** .5) - math.log(g)
        assert samples['logp'][k] == pytest.approx(want, rel=1e-10)


def test_c_abi_refusals():
    """bbx_cox_create_stratified refuses what its kernels would dereference,
    with a message, before anything is launched."""
    from bayesbridge_amd import _lib
    from bayesbridge_amd.model import cox_stratified_risk_sets
    lib = _lib.load()
    lib.bbx_launch_count.restype = c_uint64
    et, ct, lab = so.make_strata([5, 9, 4], 1, seed=1, shuffle=False)[:3]
    design = _design('dense64', np.random.RandomState(0).randn(len(et), 3))[0]
    sptr, sne, start, end, last = cox_stratified_risk_sets(et, ct, lab)
    good = [np.ascontiguousarray(sptr, dtype=np.int64)] + [
        np.ascontiguousarray(a, dtype=np.int32)
        for a in (sne, start, end, last)]

    def create(arrays, n_strata=3):
        h = c_void_p()
        st = lib.bbx_cox_create_stratified(
            design.handle, n_strata,
            *[None if a is None else a.ctypes.data_as(c_void_p)
              for a in arrays], byref(h))
        if st == 0:
            lib.bbx_cox_destroy(h)
        else:
            assert not h
        return st, _lib.last_error()

    def changed(which, index, value):
        arrays = [a.copy() for a in good]
        arrays[which][index] = value
        return arrays

    before = lib.bbx_launch_count()
    assert create(good)[0] == 0
    for k in range(5):
        st, msg = create(good[:k] + [None] + good[k + 1:])
        assert st == ERR_INVALID and 'NULL' in msg
    ne0 = int(sne[0])
    bad = [
        (changed(0, 1, sptr[2] + 1), 'stratum 1'),       # not monotone
        (changed(0, 2, sptr[1]), 'stratum 1'),           # an empty stratum
        (changed(0, 0, 1), 'stratum_ptr[0]'),
        (changed(0, 3, len(et) - 1), 'stratum_ptr[n_strata]'),
        (changed(1, 1, 0), 'stratum 1'),                 # no event
        (changed(1, 2, 5), 'stratum 2'),                 # more than its rows
        (changed(2, ne0, start[ne0] - 1), 'risk set %d' % ne0),
        (changed(2, 1, 2), 'risk set 1'),                # start past the event
        (changed(3, 0, sptr[1]), 'risk set 0'),          # end in stratum 1
        (changed(3, ne0, sptr[1] - 1), 'risk set %d' % ne0),
        (changed(4, 0, ne0), 'last_set[0]'),             # an event of stratum 1
        (changed(4, int(sptr[1]), ne0 - 1), 'last_set[%d]' % sptr[1]),
        (changed(4, len(et) - 1, int(np.sum(sne))),
         'last_set[%d]' % (len(et) - 1)),
    ]
    for arrays, name in bad:
        st, msg = create(arrays)
        assert st == ERR_INVALID and name in msg, (name, st, msg)
    assert create(good, n_strata=0)[0] == ERR_INVALID
    h = c_void_p()
    assert lib.bbx_cox_create_stratified(
        None, 3, *[a.ctypes.data_as(c_void_p) for a in good],
        byref(h)) == ERR_INVALID
    assert lib.bbx_launch_count() == before
