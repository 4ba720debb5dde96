"""GPU: the negative-binomial model (csrc/negbin.hip on csrc/hamiltonian.hpp,
csrc/negbin_predict.hip) -- the likelihood, its gradient, its Hessian matvec
and the dispersion's log-likelihood against the NumPy oracle
(tests/negbin_oracle.py) at the row counts where the row kernel changes path,
bit-equality of the dispersion sums across K and position, extreme and
infinite linear predictors, the trajectory against a host velocity Verlet,
No-U-Turn doublings against tests/nuts_oracle.py, whole seeded chains with a
sampled dispersion against the same driver on the oracle model, prediction
against a long-double oracle and the refusals.  There is no reference
implementation of this family: the oracle is the yardstick throughout."""
import math
import warnings
from ctypes import byref, c_double, c_int, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import logit_oracle as lo
import negbin_oracle as nb
import predict_oracle as pro
from test_hip_poisson import (KINDS, LAP, NPART, VEC_BLOCK, _compare_doublings,
                              _constant, _design_and_matrix)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance

U = _constant('GLM_ROW_U', 'glm_rows.hpp')
ROWS = (1, VEC_BLOCK - 1, VEC_BLOCK + 1, LAP + 1, U * LAP + 3)
DISPERSIONS = (.05, 1., 30., 1e4)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _negbin_data(kind, n, p, intercept=True, center=True, exposure=True,
                 seed=0, min_count=0, **model_args):
    """A device negative-binomial model, the oracle's design, the counts
    (overdispersed, up to a few hundred) and the offset."""
    from bayesbridge_amd import RegressionModel
    dsn, D = _design_and_matrix(kind, n, p, intercept, center, seed)
    rs = np.random.RandomState(seed + 1)
    beta = rs.randn(p) * .3
    e = rs.uniform(.5, 2., n) if exposure else None
    mu = np.exp(.2 + np.asarray(D[0].dot(beta)).ravel())
    # every eighth row has a mean in the hundreds
    mu = mu * np.where(np.arange(n) % 8 == 3, 150., 1.)
    mu = mu * (e if exposure else 1.) * rs.gamma(2., .5, n)
    y = rs.poisson(mu).astype(np.float64) + min_count
    model = RegressionModel((y, e) if exposure else y, dsn, 'negbin',
                            **model_args)
    assert model.name == 'negbin' and model.design is dsn
    return model, D, y, (np.log(e) if exposure else np.zeros(n))


# (kind, n, p, add_intercept, center_predictor, exposure)
CASES = [(kind, n, 7 if n > LAP else 23, True, True, True)
         for kind in KINDS for n in ROWS] + [
    (kind, VEC_BLOCK + 1, 23) + flags for kind in KINDS for flags in (
        (False, True, True), (True, False, True), (False, False, True),
        (True, True, False), (False, False, False))]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_likelihood_gradient_hessian_and_L_match_the_oracle(case, monkeypatch):
    kind, n, p, intercept, center, exposure = CASES[case]
    if n == 1:
        # every column of a single row is "constant", and the design classes
        # drop constant columns as hand-made intercepts: keep them, the row
        # kernel is what this case is about
        from bayesbridge_amd import design_matrix
        monkeypatch.setattr(design_matrix, 'remove_intercept_indicator',
                            lambda X: X)
    model, D, y, o = _negbin_data(kind, n, p, intercept, center, exposure,
                                  seed=case)
    assert (o != 0).any() == exposure
    if n > 8:
        assert y.max() > 100 and (y <= 8).any() and (y > 8).any()
    P = p + int(intercept)
    rs = np.random.RandomState(1)
    beta, v = rs.randn(P) * .3, rs.randn(P)
    worst = 0.
    for r in DISPERSIONS:
        model.dispersion = r
        ll, grad = model.compute_loglik_and_gradient(beta)
        oll, ograd = nb.loglik_grad(D, y, o, beta, r)
        print(kind, n, p, 'r', r, 'loglik', ll, oll, 'grad max|d| %.2e of %.3g'
              % (np.abs(grad - ograd).max(), np.abs(ograd).max()))
        assert np.isfinite(oll)
        np.testing.assert_allclose(ll, oll, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(grad, ograd, rtol=RTOL, atol=ATOL)
        ll2, grad2 = model.compute_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        hv = model.get_hessian_matvec_operator(beta)(v)
        ohv = nb.hessian_matvec(D, y, o, beta, v, r)
        print('   hessian max|d| %.2e of %.3g' % (np.abs(hv - ohv).max(),
                                                  np.abs(ohv).max()))
        np.testing.assert_allclose(hv, ohv, rtol=RTOL, atol=ATOL)
        assert np.array_equal(model.get_hessian_matvec_operator(beta)(v), hv)
        assert model.compute_loglik_and_gradient(beta, loglik_only=True) \
            == (ll, None)
        assert model.hamiltonian_loglik_and_gradient(beta)[0] == ll
    # L(r): the four values in one pass, against the long-double oracle
    rr = np.array(DISPERSIONS)
    L = model.dispersion_loglik(beta, rr)
    oL = nb.dispersion_loglik(D, y, o, beta, rr)
    worst = np.max(np.abs(L - oL) / np.abs(oL))
    print('   L(r)', L, 'max relative difference from the oracle %.2e' % worst)
    np.testing.assert_allclose(L, oL, rtol=RTOL, atol=ATOL)
    for k, r in enumerate(DISPERSIONS):
        one = model.dispersion_loglik(None, r)
        assert isinstance(one, float) and one == L[k]
    # the handle's own r and the likelihood at it were not touched
    assert model.dispersion == DISPERSIONS[-1]
    assert model.compute_loglik_and_gradient(beta)[0] == ll


@pytest.mark.parametrize('kind,n', [('tiled_binary', U * LAP + 3),
                                    ('dense64', LAP + 1)])
def test_dispersion_sums_do_not_depend_on_K_or_position(kind, n):
    model, D, y, o = _negbin_data(kind, n, 7, seed=3)
    rs = np.random.RandomState(2)
    beta = rs.randn(8) * .3
    rr = np.array([.05, .7, 1., 3., 30., 250., 1e4, 1e7])
    L8 = model.dispersion_loglik(beta, rr)
    oL = nb.dispersion_loglik(D, y, o, beta, rr)
    print('max relative difference from the oracle %.2e'
          % np.max(np.abs(L8 - oL) / np.abs(oL)))
    np.testing.assert_allclose(L8, oL, rtol=RTOL, atol=ATOL)
    # eight K = 1 calls, on the cached eta and on a fresh one
    for k in range(8):
        assert model.dispersion_loglik(None, rr[k]) == L8[k]
        assert model.dispersion_loglik(beta, rr[k:k + 1])[0] == L8[k]
    # any position, any K
    perm = rs.permutation(8)
    assert np.array_equal(model.dispersion_loglik(None, rr[perm]), L8[perm])
    for K in range(2, 8):
        assert np.array_equal(model.dispersion_loglik(None, rr[8 - K:]),
                              L8[8 - K:])
    assert np.array_equal(model.dispersion_loglik(beta, rr), L8)
    # the cached eta is the last beta's
    other = beta * .5
    Lo = model.dispersion_loglik(other, rr[:3])
    np.testing.assert_allclose(Lo, nb.dispersion_loglik(D, y, o, other, rr[:3]),
                               rtol=RTOL, atol=ATOL)
    assert np.array_equal(model.dispersion_loglik(None, rr[:3]), Lo)
    assert not np.array_equal(Lo, L8[:3])
    for bad in (np.ones(9), np.ones((2, 2)), np.array([])):
        with pytest.raises(ValueError):
            model.dispersion_loglik(None, bad)


def test_set_dispersion_changes_the_gradient_and_invalidates_the_location():
    from bayesbridge_amd import _lib
    model, D, y, o = _negbin_data('dense64', 300, 9, seed=4)
    rs = np.random.RandomState(3)
    beta, v = rs.randn(10) * .3, rs.randn(10)
    assert model.dispersion == 1.
    _, g1 = model.compute_loglik_and_gradient(beta)
    op = model.get_hessian_matvec_operator(beta)
    op(v)
    model.dispersion = 7.
    _, g7 = model.compute_loglik_and_gradient(beta)
    np.testing.assert_allclose(g1, nb.loglik_grad(D, y, o, beta, 1.)[1],
                               rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(g7, nb.loglik_grad(D, y, o, beta, 7.)[1],
                               rtol=RTOL, atol=ATOL)
    assert np.abs(g7 - g1).max() > 1.
    with pytest.raises(RuntimeError, match='location has moved'):
        op(v)
    # the C call itself: BBX_ERR_STATE until the next set_location
    lib, out = _lib.load(), np.empty(10)
    assert lib.bbx_negbin_hessian_matvec(model.handle, _ptr(v), _ptr(out)) \
        == -5
    assert 'set_location' in _lib.last_error()
    np.testing.assert_allclose(
        model.get_hessian_matvec_operator(beta)(v),
        nb.hessian_matvec(D, y, o, beta, v, 7.), rtol=RTOL, atol=ATOL)
    # refused while a No-U-Turn tree is open, accepted once its sample is
    # taken
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, y, o, 7.)
    joint = logp0 - .5 * np.dot(p0, p0)
    model.nuts_begin(scale, pp, q0, p0, logp0, grad0, joint, joint - 1.)
    with pytest.raises(_lib.BbxError, match='No-U-Turn tree'):
        model.dispersion = 2.
    assert model.dispersion == 7.
    # ... while the dispersion's log-likelihood may be asked for
    L = model.dispersion_loglik(beta, 2.)
    np.testing.assert_allclose(L, nb.dispersion_loglik(D, y, o, beta, 2.),
                               rtol=RTOL, atol=ATOL)
    model.nuts_sample()
    model.dispersion = 2.
    assert model.dispersion == 2.


def test_extreme_and_infinite_linear_predictors():
    """eta = +-1e4 stays finite (the Poisson handle overflows past 709); an
    infinite eta gives (-inf, None) and an unstable trajectory."""
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    rs = np.random.RandomState(5)
    n = VEC_BLOCK + 1
    X = rs.randn(n, 3)
    X[:, 0] = np.where(np.arange(n) % 2 == 0, 1., -1.)
    dsn = HipDenseDesignMatrix(X, add_intercept=True, center_predictor=False)
    D = lo.design(X, False, True)
    y = (1 + rs.poisson(3., n)).astype(np.float64)      # every count > 0
    model = RegressionModel(y, dsn, 'negbin', dispersion=2.)
    o = np.zeros(n)
    beta = np.array([.1, 1e4, .2, -.1])
    eta = lo.dot(D, beta)
    assert eta.max() > 9990 and eta.min() < -9990
    ll, grad = model.compute_loglik_and_gradient(beta)
    oll, ograd = nb.loglik_grad(D, y, o, beta, 2.)
    assert np.isfinite(ll) and np.all(np.isfinite(grad))
    np.testing.assert_allclose(ll, oll, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, ograd, rtol=RTOL, atol=ATOL)
    v = rs.randn(4)
    np.testing.assert_allclose(model.get_hessian_matvec_operator(beta)(v),
                               nb.hessian_matvec(D, y, o, beta, v, 2.),
                               rtol=RTOL, atol=ATOL)
    L = model.dispersion_loglik(beta, np.array([.5, 2.]))
    np.testing.assert_allclose(L, nb.dispersion_loglik(D, y, o, beta,
                                                       np.array([.5, 2.])),
                               rtol=RTOL, atol=ATOL)
    # an intercept of -inf: every eta is -inf, every count is positive
    bad = np.array([-np.inf, .1, .2, -.1])
    with np.errstate(all='ignore'):
        assert nb.loglik_grad(D, y, o, bad, 2.)[0] == -np.inf
    assert model.compute_loglik_and_gradient(bad) == (-np.inf, None)
    assert model.compute_loglik_and_gradient(bad, loglik_only=True) \
        == (-np.inf, None)
    nan = np.array([np.nan, .1, .2, -.1])
    assert np.isnan(model.compute_loglik_and_gradient(nan)[0])
    # the flags were that evaluation's only
    small = np.array([.1, .3, .2, -.1])
    ll, grad = model.compute_loglik_and_gradient(small)
    np.testing.assert_allclose(ll, nb.loglik_grad(D, y, o, small, 2.)[0],
                               rtol=RTOL, atol=ATOL)
    # a trajectory whose first step sends the intercept to -inf: no HIP
    # error, instability at step 1
    scale, pp = np.ones(4), np.ones(4)
    f = nb.precond_f(D, y, o, scale, pp, 2.)
    q0 = small.copy()
    p0 = np.array([-1e300, .1, .1, .1])
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
    assert ll2 == ll and np.array_equal(grad2, grad)
    np.testing.assert_allclose(model.design.dot(v), lo.dot(D, v), rtol=RTOL,
                               atol=ATOL)


def _traj_inputs(D, y, o, r, seed=0):
    """f of the preconditioned coordinates and a start next to the maximum of
    the likelihood (see test_hip_poisson._traj_inputs)."""
    P = D[0].shape[1] + int(D[2])
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    prior_prec = np.ones(P)
    f = nb.precond_f(D, y, o, scale, prior_prec, r)
    q0 = nb.newton_mle(D, y, o, r)[0] / scale + rs.randn(P) * .02
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


def _stability_limit(D, y, o, r, scale, pp, q0):
    """2 / sqrt(largest curvature of -f at q0), by power iteration on the
    oracle's Hessian."""
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * nb.hessian_matvec(D, y, o, q0 * scale,
                                                scale * v, r)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    return 2 / np.sqrt(curvature)


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_trajectory_matches_host_velocity_verlet(kind):
    model, D, y, o = _negbin_data(kind, 3 * VEC_BLOCK + 5, 23, dispersion=2.)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, y, o, 2.)
    limit = _stability_limit(D, y, o, 2., scale, pp, q0)
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
    model, D, y, o = _negbin_data(kind, 3 * VEC_BLOCK + 5, 23, dispersion=2.)
    oracle = nb.OracleModel(D, y, o, dispersion=2.)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, y, o, 2.)
    limit = _stability_limit(D, y, o, 2., scale, pp, q0)
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
# A chain multiplies a rounding difference from iteration to iteration: the
# step size follows log10 of the Hamiltonian's error, a small difference of
# sums of a few hundred (see test_hip_poisson.py), at a rate of about 5 per
# 'nuts' iteration and 10 to 30 per 'hmc' iteration on this problem.  The
# seeds were chosen on the oracle alone, on the CPU: for seeds 0 to 47 the
# oracle's own chain was run again with its likelihood, its gradient and L(r)
# perturbed by 1e-11 relative and by +-1e-14 relative, and compared with
# itself at this file's tolerance, rtol 1e-6 / atol 1e-9, over every saved
# parameter.  SEED_SEARCH records the outcome.  'nuts', 20 iterations: the
# seeds taken are unchanged at 1e-11.  'hmc': NO seed of the 48 is unchanged
# at 1e-11 over even 10 iterations (the best leaves the tolerance by a factor
# of 89); its chains are 10 iterations long and their seeds are the ones that
# move least, unchanged at 1e-14 with a margin of 8 (dense) and 15 (sparse).
# The rule "at most half of the seeds tried are left out" is not met in any of
# the four cases: see SEED_SEARCH.
CHAIN_SEED = {('hmc', 'sparse'): 37, ('hmc', 'dense'): 11,
              ('nuts', 'sparse'): 29, ('nuts', 'dense'): 12}
# (seeds tried, unchanged at 1e-11, unchanged at both +-1e-14), and the taken
# seed's largest deviation in units of the tolerance at 1e-11 / 1e-14
SEED_SEARCH = {('hmc', 'sparse'): (48, 0, 6, 89., .067),
               ('hmc', 'dense'): (48, 0, 2, 130., .15),
               ('nuts', 'sparse'): (48, 3, 40, .43,
                                    4e-4),
               ('nuts', 'dense'): (48, 2, 36, .94,
                                   1e-3)}


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
    e = rs.uniform(.5, 2., CHAIN_N)
    mu = e * np.exp(1. + np.asarray(X.dot(beta)).ravel())
    y = rs.poisson(mu * rs.gamma(3., 1. / 3., CHAIN_N))
    return X, y.astype(np.float64), e


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
    so no mode search runs; the dispersion starts at its default, 1."""
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, y, e = _chain_problem(fmt)
    n_iter = n_iter or CHAIN_ITER[method]
    if host:
        dsn = _HostDesign(X)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = RegressionModel((y, e), X, 'negbin', **model_args)
        dsn = model.design
    if oracle:
        D = lo.design(X, True, True, offset=dsn.column_offset)
        model = nb.OracleModel(D, y, np.log(e), design=dsn, perturb=perturb,
                               **model_args)
    prior = RegressionCoefPrior(bridge_exponent=.5, sd_for_intercept=2.,
                                regularizing_slab_size=1.)
    start = nb.newton_mle(lo.design(X), y, np.log(e), 1.)[0]
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


CHAIN_KEYS = ('coef', 'global_scale', 'logp', 'local_scale', 'dispersion')


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
    assert samples['dispersion'].shape == (n_iter,)
    assert len(set(samples['dispersion'])) == n_iter
    assert info['_markov_chain_state']['dispersion'] \
        == samples['dispersion'][-1]
    si, wsi = (i['_reg_coef_sampling_info'] for i in (info, winfo))
    assert set(si) == set(wsi) == set(HMC_INFO_KEYS if method == 'hmc'
                                      else NUTS_INFO_KEYS)
    print('dispersion', samples['dispersion'][[0, -1]], 'n_grad_evals',
          si['n_grad_evals'], 'max rel coef',
          np.max(np.abs(samples['coef'] - want['coef'])
                 / (np.abs(want['coef']) + 1e-3)), 'max rel dispersion',
          np.max(np.abs(samples['dispersion'] / want['dispersion'] - 1)))
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


def test_fixed_dispersion_chain_draws_no_uniforms_for_it(monkeypatch):
    """dispersion=3.0: samples['dispersion'] is constant, the slice update
    never runs -- the chain consumes what a Poisson chain consumes -- and it
    matches the driver on the oracle with the same fixed value.  The first
    coefficient draw of a sampled chain started at 3 is the same draw."""
    from bayesbridge_amd import bayesbridge
    fixed, info = _chain('dense', 'nuts', 12, n_iter=8, dispersion=3.)
    want, _ = _chain('dense', 'nuts', 12, n_iter=8, oracle=True,
                     dispersion=3.)
    assert np.all(fixed['dispersion'] == 3.)
    assert info['_markov_chain_state']['dispersion'] == 3.
    for key in CHAIN_KEYS:
        np.testing.assert_allclose(fixed[key], want[key], rtol=RTOL,
                                   atol=ATOL, err_msg=key)

    def never(*args, **kw):
        raise AssertionError("the dispersion is fixed")

    monkeypatch.setattr(bayesbridge, 'update_dispersion', never)
    again, _ = _chain('dense', 'nuts', 12, n_iter=8, dispersion=3.)
    for key in CHAIN_KEYS:
        assert np.array_equal(again[key], fixed[key]), key


def test_default_sampler_mode_search_and_initial_dispersion():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    from bayesbridge_amd import RegressionModel
    X, y, e = _chain_problem('dense')
    model = RegressionModel((y, e), X, 'negbin',
                            dispersion_prior={'shape': 3., 'rate': .5})
    assert model.intercept_added            # added by default, as for logit
    prior = RegressionCoefPrior(bridge_exponent=.5, sd_for_intercept=2.,
                                regularizing_slab_size=1.)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        samples, info = BayesBridge(model, prior).gibbs(
            3, init={'global_scale': .1, 'dispersion': 2.5}, seed=1,
            params_to_save=('coef', 'dispersion'))
    assert info['coef_sampler_type'] == 'hmc'
    assert info['options']['rng'] == 'reference'
    assert info['_init_optim_info']['is_success']
    assert info['init']['dispersion'] == 2.5
    assert set(samples) == {'coef', 'dispersion'}
    assert np.all(np.isfinite(samples['coef']))
    assert np.all(samples['dispersion'] > 0)
    assert model.dispersion == samples['dispersion'][-1]
    # the search went uphill from its start, at the initial dispersion
    D = lo.design(X, True, True, offset=model.design.column_offset)
    start = np.zeros(CHAIN_P + 1)
    start[0] = model.calc_intercept_mle()
    assert nb.loglik_grad(D, y, np.log(e), info['init']['coef'], 2.5)[0] > \
        nb.loglik_grad(D, y, np.log(e), start, 2.5)[0]


def test_refusals_are_exceptions():
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior, SamplerOptions
    model, D, y, o = _negbin_data('dense64', 100, 20)
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
# Tolerances relative to the largest magnitude of the vector compared, by the
# rule of test_hip_predict.py: the largest error of the oracle's float64
# recurrence against its long-double explicit form, measured on the inputs of
# the test below on the CPU (PREDICT_MEASURED), times 16, rounded up to a
# power of ten; the test repeats the measurement and holds the recurrence to
# the same tolerance first.
PREDICT_MEASURED = {'mean': 3.18e-16, 'sd': 4.26e-16, 'lpd': 1.41e-15,
                    'loglik_mean': 1.41e-16, 'loglik_var': 2.91e-15}
PREDICT_TOL = {'mean': 1e-14, 'sd': 1e-14, 'lpd': 1e-13, 'loglik_mean': 1e-14,
               'loglik_var': 1e-13}


def _predict_case():
    rs = np.random.RandomState(31)
    n, p, S = 2 * VEC_BLOCK + 37, 9, 37
    X = rs.randn(n, p) * .5
    e = rs.uniform(.5, 2., n)
    truth = rs.randn(p) * .3
    mu = e * np.exp(.8 + X.dot(truth))
    mu = mu * np.where(np.arange(n) % 8 == 3, 60., 1.)
    y = rs.poisson(mu * rs.gamma(3., 1. / 3., n)).astype(np.float64)
    coef = np.vstack((.8 + rs.randn(S) * .05,
                      truth[:, None] + rs.randn(p, S) * .05))
    r = np.exp(math.log(3.) + rs.randn(S) * .2)
    return X, e, y, coef, r


def test_predict_matches_the_long_double_oracle():
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    X, e, y, coef, r = _predict_case()
    dsn = HipDenseDesignMatrix(X, add_intercept=True, center_predictor=True)
    model = RegressionModel((y, e), dsn, 'negbin')
    Xt = pro.design_matrix(X, dsn.column_offset, True)
    want = nb.predict_explicit(Xt, coef, r, y, np.log(e))
    rec = nb.predict_recurrence(Xt, coef, r, y, np.log(e))
    got = model.predict(coef, r, return_draws=True)
    for key in pro.KEYS:
        print('%-11s oracle f64 vs ext %.2e   device vs ext %.2e   tol %.0e'
              % (key, pro.rel_err(rec[key], want[key]),
                 pro.rel_err(got[key], want[key]), PREDICT_TOL[key]))
    for key in pro.KEYS:
        assert pro.within(rec[key], want[key], PREDICT_TOL[key]), key
    for key in pro.KEYS:
        assert got[key].shape == (len(y),)
        assert pro.within(got[key], want[key], PREDICT_TOL[key]), key
    assert pro.within(got['draws'], want['mu'], PREDICT_TOL['mean'])
    lppd, p_waic, waic = pro.waic(want)
    for key, value in (('lppd', lppd), ('p_waic', p_waic), ('waic', waic)):
        np.testing.assert_allclose(got[key], float(value), rtol=1e-12)
    # no result depends on the draws per pass
    for K in (1, 5, 16, 37, 64):
        other = model.predict(coef, r, return_draws=True, _draws_per_pass=K)
        assert set(other) == set(got)
        for key in got:
            assert np.array_equal(other[key], got[key]), (K, key)
    # a scalar dispersion is that value for every draw; new rows without an
    # outcome give the means only
    one = model.predict(coef, 3.)
    same = model.predict(coef, np.full(coef.shape[1], 3.))
    for key in one:
        assert np.array_equal(one[key], same[key]), key
    new = model.predict(coef, r, X_new=X, exposure_new=e)
    assert set(new) == {'mean', 'sd'}
    assert np.array_equal(new['mean'], got['mean'])
    scored = model.predict(coef, r, X_new=X, exposure_new=e, y_new=y)
    assert np.array_equal(scored['lpd'], got['lpd'])
    # the Poisson limit: at r = 1e12 the scores are the Poisson model's
    poisson = RegressionModel((y, e), dsn, 'poisson').predict(coef)
    limit = model.predict(coef, 1e12)
    np.testing.assert_allclose(limit['lpd'], poisson['lpd'], rtol=1e-6,
                               atol=1e-6)
    for bad in (np.ones(3), -1., np.inf, np.full(coef.shape[1], np.nan)):
        with pytest.raises(ValueError):
            model.predict(coef, bad)


def test_the_shared_summary_still_refuses_family_3():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    design = HipDenseDesignMatrix(rs.randn(40, 3))
    coef, y = rs.randn(2, 4) * .1, np.ones(40)
    out = [np.empty(40) for _ in range(5)]
    st = lib.bbx_design_predictive_summary(
        design.handle, 3, 2, _ptr(coef), None, None, _ptr(y), None, None, 0,
        *[_ptr(a) for a in out], None)
    assert st == -1 and 'family 3' in _lib.last_error()
    # the family's own call refuses what it must, with the design usable
    r = np.array([1., 2.])
    for bad_r in (None, np.array([1., 0.]), np.array([1., np.inf])):
        assert lib.bbx_design_predictive_summary_negbin(
            design.handle, 2, _ptr(coef), _ptr(bad_r), None, _ptr(y), None, 0,
            *[_ptr(a) for a in out], None) == -1
        assert 'dispersion' in _lib.last_error()
    assert lib.bbx_design_predictive_summary_negbin(
        design.handle, 2, _ptr(coef), _ptr(r), None, _ptr(y), None, 0,
        _ptr(out[0]), _ptr(out[1]), None, None, None, None) == -1
    assert lib.bbx_design_predictive_summary_negbin(
        design.handle, 2, _ptr(coef), _ptr(r), None, _ptr(y), None, 0,
        *[_ptr(a) for a in out], None) == 0
    assert np.all(np.isfinite(out[2]))


def test_c_abi_errors_are_status_codes():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    n, p = 50, 4
    design = HipDenseDesignMatrix(rs.randn(n, p))
    P = p + 1
    y, o = np.ones(n), np.full(n, .5)
    vec, out = rs.randn(P) * .1, np.empty(P)
    ll, k = c_double(), c_int()
    null = c_void_p()
    assert lib.bbx_negbin_loglik_grad(null, _ptr(vec), byref(ll), None) < 0
    assert lib.bbx_negbin_set_location(null, _ptr(vec)) < 0
    assert lib.bbx_negbin_set_dispersion(null, 1.) < 0
    assert lib.bbx_negbin_destroy(null) == 0
    # bad arguments at create
    h = c_void_p()
    assert lib.bbx_negbin_create(design.handle, _ptr(y), _ptr(o), 1., None) < 0
    assert lib.bbx_negbin_create(null, _ptr(y), _ptr(o), 1., byref(h)) < 0
    assert lib.bbx_negbin_create(design.handle, None, _ptr(o), 1.,
                                 byref(h)) < 0
    at = np.arange(n)
    for bad_y, bad_o, bad_r in (
            (np.where(at == 7, -1., y), o, 1.),
            (np.where(at == 7, np.nan, y), o, 1.),
            (np.where(at == 7, np.inf, y), o, 1.),
            (y, np.where(at == 9, np.inf, o), 1.),
            (y, np.where(at == 9, np.nan, o), 1.),
            (y, o, 0.), (y, o, -1.), (y, o, np.inf), (y, o, np.nan)):
        bad_y, bad_o = np.ascontiguousarray(bad_y), np.ascontiguousarray(bad_o)
        assert lib.bbx_negbin_create(design.handle, _ptr(bad_y), _ptr(bad_o),
                                     bad_r, byref(h)) == -1
        assert not h.value
        assert _lib.last_error()
    # no offset: log_exposure = NULL
    h0 = c_void_p()
    assert lib.bbx_negbin_create(design.handle, _ptr(y), None, 2.,
                                 byref(h0)) == 0
    assert lib.bbx_negbin_create(design.handle, _ptr(y), _ptr(o), 2.,
                                 byref(h)) == 0
    # order of calls
    assert lib.bbx_negbin_hessian_matvec(h, _ptr(vec), _ptr(out)) == -5
    assert 'set_location' in _lib.last_error()
    u = rs.rand(1)
    assert lib.bbx_negbin_nuts_doubling(h, .1, 1, 0, _ptr(u), byref(k),
                                        byref(k), None, None, None) < 0
    assert 'nuts_begin' in _lib.last_error()
    rr, L = np.array([1., 2., 4.]), np.empty(8)
    assert lib.bbx_negbin_dispersion_loglik(h, None, 3, _ptr(rr),
                                            _ptr(L)) == -5
    assert 'cached' in _lib.last_error()
    for n_r in (0, 9, -1):
        assert lib.bbx_negbin_dispersion_loglik(h, _ptr(vec), n_r, _ptr(rr),
                                                _ptr(L)) == -1
    for bad in (0., -1., np.inf, np.nan):
        bad_rr = np.array([1., bad, 4.])
        assert lib.bbx_negbin_dispersion_loglik(h, _ptr(vec), 3, _ptr(bad_rr),
                                                _ptr(L)) == -1
        assert 'r[1]' in _lib.last_error()
        assert lib.bbx_negbin_set_dispersion(h, bad) == -1
    assert lib.bbx_negbin_dispersion_loglik(h, _ptr(vec), 3, None,
                                            _ptr(L)) == -1
    # a refused call with beta cached nothing
    assert lib.bbx_negbin_dispersion_loglik(h, None, 3, _ptr(rr),
                                            _ptr(L)) == -5
    assert lib.bbx_negbin_dispersion_loglik(h, _ptr(vec), 3, _ptr(rr),
                                            _ptr(L)) == 0
    assert lib.bbx_negbin_dispersion_loglik(h, None, 3, _ptr(rr),
                                            _ptr(L)) == 0
    assert np.all(np.isfinite(L[:3]))
    # the design and the handles work afterwards
    ll0 = c_double()
    assert lib.bbx_negbin_loglik_grad(h0, _ptr(vec), byref(ll0), None) == 0
    assert lib.bbx_negbin_loglik_grad(h, _ptr(vec), byref(ll), _ptr(out)) == 0
    assert np.isfinite(ll.value) and ll.value != ll0.value
    assert lib.bbx_negbin_set_dispersion(h, 5.) == 0
    assert lib.bbx_negbin_loglik_grad(h, _ptr(vec), byref(ll0), None) == 0
    assert ll0.value != ll.value
    assert lib.bbx_negbin_destroy(h0) == 0
    # use after the design is destroyed
    design.__del__()
    assert lib.bbx_negbin_loglik_grad(h, _ptr(vec), byref(ll), None) < 0
    assert 'destroyed' in _lib.last_error()
    assert lib.bbx_negbin_set_dispersion(h, 1.) < 0
    assert lib.bbx_negbin_destroy(h) == 0
