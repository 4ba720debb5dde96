"""GPU: the 'hmc' and 'nuts' coefficient samplers of the logit model
(csrc/logit.hip, csrc/hamiltonian.hpp) -- the likelihood, its gradient and
Hessian matvec against the NumPy oracle (tests/logit_oracle.py), the
trajectory against a host velocity Verlet, single No-U-Turn draws and seeded
chains against the reference's fixtures (tests/golden/
make_logit_hmc_golden.py), and the refusals."""
import os
import warnings
from ctypes import byref, c_double, c_int, c_void_p

import numpy as np
import pytest
import scipy.sparse as sparse

import logit_oracle as lo
import nuts_oracle as no

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9          # the seeded Hamiltonian chains' tolerance


def _logit_data(kind, n, p, intercept=True, center=True, multi_trial=False,
                seed=0):
    """A device logit model, the oracle's design and the counts."""
    from bayesbridge_amd import (HipDenseDesignMatrix, HipSparseDesignMatrix,
                                 RegressionModel, simulate)
    rs = np.random.RandomState(seed)
    density = .05 if p <= 1000 else 20. / p
    if kind == 'tiled_binary':
        X = simulate.simulate_binary_csr_fast(n, p, density, seed=seed)
    elif kind == 'csr_valued':
        X = sparse.random(n, p, density=density, format='csr',
                          random_state=rs)
    elif kind == 'mixed':
        X = simulate.simulate_design_csr(n, p, binary_frac=.9, seed=seed)
    else:
        X = rs.randn(n, p)
    beta = np.zeros(p)
    beta[:10] = rs.randn(10)
    m = rs.randint(1, 4, n) if multi_trial else np.ones(n, dtype=int)
    y = rs.binomial(m, 1 / (1 + np.exp(-np.asarray(X.dot(beta)).ravel())))
    y, m = y.astype(np.float64), m.astype(np.float64)
    if kind in ('tiled_binary', 'mixed'):
        dsn = HipSparseDesignMatrix(X, add_intercept=intercept,
                                    center_predictor=center, storage='tiled')
    elif kind == 'csr_valued':
        dsn = HipSparseDesignMatrix(X, add_intercept=intercept,
                                    center_predictor=center, storage='csr')
    else:
        dtype = 'float32' if kind == 'dense32' else 'float64'
        dsn = HipDenseDesignMatrix(X, add_intercept=intercept,
                                   center_predictor=center,
                                   storage_dtype=dtype)
    assert dsn.shape == (n, p + int(intercept))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((y, m), dsn, 'logit')
    if kind == 'dense32':
        # float32 storage holds the CENTRED entries rounded to float32
        if center:
            X = X - dsn.column_offset
        X = X.astype(np.float32).astype(np.float64)
        return model, lo.design(X, False, intercept), y, m
    D = lo.design(X, center, intercept,
                  offset=dsn.column_offset if center else None)
    return model, D, y, m


# (kind, n, p, add_intercept, center_predictor)
CASES = [(kind, 3000, 200, True, True) for kind in (
    'tiled_binary', 'csr_valued', 'dense64', 'dense32', 'mixed')] + [
    ('dense64', 3000, 200, False, True), ('dense64', 3000, 200, True, False),
    ('tiled_binary', 3000, 200, False, True),
    ('tiled_binary', 3000, 200, True, False),
    ('dense64', 100, 20, True, True),           # most workgroups get no row
    ('dense32', 65536, 64, True, True),         # one lap of NPART x VEC_BLOCK
    ('dense32', 70001, 300, True, True),        # second lap, ragged; P > 256
    ('tiled_binary', 200000, 5000, True, True)]  # P over many workgroups


@pytest.mark.parametrize('case', range(len(CASES)))
def test_likelihood_gradient_hessian_match_the_oracle(case):
    kind, n, p, intercept, center = CASES[case]
    model, D, y, m = _logit_data(kind, n, p, intercept, center,
                                 multi_trial=case % 2 == 1)
    assert (m.max() > 1) == (case % 2 == 1)
    P = p + int(intercept)
    tol, htol = 1e-11, 1e-10
    rs = np.random.RandomState(1)
    betas = [rs.randn(P) * .1, rs.randn(P)]
    # saturated probabilities, exp(-eta) = inf: |eta| up to 720
    b = rs.randn(P)
    betas.append(b * (720. / np.abs(lo.dot(D, b)).max()))
    for k, beta in enumerate(betas):
        v = rs.randn(P)
        ll, grad = model.hamiltonian_loglik_and_gradient(beta)
        oll, ograd = lo.loglik_grad(D, y, m, beta)
        print(kind, n, p, 'case', k, 'max|eta| %.3g' %
              np.abs(lo.dot(D, beta)).max(), 'loglik rel %.2e'
              % (abs(ll - oll) / abs(oll)), 'grad %.2e'
              % (np.abs(grad - ograd).max() / np.abs(ograd).max()))
        assert np.isfinite(ll) and np.isfinite(oll)
        assert abs(ll - oll) <= tol * abs(oll)
        assert np.abs(grad - ograd).max() <= tol * np.abs(ograd).max()
        ll2, grad2 = model.hamiltonian_loglik_and_gradient(beta)
        assert ll2 == ll and np.array_equal(grad2, grad)
        if k == 2:
            assert np.abs(lo.dot(D, beta)).max() > 709.8
            continue
        hv = model.get_hessian_matvec_operator(beta)(v)
        ohv = lo.hessian_matvec(D, y, m, beta, v)
        print('   hessian %.2e' % (np.abs(hv - ohv).max() / np.abs(ohv).max()))
        assert np.abs(hv - ohv).max() <= htol * np.abs(ohv).max()
        hv2 = model.get_hessian_matvec_operator(beta)(v)
        assert np.array_equal(hv2, hv)
    ll, none = model.hamiltonian_loglik_and_gradient(beta, loglik_only=True)
    assert none is None and ll == model.hamiltonian_loglik_and_gradient(beta)[0]
    # the samplers that do not use the handle keep the host likelihood
    host = model.compute_loglik_and_gradient(betas[1])
    assert host[0] == pytest.approx(
        model.hamiltonian_loglik_and_gradient(betas[1])[0], rel=1e-11)


def test_an_operator_stops_once_the_location_has_moved():
    model, D, y, m = _logit_data('dense64', 100, 20)
    rs = np.random.RandomState(2)
    op = model.get_hessian_matvec_operator(rs.randn(21))
    op(rs.randn(21))
    model.get_hessian_matvec_operator(rs.randn(21))
    with pytest.raises(RuntimeError, match='location has moved'):
        op(rs.randn(21))


def _traj_inputs(D, y, m, seed=0):
    P = D[0].shape[1] + int(D[2])
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.randn(P) * .3) * .3
    prior_prec = np.ones(P)
    f = lo.precond_f(D, y, m, scale, prior_prec)
    q0 = rs.randn(P) * .1
    p0 = rs.randn(P)
    logp0, grad0 = f(q0)
    return f, scale, prior_prec, q0, p0, logp0, grad0


@pytest.mark.parametrize('kind', ['tiled_binary', 'dense64'])
def test_trajectory_matches_host_velocity_verlet(kind):
    """The intercept column and the centring are live here: step1's offset
    partials and the sum-of-w partials of X~^T w."""
    model, D, y, m = _logit_data(kind, 3000, 200, multi_trial=True)
    f, scale, pp, q0, p0, logp0, grad0 = _traj_inputs(D, y, m)
    # the stability limit of the leapfrog map is 2 / sqrt(largest curvature
    # of -f); the curvature at q0 by power iteration on the oracle's Hessian
    v = np.ones(len(q0))
    for _ in range(30):
        hv = pp * v - scale * lo.hessian_matvec(D, y, m, q0 * scale, scale * v)
        curvature = np.linalg.norm(hv) / np.linalg.norm(v)
        v = hv / np.linalg.norm(hv)
    limit = 2 / np.sqrt(curvature)
    dt, dt_unstable = limit / 4, 10 * limit
    print('stability limit', limit)
    want = lo.trajectory(f, dt, 25, q0, p0, logp0, grad0)
    got = model.hmc_trajectory(dt, 25, scale, pp, q0, p0, logp0, grad0)
    assert not want[5] and not got['instability']
    assert got['n_steps'] == want[4] == 25
    for key, ref in (('q', want[0]), ('p', want[1]), ('grad', want[3])):
        print(key, np.abs(got[key] - ref).max() / np.abs(ref).max())
        assert np.abs(got[key] - ref).max() <= 1e-9 * np.abs(ref).max()
    assert got['logp'] == pytest.approx(want[2], rel=1e-9)
    assert got['hamiltonian'][0] == pytest.approx(want[6], rel=1e-9)
    assert got['hamiltonian'][1] == pytest.approx(want[7], rel=1e-9)
    again = model.hmc_trajectory(dt, 25, scale, pp, q0, p0, logp0, grad0)
    for key in ('q', 'p', 'grad', 'hamiltonian'):
        assert np.array_equal(again[key], got[key])
    assert again['logp'] == got['logp']
    # a step size far past the stability limit: the device stops at the host
    # loop's step, and where it stopped.  (The steps before the stop multiply
    # a rounding difference by up to dt^2 x curvature each; the chain
    # tolerance covers the few there are.)
    # (the logit gradient is bounded, so H saturates instead of diverging:
    # the default tolerance of 100 trips at once, 1e6 after a few steps)
    for tol in (100., 1e6):
        with np.errstate(all='ignore'):
            want = lo.trajectory(f, dt_unstable, 200, q0, p0, logp0, grad0,
                                 tol=tol)
        got = model.hmc_trajectory(dt_unstable, 200, scale, pp, q0, p0, logp0,
                                   grad0, tol)
        print('unstable: tol', tol, 'steps', got['n_steps'], want[4],
              'max|dq|', np.abs(got['q'] - want[0]).max())
        assert got['instability'] == want[5]
        assert got['n_steps'] == want[4]
        np.testing.assert_allclose(got['q'], want[0], rtol=RTOL, atol=ATOL)
        if tol == 100.:
            assert want[5] and want[4] < 200
    # the skip flag was the trajectory's only
    ll, grad = model.hamiltonian_loglik_and_gradient(q0 * scale)
    assert ll + np.sum(-pp * q0 ** 2) / 2 == pytest.approx(logp0, rel=1e-11)


def _draw(model, seed, dt, q, p, scale, pp, max_height, tol=100.):
    from bayesbridge_amd import nuts
    np.random.seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return nuts.generate_next_state(
            model, dt, q, scale, pp, p=p, max_height=max_height,
            hamiltonian_error_tol=tol)


def _fixture_model(X, y, m, fmt):
    from bayesbridge_amd import RegressionModel
    if fmt == 'sparse':
        X = sparse.csr_matrix(X)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return RegressionModel((y, m), X, 'logit')


def test_single_draws_reproduce_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, 'logit_nuts_calls.npz'))
    kinds, n = set(), 0
    for fmt in ('dense', 'sparse'):
        problem = 'chain_' + fmt
        model = _fixture_model(g[problem + '_X'], g[problem + '_n_success'],
                               g[problem + '_n_trial'], fmt)
        scale, pp = g[problem + '_scale'], g[problem + '_prior_prec']
        for k in range(int(g['n_call'])):
            pre = 'call%03d_' % k
            if str(g[pre + 'problem']) != problem:
                continue
            n += 1
            q, info = _draw(model, int(g[pre + 'seed']), float(g[pre + 'dt']),
                            g[pre + 'q'], g[pre + 'p'], scale, pp,
                            int(g[pre + 'max_height']), float(g[pre + 'tol']))
            what = (k, float(g[pre + 'dt']))
            print(what, 'height', info['tree_height'], 'steps',
                  info['n_grad_evals'], 'uniforms', info['n_uniform'],
                  'max|dq|', np.abs(q - g[pre + 'q_out']).max())
            np.testing.assert_array_equal(info['directions'],
                                          g[pre + 'directions'])
            assert info['tree_height'] == int(g[pre + 'tree_height']), what
            assert info['n_grad_evals'] == int(g[pre + 'n_grad_evals']), what
            assert info['n_uniform'] == int(g[pre + 'n_uniform']), what
            for key in ('u_turn_detected', 'instability_detected',
                        'last_doubling_rejected'):
                assert info[key] == bool(g[pre + key]), (what, key)
            # the stream is where the reference leaves it
            assert np.random.rand() == float(g[pre + 'next_number']), what
            np.testing.assert_allclose(q, g[pre + 'q_out'], rtol=RTOL,
                                       atol=ATOL)
            np.testing.assert_allclose(info['grad'], g[pre + 'grad'],
                                       rtol=RTOL, atol=ATOL)
            np.testing.assert_allclose(info['logp'], float(g[pre + 'logp']),
                                       rtol=RTOL, atol=ATOL)
            for key in ('ave_accept_prob', 'ave_hamiltonian_error'):
                assert info[key] == pytest.approx(float(g[pre + key]),
                                                  rel=1e-9), (what, key)
            maxed = info['tree_height'] >= int(g[pre + 'max_height']) \
                and not info['u_turn_detected']
            kinds |= {name for name, hit in (
                ('u_turn_inside', info['u_turn_detected']
                 and info['last_doubling_rejected']),
                ('u_turn_top', info['u_turn_detected']
                 and not info['last_doubling_rejected']),
                ('maxed', maxed),
                ('instability', info['instability_detected'])) if hit}
    assert n == int(g['n_call']) >= 40
    assert kinds == {'u_turn_inside', 'u_turn_top', 'maxed', 'instability'}


def test_a_draw_with_reductions_over_many_workgroups_matches_the_restatement():
    """P = 5001: the P-length kernels run 20 workgroups; n = 200 000: three
    laps of the row kernel.  The restated recursion runs on the oracle."""
    model, D, y, m = _logit_data('tiled_binary', 200000, 5000)
    P = 5001
    rs = np.random.RandomState(1)
    scale, pp = np.exp(rs.randn(P) * .3) * .05, np.ones(P)
    f = lo.precond_f(D, y, m, scale, pp)
    q0, p0 = rs.randn(P) * .1, rs.randn(P)
    dt, max_height = .02, 5
    q, info = _draw(model, 70, dt, q0, p0, scale, pp, max_height)
    np.random.seed(70)
    wq, want = no.generate_next_state(f, dt, q0, *f(q0), p=p0,
                                      max_height=max_height)
    print('height', info['tree_height'], want['tree_height'], 'steps',
          info['n_grad_evals'], want['n_grad_evals'], 'u-turn',
          info['u_turn_detected'], 'max|dq|', np.abs(q - wq).max())
    assert info['tree_height'] == want['tree_height'] >= 3
    assert info['n_grad_evals'] == want['n_grad_evals'] + 1
    assert info['n_uniform'] == want['n_uniform']
    for key in ('u_turn_detected', 'instability_detected',
                'last_doubling_rejected'):
        assert info[key] == want[key]
    np.testing.assert_allclose(q, wq, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(info['grad'], want['grad'], rtol=RTOL,
                               atol=ATOL)
    for key in ('ave_accept_prob', 'ave_hamiltonian_error'):
        assert info[key] == pytest.approx(want[key], rel=1e-9)
    q2, info2 = _draw(model, 70, dt, q0, p0, scale, pp, max_height)
    assert np.array_equal(q2, q) and np.array_equal(info2['grad'],
                                                    info['grad'])


def _chain(golden_dir, method, fmt, n_iter=None, resume=None):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior
    g = np.load(os.path.join(golden_dir,
                             'chain_logit_%s_%s.npz' % (method, fmt)))
    model = _fixture_model(g['X'], g['n_success'], g['n_trial'], fmt)
    prior = RegressionCoefPrior(sd_for_intercept=2., regularizing_slab_size=1.,
                                bridge_exponent=.25)
    init = {'global_scale': 0.1, 'local_scale': np.ones(g['X'].shape[1])}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        samples, info = BayesBridge(model, prior).gibbs(
            n_iter or int(g['n_iter']), init=init, seed=int(g['seed']),
            params_to_save='all', coef_sampler_type=method,
            options={'rng': 'reference'})
        if resume:
            samples, info = BayesBridge(model, prior).gibbs_resume(
                info, resume, merge=True, prev_samples=samples)
    return g, samples, info


@pytest.mark.parametrize('method,fmt', [('hmc', 'dense'), ('hmc', 'sparse'),
                                        ('nuts', 'dense'), ('nuts', 'sparse')])
def test_seeded_chain_reproduces_the_reference(golden_dir, method, fmt):
    from bayesbridge_amd.bayesbridge import HMC_INFO_KEYS, NUTS_INFO_KEYS
    g, samples, info = _chain(golden_dir, method, fmt)
    n_iter = int(g['n_iter'])
    assert n_iter >= 10
    assert info['coef_sampler_type'] == method
    assert info['options']['coef_sampler_type'] == method
    assert info['options']['rng'] == 'reference'
    si = info['_reg_coef_sampling_info']
    assert set(si) == set(HMC_INFO_KEYS if method == 'hmc'
                          else NUTS_INFO_KEYS)
    assert 'n_cg_iter' not in si
    steps = 'n_integrator_step' if method == 'hmc' else 'tree_height'
    print(steps, si[steps], 'n_grad_evals', si['n_grad_evals'], 'max rel coef',
          np.max(np.abs(samples['coef'] - g['samples_coef'])
                 / (np.abs(g['samples_coef']) + 1e-3)))
    assert len(si[steps]) == n_iter
    integer = (steps, 'n_grad_evals', 'n_hessian_matvec',
               'instability_detected') + (('accepted',) if method == 'hmc'
                                          else ())
    for key in integer:
        np.testing.assert_array_equal(si[key], g['info_' + key])
    accept = 'accept_prob' if method == 'hmc' else 'ave_accept_prob'
    for key in ('stepsize', 'stability_limit_est', accept):
        np.testing.assert_allclose(si[key], g['info_' + key], rtol=RTOL)
    assert samples['obs_prec'].shape == g['samples_obs_prec'].shape
    for key in ('coef', 'local_scale', 'global_scale', 'logp', 'obs_prec'):
        np.testing.assert_allclose(samples[key], g['samples_' + key],
                                   rtol=RTOL, atol=ATOL)
    # two halves through gibbs_resume equal the straight run bit for bit
    half = n_iter // 2
    _, resumed, rinfo = _chain(golden_dir, method, fmt, half,
                               resume=n_iter - half)
    for key in samples:
        np.testing.assert_array_equal(resumed[key], samples[key])
    for key in si:
        np.testing.assert_array_equal(rinfo['_reg_coef_sampling_info'][key],
                                      si[key])


def test_refusals_are_exceptions(golden_dir):
    from bayesbridge_amd import BayesBridge, RegressionCoefPrior, RegressionModel
    model, D, y, m = _logit_data('dense64', 100, 20)
    bridge = BayesBridge(model, RegressionCoefPrior(bridge_exponent=.5))
    init = {'global_scale': .1}
    for method in ('hmc', 'nuts'):
        with pytest.raises(ValueError, match="'rng': 'reference'"):
            bridge.gibbs(2, init=init, seed=0, coef_sampler_type=method)
        with pytest.raises(ValueError):
            bridge.gibbs(2, init=init, seed=0, coef_sampler_type=method,
                         options={'rng': 'device'})
        with pytest.raises(ValueError):
            bridge.gibbs_batch([0, 1], 2, init=init, options={
                'coef_sampler_type': method, 'rng': 'reference'})
        with pytest.raises(ValueError):
            bridge.gibbs_multichain(2, 2, init=init, options={
                'coef_sampler_type': method, 'rng': 'reference'})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        linear = RegressionModel(np.random.RandomState(0).randn(100),
                                 model.design, 'linear')
    for options in (None, {'rng': 'reference'}):
        with pytest.raises(ValueError):
            BayesBridge(linear).gibbs(2, init=init, seed=0,
                                      coef_sampler_type='hmc',
                                      options=options)


def _ptr(a):
    return a.ctypes.data_as(c_void_p)


def test_c_abi_errors_are_status_codes():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    rs = np.random.RandomState(0)
    n, p = 50, 4
    design = HipDenseDesignMatrix(rs.randn(n, p))
    P = p + 1
    y, m = np.ones(n), np.full(n, 2.)
    vec, out = rs.randn(P), np.empty(P)
    ll, k = c_double(), c_int()
    # NULL handle
    null = c_void_p()
    assert lib.bbx_logit_loglik_grad(null, _ptr(vec), byref(ll), None) < 0
    assert lib.bbx_logit_set_location(null, _ptr(vec)) < 0
    assert lib.bbx_logit_hessian_matvec(null, _ptr(vec), _ptr(out)) < 0
    assert lib.bbx_logit_nuts_sample(null, None, byref(ll), None) < 0
    assert lib.bbx_logit_destroy(null) == 0
    # bad arguments at create
    h = c_void_p()
    assert lib.bbx_logit_create(design.handle, _ptr(y), _ptr(m), None) < 0
    assert lib.bbx_logit_create(null, _ptr(y), _ptr(m), byref(h)) < 0
    assert lib.bbx_logit_create(design.handle, None, _ptr(m), byref(h)) < 0
    for bad_y, bad_m in ((y, np.where(np.arange(n) == 3, 0., m)),
                         (y, np.where(np.arange(n) == 3, -1., m)),
                         (np.where(np.arange(n) == 7, 3., y), m),
                         (np.where(np.arange(n) == 7, -1., y), m),
                         (np.where(np.arange(n) == 7, np.nan, y), m),
                         (y, np.where(np.arange(n) == 9, np.inf, m))):
        bad_y, bad_m = np.ascontiguousarray(bad_y), np.ascontiguousarray(bad_m)
        assert lib.bbx_logit_create(design.handle, _ptr(bad_y), _ptr(bad_m),
                                    byref(h)) < 0
        assert not h.value
        assert _lib.last_error()
    assert lib.bbx_logit_create(design.handle, _ptr(y), _ptr(m),
                                byref(h)) == 0
    # order of calls
    assert lib.bbx_logit_hessian_matvec(h, _ptr(vec), _ptr(out)) < 0
    assert 'set_location' in _lib.last_error()
    u = rs.rand(1)
    assert lib.bbx_logit_nuts_doubling(h, .1, 1, 0, _ptr(u), byref(k),
                                       byref(k), None, None, None) < 0
    assert 'nuts_begin' in _lib.last_error()
    assert lib.bbx_logit_nuts_sample(h, None, byref(ll), None) < 0
    assert lib.bbx_logit_hmc_trajectory(
        h, .1, -1, _ptr(vec), _ptr(vec), _ptr(vec), _ptr(vec), 0., _ptr(vec),
        100., None, None, None, None, None, None, None) < 0
    assert lib.bbx_logit_loglik_grad(h, _ptr(vec), byref(ll), _ptr(out)) == 0
    assert np.isfinite(ll.value)
    # use after the design is destroyed
    design.__del__()
    assert lib.bbx_logit_loglik_grad(h, _ptr(vec), byref(ll), None) < 0
    assert 'destroyed' in _lib.last_error()
    assert lib.bbx_logit_destroy(h) == 0
