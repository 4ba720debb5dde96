"""GPU: the censored-outcome model (family='tobit', family='lognormal') on the
Gaussian samplers -- csrc/censored.hip (the latents), the censored branches of
csrc/chain.hip, csrc/censored_predict.hip and the Python layers above them.

  the stand-alone latent kernel against the host replay, draw by draw;
  four chain iterations on three designs against the oracle: tau, the latents,
    zbase = X~^T z, the coefficient draw, the log-likelihood, the refresh;
  the three coefficient samplers against the NumPy chain
    (tests/censored_oracle.py), with a linear chain on the bounds as the
    negative control;
  no censored row is the linear model; resume, repeatability; prediction and
    the survival summary against a long-double oracle; the C ABI's refusals.
Tolerances: tests/censored_cases.py (measured on the CPU by
tests/test_censored_replay_cpu.py) and tests/replay_cases.py."""
import math
from ctypes import byref, c_void_p

import numpy as np
import pytest

import oracle
from oracle.summarizer import CoefSummarizer, regularized_prior_scale

import censored_cases as K
import censored_oracle as O
import probit_cases as P
import replay_cases as C
from bayesbridge_amd import replay as R

pytestmark = pytest.mark.gpu

ALPHA, SLAB = .5, 2.
ERR_INVALID = -1


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _device_censored_normal(seed, psi, bound, status, tau):
    from bayesbridge_amd import _lib
    out = np.empty(psi.size)
    _lib.check(_lib.load().bbx_device_censored_normal(
        0, seed, psi.size, _ptr(psi), _ptr(bound), _ptr(status), float(tau),
        _ptr(out)))
    return out


# ------------------------------------------------ the stand-alone kernel

@pytest.mark.parametrize("case", K.CN_CASES,
                         ids=[K.case_id(c) for c in K.CN_CASES])
def test_device_censored_normal_equals_the_replay(case):
    seed, tau = K.CN_SEEDS[case], case[3]
    psi, bound, status, bad = K.cn_inputs(case)
    dev = _device_censored_normal(seed, psi, bound, status, tau)
    rep, trials = R.censored_normal(seed, R.STREAM_LATENT, psi, bound, status,
                                    tau, 0, trace=True)
    obs, right, left = (status == s for s in (0, 1, 2))
    # observed rows are their values bit for bit, whatever psi is
    assert np.array_equal(dev[obs], bound[obs])
    cens_bad = bad[status[bad] != 0]
    assert np.all(np.isnan(dev[cens_bad])) and np.all(np.isnan(rep[cens_bad]))
    K.compare("censored normal %s" % K.case_id(case), dev, rep, psi, bound,
              status, tau, K.CN_TOL, lambda i: "psi %.17g b %.17g status %d "
              "trials %d" % (psi[i], bound[i], status[i], trials[i]))
    ok = np.isfinite(psi)
    # the side and the boundary convention
    assert np.all(dev[ok & right] > bound[ok & right])
    assert np.all(dev[ok & left] <= bound[ok & left])
    # an included draw was accepted at the replay's trial: shown directly by
    # replaying the 64 longest included draws' own trial
    d = K.difference(dev, rep, psi, bound, status, tau)
    p = K.scaled(psi, bound, tau)
    included = np.flatnonzero(ok & ~obs & (d <= K.CN_TOL))
    assert included.size >= (ok & ~obs).sum() - C.cap(case[0])
    probe = included[np.argsort(trials[included])[-64:]]    # the longest
    u_dev = K.to_u(dev, bound, tau)
    for i in probe:
        u = R.uniform(seed, R.STREAM_LATENT, int(i), int(trials[i]) - 1, 2)
        if P.regime(p[i:i + 1], right[i:i + 1])[0]:
            lam = .5 * abs(p[i]) + .5 * math.hypot(p[i], 2.)
            own = -math.log(u[0]) / lam
        else:
            own = abs(p[i] + math.sqrt(-2. * math.log(u[0]))
                      * math.cos(2. * math.pi * u[1]))
        # (1e-9, plus what an ulp of b is in u's units)
        slack = 1e-9 * max(1., abs(p[i]), own) \
            + 2. ** -51 * abs(bound[i]) * math.sqrt(tau)
        assert abs(abs(u_dev[i]) - own) <= slack, (i, trials[i])


# ------------------------------------------------------ one chain iteration

def _problem(kind, n=3000, p=200, seed=3):
    """(X, bound, status): about 35 % right-censored and 5 % left-censored."""
    from bayesbridge_amd import simulate
    rng = np.random.default_rng(seed)
    if kind == 'dense':
        X = rng.standard_normal((n, p))
    else:
        X = simulate.simulate_design_csr(n, p, binary_frac=.8,
                                         binary_pred_freq=.1, seed=seed)
    beta = np.zeros(p)
    beta[:5], beta[5:10] = 1.5, -1.
    rng = np.random.default_rng(seed + 1)
    z = .3 + np.asarray(X.dot(beta)).ravel() + rng.standard_normal(n)
    sd = z.std()
    upper = z.mean() + sd * (.385 + rng.standard_normal(n))   # P(z > upper) ~ .39
    lower = z.mean() - 1.85 * sd
    status = np.where(z <= lower, 2, np.where(z > upper, 1, 0)) \
        .astype(np.uint8)
    bound = np.where(status == 1, upper, np.where(status == 2, lower, z))
    return X, bound, status


def _hip_design(X, kind, storage):
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if kind == 'dense':
        return HipDenseDesignMatrix(X, center_predictor=True,
                                    add_intercept=True, storage_dtype=storage)
    return HipSparseDesignMatrix(X, center_predictor=True, add_intercept=True,
                                 storage=storage)


def _log_prior(coef, gscale, nu, sd_unshrunk, shape0, rate0):
    """bayesbridge.py:480-511 without the likelihood."""
    lp = -.5 * np.sum((coef / SLAB) ** 2)
    beta = coef[nu:]
    lp += -beta.size * math.log(gscale) \
        - np.sum(np.abs(beta / gscale) ** ALPHA)
    lp += -.5 * np.sum((coef[:nu] / sd_unshrunk) ** 2)
    lp += -np.sum(np.log(sd_unshrunk[np.isfinite(sd_unshrunk)]))
    return lp + (shape0 - 1.) * math.log(gscale) - rate0 * gscale


@pytest.mark.parametrize("kind,storage", [('sparse', 'tiled'),
                                          ('dense', 'float64'),
                                          ('dense', 'float32')])
def test_chain_iteration_equals_oracle(kind, storage):
    """Four consecutive iterations, each compared with the oracle started from
    the device state before it (the pattern of test_hip_probit.py and
    test_hip_student_t.py, whose tolerances these are)."""
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, bound, status = _problem(kind)
    share = np.bincount(status, minlength=3) / len(status)
    assert .30 <= share[1] <= .40 and .03 <= share[2] <= .07, share
    hip = _hip_design(X, kind, storage)
    ora = oracle.make_design(X, add_intercept=True, center_predictor=True)
    seed, shape0, rate0 = 17, 1.5, .3
    sd_unshrunk = np.array([2.])
    chain = HipGibbsChain(hip, 'censored', bound, status=status,
                          sd_unshrunk=sd_unshrunk, bridge_exponent=ALPHA,
                          slab_size=SLAB, gscale_shape=shape0,
                          gscale_rate=rate0, seed=seed)
    n, P_ = hip.shape
    nu = 1
    # at creation z = b
    assert np.array_equal(chain.get_latent(), bound)
    rng = np.random.default_rng(5)
    chain.set_state(np.zeros(P_), .4, np.exp(rng.normal(0., 1., P_ - nu)),
                    .07)
    # The solves stop at 1e-9 sqrt(P), not at the chain's default 1e-5 sqrt(P):
    # with the default, the oracle's own draw on the sparse problem moves by
    # 1.9e-6 when its right-hand side is perturbed by 1e-15, and is 4.0e-6
    # from the converged one, on one weakly shrunk coefficient (local scale
    # 8.7) -- more than the rule below allows two solvers to differ.  At
    # 1e-9 sqrt(P) the same two figures are 4.3e-12 and 5.3e-10 (dense: 2.7e-11
    # and 2.1e-11), measured on the CPU at this test's starting state.
    atol = 1e-9 * np.sqrt(P_)
    f32 = storage == 'float32'
    lp_tol = 1e-7 if f32 else 1e-10
    scalar_tol = C.CHAIN_F32_TOL if f32 else C.CHAIN_SCALAR_TOL
    latent_tol = C.CHAIN_F32_TOL if f32 else K.CHAIN_LATENT_TOL
    obs = status == 0
    hip.reset_matvec_count()
    for it in range(4):
        coef_b, tau_b, ls_b, g_b = chain.get_state()
        assert isinstance(tau_b, float)
        mean_b, square_b, n_avg = chain.get_summary()
        assert n_avg == it and chain.iteration == it
        latent_b = chain.get_latent()
        # ---- zbase == X~^T z, to 1e-12 of the largest entry (with f32
        # storage: of the STORED operator; the oracle's differs from it by
        # CHAIN_F32_TOL)
        zbase = chain.get_zbase()
        z = ora.Tdot(latent_b)
        own = hip.Tdot(latent_b)
        assert np.abs(zbase - own).max() <= 1e-12 * np.abs(own).max()
        assert np.abs(zbase - z).max() <= \
            (C.CHAIN_F32_TOL if f32 else 1e-12) * np.abs(z).max()
        summ = CoefSummarizer(P_, nu, SLAB)
        summ.set_state({'mean': mean_b, 'square': square_b,
                        'n_averaged': n_avg})
        prior_sd = np.concatenate((
            sd_unshrunk, regularized_prior_scale(g_b, ls_b, SLAB)))
        phi = 1 / prior_sd
        x0 = summ.extrapolate_coef_condmean(g_b, ls_b)
        sd = summ.estimate_post_sd()
        eta1, eta2 = chain.eta(it)
        # the linear model's draw with z for y: Omega = tau, rhs tau X~^T z
        coef_o, info_o = oracle.cg_sample(ora, np.full(n, tau_b), phi,
                                          tau_b * z, x0, sd, nu, eta1, eta2,
                                          500, atol)
        # ---- one device iteration
        before = hip.get_dot_count()
        kept, n_unconv = chain.run(1, atol=atol,
                                   save=('coef', 'local_scale', 'obs_prec'))
        assert n_unconv == 0 and kept['obs_prec'].shape == (1, 1)
        coef_d = kept['coef'][0]
        n_cg = int(kept['n_cg_iter'][0])
        slack = max(2, math.ceil(.10 * info_o['n_iter']))
        assert abs(n_cg - info_o['n_iter']) <= slack, (n_cg, info_o['n_iter'])
        scale = max(1., np.abs(coef_o).max())
        tol = 1e-6 if n_cg == info_o['n_iter'] else 1e-5
        assert np.abs(coef_d - coef_o).max() <= tol * scale, \
            (it, np.abs(coef_d - coef_o).max())
        # counters: as a linear iteration, plus ONE X~^T w for zbase
        after = hip.get_dot_count()
        warm = 1 if np.any(x0 != 0.) else 0
        assert after[0] - before[0] == n_cg + warm + 1
        assert after[1] - before[1] == n_cg + 2
        # ---- tau: the Gamma variate over S / 2, S with the OLD latents and the
        # oracle's psi of the new coefficients
        coef_a, tau_a, ls_a, g_a = chain.get_state()
        assert np.array_equal(coef_a, coef_d)
        assert tau_a == float(kept['obs_prec'][0, 0])
        psi = ora.dot(coef_a)
        S = np.sum((latent_b - psi) ** 2)
        tau_o = R.gamma(seed, R.iter_stream(R.STREAM_OBSVAR, it), n / 2.)[0] \
            / (S / 2.)
        assert abs(tau_a - tau_o) <= scalar_tol * tau_o, (it, tau_a, tau_o)
        # ---- the new latents against the replay, with the device's tau
        latent_a = chain.get_latent()
        rep, trials = R.censored_normal(
            seed, R.iter_stream(R.STREAM_LATENT, it), psi, bound, status,
            tau_a, 0, trace=True)
        K.compare("%s/%s it %d latents" % (kind, storage, it), latent_a, rep,
                  psi, bound, status, tau_a, latent_tol,
                  lambda i: "psi %.17g b %.17g status %d trials %d"
                  % (psi[i], bound[i], status[i], trials[i]))
        assert np.array_equal(latent_a[obs], bound[obs])
        assert np.all(latent_a[status == 1] > bound[status == 1])
        assert np.all(latent_a[status == 2] <= bound[status == 2])
        # ---- log-likelihood and log posterior
        ll_d, lp_d = chain.logp()
        ll_o = O.loglik(psi, bound, status, tau_a)
        print("%s/%s it %d: tau %.6g, loglik %.10g (oracle %.10g), n_cg %d"
              % (kind, storage, it, tau_a, ll_d, ll_o, n_cg))
        assert abs(ll_d - ll_o) <= lp_tol * abs(ll_o), (ll_d, ll_o)
        lp_o = ll_o + _log_prior(coef_a, g_a, nu, sd_unshrunk, shape0, rate0)
        assert lp_d == float(kept['logp'][0])
        assert abs(lp_d - lp_o) <= lp_tol * abs(lp_o), (lp_d, lp_o)
    # ---- a state refresh (set_state with nothing to set) recomputes psi, the
    # latents, zbase and the log-likelihood of the last iteration bit for bit
    # and keeps tau
    latent, zbase, lp = chain.get_latent(), chain.get_zbase(), chain.logp()
    tau = chain.get_state()[1]
    chain.set_state()
    assert np.array_equal(chain.get_latent(), latent)
    assert np.array_equal(chain.get_zbase(), zbase)
    assert chain.logp() == lp and chain.get_state()[1] == tau
    chain.close()


# --------------------------------- the three samplers, one posterior

# device iterations per sampler, the first N_BURN dropped: 2000 for 'woodbury',
# whose draw solves an n x n system (400 x 400 here) with a host
# synchronisation per iteration, as in test_hip_probit.py
N_DEV = {'cg': 6000, 'cholesky': 6000, 'woodbury': 2000}
N_BURN = 500
_cache = {}


def _posterior_problem():
    if 'problem' not in _cache:
        bound, status, X = O.posterior_problem(K.POSTERIOR_DATA_SEED)
        ora = O.CensoredOracle(bound, status, X, ALPHA, 2., SLAB)
        # 4 x 5000 iterations of the NumPy chain, the first 500 of each dropped
        ref = [ora.run(5000, N_BURN, 100 + k) for k in range(4)]
        _cache['problem'] = (X, bound, status, ref)
    return _cache['problem']


def _device_draws(family, sampler, X, bound, status, seed):
    """[n_sample, P + 1]: the coefficients, then tau."""
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    kw = {'status': status} if family == 'censored' else {}
    chain = HipGibbsChain(hip, family, bound, sd_unshrunk=[2.],
                          bridge_exponent=ALPHA, slab_size=SLAB, seed=seed,
                          **kw)
    chain.set_coef_sampler(sampler)
    chain.set_state(np.zeros(hip.shape[1]), None, np.ones(hip.shape[1] - 1),
                    .1)
    chain.init_obs_prec()
    kept, n_unconv = chain.run(N_DEV[sampler], n_burnin=N_BURN,
                               save=('coef', 'obs_prec'))
    assert n_unconv == 0
    chain.close()
    return np.hstack((kept['coef'], kept['obs_prec']))


@pytest.mark.parametrize("sampler", ('cg', 'cholesky', 'woodbury'))
def test_every_sampler_draws_the_oracles_posterior(sampler):
    """N_DEV device iterations (500 dropped) against 4 x 5000 of the oracle:
    |z| < 4.5 on every ergodic mean and variance of the 13 coefficients and of
    tau, batch-means errors.  On the CPU, with this data seed (43 % of the
    rows right-censored), a second oracle run of 6000 iterations gave a largest
    z of 2.20 against the same reference, and the NumPy LINEAR chain on the
    bounds taken as observed 643.04 (on the intercept's mean; 545.6, 372.7 and
    365.0 on the next three moments)."""
    X, bound, status, ref = _posterior_problem()
    assert .35 <= status.mean() <= .45 and set(status) == {0, 1}
    draws = _device_draws('censored', sampler, X, bound, status, seed=31)
    z = O.z_scores([draws], ref)
    print("%s: largest z %.2f (moment %d)" % (sampler, z.max(), z.argmax()))
    assert z.shape == (28,) and np.all(np.isfinite(z))
    assert z.max() < 4.5


def test_a_linear_chain_on_the_bounds_fails_the_same_check():
    """The negative control: the bounds taken as observed pull the intercept
    and the slopes towards the censoring limits."""
    X, bound, status, ref = _posterior_problem()
    draws = _device_draws('linear', 'cg', X, bound, status, seed=31)
    z = O.z_scores([draws], ref)
    print("linear control: largest z %.2f; intercept %.3f against %.3f"
          % (z.max(), draws[:, 0].mean(),
             np.mean([r[:, 0].mean() for r in ref])))
    assert z.max() > 4.5


# --------------------------------------- no censored row: the linear model

def test_without_a_censored_row_the_chain_is_the_linear_models():
    """All status 0, one 'cholesky' iteration of a censored and of a linear
    chain from the same state and seed: the latents are y bit for bit, tau is
    equal (the same kernels on the same residuals), and the coefficient draws
    agree to K.RHS_ORDER_TOL of the largest coefficient -- 1000 x what two
    summation orders of X~^T y differ by on this data on the CPU: zbase = X~^T
    z is formed through another fold of the centring sum than X~^T y."""
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, y = K.linear_problem()
    n = len(y)
    beta = np.array([4., -3., 2., -1., .5] + [0.] * 5)
    start = np.concatenate(([.3 + X.mean(axis=0) @ beta], beta))
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    out = {}
    for family in ('censored', 'linear'):
        kw = {'status': np.zeros(n, dtype=np.uint8)} \
            if family == 'censored' else {}
        chain = HipGibbsChain(hip, family, y, sd_unshrunk=[2.], seed=9, **kw)
        chain.set_coef_sampler('cholesky')
        chain.set_state(start, 25., np.ones(10), .1)
        kept, _ = chain.run(1, save=('coef', 'obs_prec'))
        if family == 'censored':
            assert np.array_equal(chain.get_latent(), y)
        out[family] = (kept['coef'][0], float(kept['obs_prec'][0, 0]),
                       chain.logp()[0])
        chain.close()
    assert out['censored'][1] == out['linear'][1]
    diff = np.abs(out['censored'][0] - out['linear'][0]).max()
    scale = np.abs(out['linear'][0]).max()
    print("no censored row against linear: %.3g of the largest coefficient "
          "(tolerance %.3g)" % (diff / scale, K.RHS_ORDER_TOL))
    assert diff <= K.RHS_ORDER_TOL * scale
    # and the log-likelihood is the linear model's
    assert abs(out['censored'][2] - out['linear'][2]) \
        <= 1e-12 * abs(out['linear'][2])


# ------------------------------------------------- resume, repeatability

def _bridge(family='lognormal', seed=2, n=500, p=30):
    from bayesbridge_amd import (BayesBridge, LogNormalAFTModel,
                                 RegressionCoefPrior, RegressionModel)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[:4] = [1., -1., .5, -.5]
    outcome = LogNormalAFTModel.simulate_outcome(X, beta, 1., .4, seed + 1)
    if family == 'tobit':
        event, censoring = outcome
        outcome = (np.log(np.minimum(event, censoring)),
                   np.isinf(event).astype(np.uint8))
    model = RegressionModel(outcome, X, family)
    assert model.name == family
    prior = RegressionCoefPrior(bridge_exponent=ALPHA,
                                regularizing_slab_size=SLAB)
    return BayesBridge(model, prior)


INIT = {'global_scale': .1, 'coef': np.zeros(31)}
KEYS = ('coef', 'local_scale', 'global_scale', 'obs_prec', 'logp')


@pytest.mark.parametrize("sampler", ('cg', 'cholesky'))
def test_resume_is_exact(sampler):
    whole, _ = _bridge().gibbs(20, seed=5, init=dict(INIT),
                               params_to_save=KEYS, coef_sampler_type=sampler)
    bridge = _bridge()
    first, info = bridge.gibbs(10, seed=5, init=dict(INIT),
                               params_to_save=KEYS, coef_sampler_type=sampler)
    assert isinstance(info['_markov_chain_state']['obs_prec'], float)
    second, _ = bridge.gibbs_resume(info, 10)
    # and from a fresh handle, as after a restart of the process
    third, _ = _bridge().gibbs_resume(info, 10)
    assert whole['obs_prec'].shape == (20,)
    for key in KEYS:
        assert np.array_equal(whole[key][..., :10], first[key]), key
        assert np.array_equal(whole[key][..., 10:], second[key]), key
        assert np.array_equal(whole[key][..., 10:], third[key]), key


def test_same_seed_same_bits_and_another_seed_other_latents():
    runs = []
    for seed in (5, 5, 6):
        bridge = _bridge()
        samples, _ = bridge.gibbs(6, seed=seed, init=dict(INIT),
                                  params_to_save='all')
        assert samples['obs_prec'].shape == (6,)
        assert 'latent' not in samples       # only when asked for
        runs.append((samples, bridge._chain.get_latent()))
    status, y = bridge.model.status, bridge.model.y
    assert .3 < (status == 1).mean() < .5
    for key in KEYS:
        assert np.array_equal(runs[0][0][key], runs[1][0][key]), key
    assert np.array_equal(runs[0][1], runs[1][1])
    cens = status != 0
    assert not np.any(runs[0][1][cens] == runs[2][1][cens])
    assert np.array_equal(runs[0][1][~cens], runs[2][1][~cens])
    assert np.array_equal(runs[0][1][~cens], y[~cens])
    assert not np.array_equal(runs[0][0]['coef'], runs[2][0]['coef'])
    # the latents of every kept sample, when asked for: the run is cut at the
    # kept iterations, which changes no bit of the chain
    bridge = _bridge()
    samples, _ = bridge.gibbs(6, 2, thin=2, seed=5, init=dict(INIT),
                              params_to_save=KEYS + ('latent',))
    assert samples['latent'].shape == (500, 2)
    assert np.all(samples['latent'][cens] > y[cens, None])
    for key in KEYS:
        assert np.array_equal(samples[key], runs[0][0][key][..., [3, 5]]), key
    assert np.array_equal(samples['latent'][:, -1], runs[0][1])
    # the Tobit front on the same rows is the same chain
    tobit, _ = _bridge('tobit').gibbs(6, seed=5, init=dict(INIT),
                                      params_to_save=KEYS)
    for key in KEYS:
        assert np.array_equal(tobit[key], runs[0][0][key]), key


def test_unsupported_requests_name_what_is_unsupported():
    for family in ('lognormal', 'tobit'):
        bridge = _bridge(family)
        for kind in ('hmc', 'nuts'):
            with pytest.raises(ValueError, match="'%s' sampler" % kind):
                bridge.gibbs(2, seed=1, init=dict(INIT),
                             coef_sampler_type=kind,
                             options={'rng': 'reference'})
        with pytest.raises(ValueError, match="rng='reference'"):
            bridge.gibbs(2, seed=1, init=dict(INIT),
                         options={'rng': 'reference'})
        with pytest.raises(ValueError, match='gibbs_batch.*%s' % family):
            bridge.gibbs_batch([1, 2], 2)
        with pytest.raises(ValueError, match='gibbs_multichain.*%s' % family):
            bridge.gibbs_multichain(2, 2)
    # without an initial coefficient vector: the mode search, then the chain;
    # 'woodbury' as well, and an initial obs_prec is taken
    samples, info = bridge.gibbs(3, seed=1, init={'global_scale': .1},
                                 params_to_save=('coef', 'obs_prec'))
    assert info['_init_optim_info']['is_success']
    assert np.all(np.isfinite(samples['coef']))
    assert np.all(samples['obs_prec'] > 0.)
    samples, _ = bridge.gibbs(3, seed=1, init=dict(INIT, obs_prec=2.),
                              params_to_save=('coef', 'obs_prec'),
                              coef_sampler_type='woodbury')
    assert np.all(np.isfinite(samples['coef']))


# -------------------------------------------------------------- prediction

PRED_TOL = {k: O.pred_tolerance(v) for k, v in O.PRED_MEASURED.items()}


def _pred_design(X):
    import scipy.sparse as sparse
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if X.shape[0] == 1:
        # (a single row makes every column constant: the raw CSR path keeps
        # them)
        Xs = sparse.csr_matrix(X)
        return HipSparseDesignMatrix.from_csr_arrays(
            Xs.shape, Xs.indptr, Xs.indices, Xs.data, add_intercept=False,
            storage='csr')
    return HipDenseDesignMatrix(X, add_intercept=False, center_predictor=False)


@pytest.mark.parametrize("n", (1, 257, 4099))
def test_predict_against_the_long_double_oracle(n):
    from bayesbridge_amd import CensoredNormalModel, LogNormalAFTModel
    cases = O.predict_cases()
    for S in (2, 16, 17, 33):
        X, coef, tau, y, status = cases[n, S]
        design = _pred_design(X)
        points = O.survival_points(y)
        times = np.exp(points[1:-1])
        # ---- the Tobit front
        tobit = CensoredNormalModel(y, status, design)
        want = O.predict_explicit(X, coef, tau, y, status)
        rec = O.predict_recurrence(X, coef, tau, y, status)
        got = tobit.predict(coef, tau)
        # ---- the log-normal AFT front on the same latent scale: right-
        # censored where the status is not 0, the density that of t
        event = np.where(status == 0, np.exp(y), np.inf)
        censoring = np.where(status == 0, np.inf, np.exp(y))
        aft = LogNormalAFTModel(event, censoring, design)
        st_aft = (status != 0).astype(np.uint8)
        assert np.array_equal(aft.status, st_aft)
        jac = np.where(st_aft == 0, -aft.y, 0.)
        want_aft = O.predict_explicit(X, coef, tau, aft.y, st_aft, True, jac,
                                      np.log(times))
        rec_aft = O.predict_recurrence(X, coef, tau, aft.y, st_aft, True, jac,
                                       np.log(times))
        got_aft = aft.predict(coef, tau)
        surv = aft.predict_survival(coef, tau, times=times)
        got_aft['surv_mean'], got_aft['surv_sd'] = surv['mean'], surv['sd']
        assert np.array_equal(surv['time'], times)
        for name, w, r, g, keys in (
                ('tobit', want, rec, got, O.PRED_KEYS),
                ('lognormal', want_aft, rec_aft, got_aft,
                 O.PRED_KEYS + O.SURV_KEYS)):
            for key in keys:
                e_rec, e_dev = (O.rel_err(x[key], w[key]) for x in (r, g))
                print("%-9s n %d S %d %-11s oracle f64 vs ext %.2e  device vs "
                      "ext %.2e  tol %.0e" % (name, n, S, key, e_rec, e_dev,
                                              PRED_TOL[key]))
                assert e_rec <= PRED_TOL[key], (name, key)
                assert e_dev <= PRED_TOL[key], (name, key)
            assert g['waic'] == -2. * (g['lppd'] - g['p_waic'])
        # the survival summary at every point of the latent scale, -inf and
        # +inf included (t = 0: everyone survives; never: no one)
        full = tobit._predict_censored(coef, tau, None, None, None,
                                       points=points)
        w = O.predict_explicit(X, coef, tau, y, status, points=points)
        for key in O.SURV_KEYS:
            assert O.rel_err(full[key], w[key]) <= PRED_TOL[key], key
        assert np.all(full['surv_mean'][:, 0] == 1.)
        assert np.all(full['surv_mean'][:, -1] == 0.)
        assert np.all(np.diff(full['surv_mean'], axis=1) <= 0.)
        # the 'lognormal' lppd differs from the 'tobit' lppd on the log times
        # by exactly sum log t over the observed rows: every row's lpd to the
        # measured tolerance (relative to the largest lpd), their sum to n
        # times that
        on_log = CensoredNormalModel(aft.y, st_aft, design).predict(coef, tau)
        tol = PRED_TOL['lpd'] * max(np.abs(on_log['lpd']).max(),
                                    np.abs(got_aft['lpd']).max())
        shift = on_log['lpd'] - got_aft['lpd']
        assert np.abs(shift - np.where(st_aft == 0, aft.y, 0.)).max() \
            <= 2. * tol
        assert abs((on_log['lppd'] - got_aft['lppd'])
                   - aft.y[st_aft == 0].sum()) <= 2. * tol * n
        # the pass size changes no bit
        for per in (1, 16):
            other = aft._predict_censored(coef, tau, None, aft.y, st_aft, jac,
                                          draws_per_pass=per,
                                          points=np.log(times))
            for key in O.PRED_KEYS + O.SURV_KEYS:
                assert np.array_equal(
                    got_aft[key] if key in got_aft else None,
                    other[key]), (key, per)
        # without an outcome: new rows, the mean alone
        plain = tobit.predict(coef, tau, X_new=X)
        assert set(plain) == {'mean', 'sd'}
        assert O.rel_err(plain['mean'], want['mean']) <= PRED_TOL['mean']


# ---------------------------------------------------------------- the C ABI

def test_c_abi_refusals():
    import ctypes
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    from bayesbridge_amd.device_chain import HipGibbsChain
    lib = _lib.load()
    rng = np.random.default_rng(0)
    n = 300
    X = rng.standard_normal((n, 8))
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    y = rng.standard_normal(n)
    status = rng.integers(0, 3, n).astype(np.uint8)
    sd = np.array([2.])

    def create(bound, st, model=_lib.MODEL_CENSORED, design=hip.handle,
               entry=lib.bbx_chain_create_censored, out=True):
        c = c_void_p()
        code = entry(design, model, _ptr(bound), _ptr(st), 1, _ptr(sd), .5,
                     2., 0., 0., 1, byref(c) if out else None)
        if code == 0:
            lib.bbx_chain_destroy(c)
        return code

    assert create(y, status) == 0
    # NULL arguments
    assert create(None, status) == ERR_INVALID
    assert create(y, None) == ERR_INVALID
    assert create(y, status, design=None) == ERR_INVALID
    assert create(y, status, out=False) == ERR_INVALID
    # a bad status code, a non-finite bound: the first offending row is named
    bad = status.copy()
    bad[41], bad[200] = 3, 7
    assert create(y, bad) == ERR_INVALID
    assert 'status[41]' in _lib.last_error()
    for value in (np.nan, np.inf):
        b = y.copy()
        b[17], b[100] = value, value
        assert create(b, status) == ERR_INVALID
        assert 'bound[17]' in _lib.last_error()
    # the two creation entries keep to their models; code 7 stays invalid
    assert create(y, status, model=_lib.MODEL_LINEAR) == ERR_INVALID
    assert create(y, None, entry=lib.bbx_chain_create) == ERR_INVALID
    assert 'bbx_chain_create_censored' in _lib.last_error()
    assert create(y, None, model=7, entry=lib.bbx_chain_create) == ERR_INVALID
    # get_latent: somewhere to put them, and not of a linear chain
    pair = [HipGibbsChain(hip, 'censored', y, status=status, sd_unshrunk=sd,
                          seed=s) for s in (1, 2)]
    linear = HipGibbsChain(hip, 'linear', y, sd_unshrunk=sd, seed=1)
    h = pair[0].handle
    out = np.empty(n)
    assert lib.bbx_chain_get_latent(h, _ptr(out)) == 0
    assert np.array_equal(out, y)
    assert lib.bbx_chain_get_latent(h, None) == ERR_INVALID
    assert lib.bbx_chain_get_latent(linear.handle, _ptr(out)) == ERR_INVALID
    # a batch refuses censored chains, by name
    arr = (c_void_p * 2)(*[c.handle.value for c in pair])
    arr_p = ctypes.cast(arr, c_void_p)
    b = c_void_p()
    for create_batch in (
            lambda: lib.bbx_batch_create(hip.handle, 2, arr_p, byref(b)),
            lambda: lib.bbx_batch_create_opts(hip.handle, 2, arr_p,
                                              _lib.BATCH_ALLOW_SLOW,
                                              byref(b))):
        assert create_batch() == ERR_INVALID
        assert 'censored' in _lib.last_error()
    # obs_prec is the scalar tau in the state
    tau = np.array([2.5])
    assert lib.bbx_chain_set_state(h, None, _ptr(tau), None, None) == 0
    back = np.zeros(1)
    assert lib.bbx_chain_get_state(h, None, _ptr(back), None, None) == 0
    assert back[0] == 2.5
    with pytest.raises(ValueError):
        pair[0].set_state(obs_prec=np.ones(n))
    with pytest.raises(ValueError):
        HipGibbsChain(hip, 'censored', y)            # no status
    with pytest.raises(ValueError):
        HipGibbsChain(hip, 'linear', y, status=status)
    # the three samplers
    for kind in ('cg', 'cholesky', 'woodbury'):
        pair[1].set_coef_sampler(kind)
    # the stand-alone sampler's checks
    fn = lib.bbx_device_censored_normal
    psi = np.zeros(n)

    def draw(n_draw=n, psi=psi, bound=y, st=status, tau=1., out=out, dev=0):
        return fn(dev, 1, n_draw, _ptr(psi), _ptr(bound), _ptr(st), tau,
                  _ptr(out))
    assert draw() == 0 and draw(n_draw=0) == 0
    assert draw(n_draw=-1) == ERR_INVALID
    for name in ('psi', 'bound', 'st', 'out'):
        assert draw(**{name: None}) == ERR_INVALID
    assert draw(st=bad) == ERR_INVALID and 'status[41]' in _lib.last_error()
    nb = y.copy()
    nb[5] = -np.inf
    assert draw(bound=nb) == ERR_INVALID and 'bound[5]' in _lib.last_error()
    for value in (0., -1., float('nan'), float('inf')):
        assert draw(tau=value) == ERR_INVALID and 'tau' in _lib.last_error()
    assert draw(dev=-1) == ERR_INVALID and draw(dev=4096) == ERR_INVALID
    # the predictive summary's checks
    fn = lib.bbx_design_predictive_summary_censored
    coef, taus = np.zeros((2, 9)), np.ones(2)
    res = [np.empty(n) for _ in range(5)]
    pts = np.array([0., 1.])
    surv = [np.empty((2, n)) for _ in range(2)]

    def call(taus=taus, y=y, st=status, n_draw=2, n_point=2, pts=pts):
        return fn(hip.handle, n_draw, 0, _ptr(coef), _ptr(taus), None,
                  _ptr(y), _ptr(st), None, 0, *[_ptr(r) for r in res], None,
                  n_point, _ptr(pts), *[_ptr(s) for s in surv])
    assert call() == 0 and call(n_point=0, pts=None) == 0
    assert call(taus=None) == ERR_INVALID
    assert call(taus=np.array([1., -1.])) == ERR_INVALID
    assert 'obs_prec[1]' in _lib.last_error()
    assert call(y=nb) == ERR_INVALID and 'y[5]' in _lib.last_error()
    assert call(st=bad) == ERR_INVALID and 'status[41]' in _lib.last_error()
    assert call(st=None) == ERR_INVALID
    assert call(n_draw=1) == ERR_INVALID
    assert call(n_draw=-1) == ERR_INVALID
    assert call(n_point=-1) == ERR_INVALID
    assert call(pts=None) == ERR_INVALID
    assert call(pts=np.array([0., np.nan])) == ERR_INVALID
    for c in pair + [linear]:
        c.close()
