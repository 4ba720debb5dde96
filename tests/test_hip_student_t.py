"""GPU: the Student-t regression model (family='student_t') on the Gaussian
samplers -- csrc/student_t.hip (tau and the mixing weights), the student_t
branches of csrc/chain.hip, csrc/student_t_predict.hip and the Python layers
above them.

  the mixing weights against the host replay of gamma_draw, draw by draw;
  four chain iterations on three designs against the oracle: tau, zbase =
    X~^T (tau omega y), the coefficient draw with Omega = tau omega, the
    weights, the log-likelihood, the operator counters;
  the three coefficient samplers against the NumPy chain
    (tests/student_t_oracle.py), with a linear chain as the negative control;
  resume, repeatability, df -> inf, prediction against a long-double oracle,
    the C ABI's refusals.
Tolerances: tests/student_t_cases.py (measured on the CPU by
tests/test_student_t_replay_cpu.py) and tests/replay_cases.py."""
import math
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

import oracle
from oracle.summarizer import CoefSummarizer, regularized_prior_scale

import replay_cases as C
import student_t_cases as K
import student_t_oracle as O
from bayesbridge_amd import replay as R

pytestmark = pytest.mark.gpu

ALPHA, SLAB = .5, 2.
ERR_INVALID = -1


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _relative(dev, rep):
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(dev - rep) / np.abs(rep)
    rel[dev == rep] = 0.
    return rel


# ------------------------------------------------ the weights, draw by draw

def _weights_design(X):
    """The n x 3 dense design, centred, with an intercept; one row centred
    would be a row of zeros, so n = 1 is the raw row (the CSR path keeps it)."""
    import scipy.sparse as sparse
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if X.shape[0] > 1:
        return HipDenseDesignMatrix(X, center_predictor=True,
                                    add_intercept=True)
    Xs = sparse.csr_matrix(X)
    return HipSparseDesignMatrix.from_csr_arrays(
        Xs.shape, Xs.indptr, Xs.indices, Xs.data, add_intercept=False,
        storage='csr')


@pytest.mark.parametrize("n", K.SIZES)
def test_weights_equal_the_replay(n):
    """The weights of iteration K.ITERATION's stream at a state with planted
    residuals, every df: a residual can only be planted where psi is known, so
    the state (coef, tau) is set and the iteration counter put one past the
    stream's -- the refresh draws through the kernel an iteration uses, and
    test_chain_iteration_equals_oracle pins the weights an iteration leaves.
    No draw may be excluded (the Gamma variate never looks at the data)."""
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, coef, psi, y, where = K.weight_inputs(n)
    hip = _weights_design(X)
    assert hip.shape == (n, len(coef))
    chain = HipGibbsChain(hip, 'student_t', y, sd_unshrunk=[2.], seed=K.SEED)
    assert chain.get_df() == 4.
    chain.iteration = K.ITERATION + 1
    stream = R.iter_stream(R.STREAM_MIX, K.ITERATION)
    for nu in K.DFS:
        chain.set_df(nu)
        assert chain.get_df() == nu
        chain.set_state(coef, K.TAU, np.ones(len(coef) - 1), .1)
        tau = chain.get_state()[1]
        assert tau == K.TAU
        dev = chain.get_latent()
        rep = O.weights(R.gamma(K.SEED, stream, (nu + 1.) / 2., n), psi, y,
                        tau, nu)
        rel = _relative(dev, rep)
        print("n %d nu %g: largest relative difference %.3g (tolerance %.3g)"
              % (n, nu, rel.max(), K.WEIGHT_TOL[nu]))
        assert np.all(np.isfinite(dev)) and np.all(dev >= 0.)
        assert int((~(rel <= K.WEIGHT_TOL[nu])).sum()) == K.WEIGHT_CAP
        if n >= 255:
            # the planted residuals: omega = g / (nu / 2) at r = 0, and at
            # 1e150 a weight of order 1e-300 that is still a number
            r = np.array(K.PLANTED + K.PLANTED)
            assert np.all(dev[where][np.abs(r) == 1e150] > 0.)
            assert np.all(dev[where][np.abs(r) == 1e150] < 1e-290)
        # log-likelihood of the state, against long double
        ll = chain.logp()[0]
        want = O.loglik(psi, y, tau, nu)
        assert abs(ll - want) <= 1e-10 * abs(want), (ll, want)
    chain.close()


def test_nonfinite_outcomes_are_refused_and_nonfinite_coefficients_give_nan():
    from bayesbridge_amd import BbxError, HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, _, psi, y, _ = K.weight_inputs(257)
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    for row, value in ((41, np.nan), (256, np.inf)):
        bad = y.copy()
        bad[row] = value
        with pytest.raises(BbxError, match=r'outcome\[%d\]' % row):
            HipGibbsChain(hip, 'student_t', bad)
    chain = HipGibbsChain(hip, 'student_t', y, seed=K.SEED)
    for value in (np.nan, np.inf):
        coef = K.COEF.copy()
        coef[1] = value
        chain.set_state(coef, K.TAU, np.ones(3), .1)
        assert np.all(np.isnan(chain.get_latent()))
        assert math.isnan(chain.logp()[0])
    # and a finite state afterwards is a finite state again
    chain.set_state(K.COEF, K.TAU, np.ones(3), .1)
    assert np.all(np.isfinite(chain.get_latent()))
    chain.close()


# ------------------------------------------------------ one chain iteration

def _problem(kind, n=3000, p=200, seed=3):
    from bayesbridge_amd import simulate
    if kind == 'dense':
        X = np.random.default_rng(seed).standard_normal((n, p))
    else:
        X = simulate.simulate_design_csr(n, p, binary_frac=.8,
                                         binary_pred_freq=.1, seed=seed)
    beta = np.zeros(p)
    beta[:5], beta[5:10] = 1.5, -1.
    y = simulate.simulate_outcome(X, beta, 'student_t', seed=seed + 1)
    return X, y


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
    the device state before it (the pattern of test_hip_probit.py)."""
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, y = _problem(kind)
    hip = _hip_design(X, kind, storage)
    ora = oracle.make_design(X, add_intercept=True, center_predictor=True)
    seed, shape0, rate0, df = 17, 1.5, .3, 4.
    sd_unshrunk = np.array([2.])
    chain = HipGibbsChain(hip, 'student_t', y, sd_unshrunk=sd_unshrunk,
                          bridge_exponent=ALPHA, slab_size=SLAB,
                          gscale_shape=shape0, gscale_rate=rate0, seed=seed,
                          df=df)
    n, P_ = hip.shape
    nu = 1
    rng = np.random.default_rng(5)
    chain.set_state(np.zeros(P_), .4, np.exp(rng.normal(0., 1., P_ - nu)),
                    .07)
    atol = 10e-6 * np.sqrt(P_)
    f32 = storage == 'float32'
    lp_tol = 1e-7 if f32 else 1e-10
    scalar_tol = C.CHAIN_F32_TOL if f32 else C.CHAIN_SCALAR_TOL
    weight_tol = C.CHAIN_F32_TOL if f32 else K.WEIGHT_TOL[df]
    hip.reset_matvec_count()
    for it in range(4):
        coef_b, tau_b, ls_b, g_b = chain.get_state()
        assert isinstance(tau_b, float)
        mean_b, square_b, n_avg = chain.get_summary()
        assert n_avg == it and chain.iteration == it
        omega_b = chain.get_latent()
        # ---- zbase == X~^T (tau omega y), to 1e-12 of the largest entry (with
        # f32 storage: of the STORED operator; the oracle's differs from it by
        # CHAIN_F32_TOL)
        zbase = chain.get_zbase()
        kappa = tau_b * omega_b * y
        z = ora.Tdot(kappa)
        own = hip.Tdot(kappa)
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
        coef_o, info_o = oracle.cg_sample(ora, tau_b * omega_b, phi, z, x0,
                                          sd, nu, eta1, eta2, 500, atol)
        # ---- one device iteration
        before = hip.get_dot_count()
        kept, n_unconv = chain.run(1, save=('coef', 'local_scale',
                                            'obs_prec'))
        assert n_unconv == 0 and kept['obs_prec'].shape == (1, 1)
        coef_d = kept['coef'][0]
        n_cg = int(kept['n_cg_iter'][0])
        slack = max(2, math.ceil(.10 * info_o['n_iter']))
        assert abs(n_cg - info_o['n_iter']) <= slack, (n_cg, info_o['n_iter'])
        scale = max(1., np.abs(coef_o).max())
        tol = 1e-6 if n_cg == info_o['n_iter'] else 1e-5
        assert np.abs(coef_d - coef_o).max() <= tol * scale, \
            (it, np.abs(coef_d - coef_o).max())
        # counters: as a logit iteration, plus ONE X~^T w for zbase
        after = hip.get_dot_count()
        warm = 1 if np.any(x0 != 0.) else 0
        assert after[0] - before[0] == n_cg + warm + 1
        assert after[1] - before[1] == n_cg + 2
        # ---- tau: the Gamma variate over S / 2, S with the OLD weights and the
        # oracle's psi of the new coefficients
        coef_a, tau_a, ls_a, g_a = chain.get_state()
        assert np.array_equal(coef_a, coef_d)
        assert tau_a == float(kept['obs_prec'][0, 0])
        psi = ora.dot(coef_a)
        S = np.sum(omega_b * (y - psi) ** 2)
        tau_o = R.gamma(seed, R.iter_stream(R.STREAM_OBSVAR, it), n / 2.)[0] \
            / (S / 2.)
        assert abs(tau_a - tau_o) <= scalar_tol * tau_o, (it, tau_a, tau_o)
        # ---- the new weights against the replay, with the device's tau
        omega_a = chain.get_latent()
        rep = O.weights(R.gamma(seed, R.iter_stream(R.STREAM_MIX, it),
                                (df + 1.) / 2., n), psi, y, tau_a, df)
        rel = _relative(omega_a, rep)
        print("%s/%s it %d: tau %.6g, weights within %.3g"
              % (kind, storage, it, tau_a, rel.max()))
        assert int((~(rel <= weight_tol)).sum()) == 0
        # ---- log-likelihood and log posterior
        ll_d, lp_d = chain.logp()
        ll_o = O.loglik(psi, y, tau_a, df)
        assert abs(ll_d - ll_o) <= lp_tol * abs(ll_o), (ll_d, ll_o)
        lp_o = ll_o + _log_prior(coef_a, g_a, nu, sd_unshrunk, shape0, rate0)
        assert lp_d == float(kept['logp'][0])
        assert abs(lp_d - lp_o) <= lp_tol * abs(lp_o), (lp_d, lp_o)
    # ---- a state refresh (set_state with nothing to set) recomputes psi, the
    # weights, zbase and the log-likelihood of the last iteration bit for bit
    # and keeps tau
    latent, zbase, lp = chain.get_latent(), chain.get_zbase(), chain.logp()
    tau = chain.get_state()[1]
    chain.set_state()
    assert np.array_equal(chain.get_latent(), latent)
    assert np.array_equal(chain.get_zbase(), zbase)
    assert chain.logp() == lp and chain.get_state()[1] == tau
    chain.set_df(df)
    assert np.array_equal(chain.get_latent(), latent)
    assert chain.logp() == lp
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
        X, y, _ = O.contaminated_problem(K.POSTERIOR_DATA_SEED)
        ora = O.StudentTOracle(y, X, 4., ALPHA, 2., SLAB)
        # 4 x 5000 iterations of the NumPy chain, the first 500 of each dropped
        ref = [ora.run(5000, N_BURN, 100 + k) for k in range(4)]
        _cache['problem'] = (X, y, ref)
    return _cache['problem']


def _device_draws(family, sampler, X, y, seed):
    """[n_sample, P + 1]: the coefficients, then tau."""
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    chain = HipGibbsChain(hip, family, y, sd_unshrunk=[2.],
                          bridge_exponent=ALPHA, slab_size=SLAB, seed=seed)
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
    tau, batch-means errors.  On the CPU, with this data seed, a second oracle
    run of 6000 iterations gave a largest z of 2.73 against the same
    reference, and the NumPy LINEAR chain (omega = 1) 665.7 (on tau's mean;
    152 and 199 on the intercept's and the first slope's)."""
    X, y, ref = _posterior_problem()
    draws = _device_draws('student_t', sampler, X, y, seed=31)
    z = O.z_scores([draws], ref)
    print("%s: largest z %.2f (moment %d)" % (sampler, z.max(), z.argmax()))
    assert z.shape == (28,) and np.all(np.isfinite(z))
    assert z.max() < 4.5


def test_a_linear_chain_fails_the_same_check():
    """The negative control: the contaminated tenth of the rows drags the
    Gaussian fit's first slope and intercept, and its tau is the variance of
    everything."""
    X, y, ref = _posterior_problem()
    draws = _device_draws('linear', 'cg', X, y, seed=31)
    z = O.z_scores([draws], ref)
    print("linear control: largest z %.2f; first slope %.3f against %.3f"
          % (z.max(), draws[:, 1].mean(),
             np.mean([r[:, 1].mean() for r in ref])))
    assert z.max() > 4.5


# ------------------------------------------- resume, repeatability, df

def _bridge(seed=2, n=500, p=30, df=4.):
    from bayesbridge_amd import (BayesBridge, RegressionCoefPrior,
                                 RegressionModel, simulate)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[:4] = [1., -1., .5, -.5]
    y = simulate.simulate_outcome(X, beta, 'student_t', seed=seed + 1)
    model = RegressionModel(y, X, 'student_t', df=df)
    assert model.name == 'student_t' and model.df == df
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


def test_same_seed_same_bits_and_another_seed_other_weights():
    runs = []
    for seed in (5, 5, 6):
        bridge = _bridge()
        samples, _ = bridge.gibbs(6, seed=seed, init=dict(INIT),
                                  params_to_save='all')
        assert samples['obs_prec'].shape == (6,)
        assert 'mixing_weight' not in samples       # only when asked for
        runs.append((samples, bridge._chain.get_latent()))
    for key in KEYS:
        assert np.array_equal(runs[0][0][key], runs[1][0][key]), key
    assert np.array_equal(runs[0][1], runs[1][1])
    assert not np.any(runs[0][1] == runs[2][1])
    assert not np.array_equal(runs[0][0]['coef'], runs[2][0]['coef'])
    # the weights of every kept sample, when asked for: the run is cut at the
    # kept iterations, which changes no bit of the chain
    bridge = _bridge()
    samples, _ = bridge.gibbs(6, 2, thin=2, seed=5, init=dict(INIT),
                              params_to_save=KEYS + ('mixing_weight',))
    assert samples['mixing_weight'].shape == (500, 2)
    assert np.all(samples['mixing_weight'] > 0.)
    for key in KEYS:
        assert np.array_equal(samples[key], runs[0][0][key][..., [3, 5]]), key
    assert np.array_equal(samples['mixing_weight'][:, -1], runs[0][1])


def test_unsupported_requests_name_what_is_unsupported():
    bridge = _bridge()
    for kind in ('hmc', 'nuts'):
        with pytest.raises(ValueError, match="'%s' sampler" % kind):
            bridge.gibbs(2, seed=1, init=dict(INIT), coef_sampler_type=kind,
                         options={'rng': 'reference'})
    with pytest.raises(ValueError, match="rng='reference'"):
        bridge.gibbs(2, seed=1, init=dict(INIT), options={'rng': 'reference'})
    with pytest.raises(ValueError, match='gibbs_batch'):
        bridge.gibbs_batch([1, 2], 2)
    with pytest.raises(ValueError, match='gibbs_multichain'):
        bridge.gibbs_multichain(2, 2)
    # without an initial coefficient vector: the mode search, then the chain
    samples, info = bridge.gibbs(3, seed=1, init={'global_scale': .1},
                                 params_to_save=('coef', 'obs_prec'))
    assert info['_init_optim_info']['is_success']
    assert np.all(np.isfinite(samples['coef']))
    assert np.all(samples['obs_prec'] > 0.)


def test_a_huge_df_is_the_linear_model():
    """df = 1e8, one 'cholesky' iteration of a student_t and of a linear chain
    from the same state (the planted coefficients, tau = 25, the same seed):
    the coefficient draws agree to 1e-6 of the largest coefficient.

    The bound is derived from Var(omega) ~ 2/nu.  omega_i = Gamma(a) / (a - 1/2
    + tau r_i^2 / 2), a = (nu+1)/2, is 1 + e_i with sd(e_i) = sqrt(2/nu) =
    1.4e-4 and a mean offset (1 - tau r_i^2) / nu = O(1e-8).  To first order
    the draw moves by (X~^T Omega X~)^-1 X~^T (tau e r), per coordinate a sum
    of n independent terms: sd = sqrt(2/nu) sigma_r / (sqrt(n) sd_x) = 1.4e-4 x
    0.2 / sqrt(16000) = 2.2e-7, i.e. 5.6e-8 of the largest coefficient (4);
    the largest of 11 coordinates stays below 4 sd = 2.3e-7, a quarter of
    1e-6.  (The draw's random part moves by 1.4e-4 / sqrt(n) of a posterior sd
    of 1.6e-3: nothing.)  The same conditional in NumPy over 50 seeds of this
    shape gave at most 2.1e-7.  'cholesky' so that no CG stopping rule stands
    between the two draws."""
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    rng = np.random.default_rng(3)
    n, nu = 16000, 1e8
    X = rng.standard_normal((n, 10))
    beta = np.array([4., -3., 2., -1., .5] + [0.] * 5)
    y = .3 + X @ beta + .2 * rng.standard_normal(n)
    start = np.concatenate(([.3 + X.mean(axis=0) @ beta], beta))
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    draws = {}
    for family in ('student_t', 'linear'):
        kw = {'df': nu} if family == 'student_t' else {}
        chain = HipGibbsChain(hip, family, y, sd_unshrunk=[2.], seed=9, **kw)
        chain.set_coef_sampler('cholesky')
        chain.set_state(start, 25., np.ones(10), .1)
        if family == 'student_t':
            assert np.abs(chain.get_latent() - 1.).max() \
                < 6. * math.sqrt(2. / nu)
        kept, _ = chain.run(1, save=('coef',))
        draws[family] = kept['coef'][0]
        chain.close()
    diff = np.abs(draws['student_t'] - draws['linear']).max()
    print("df = 1e8 against linear: %.3g of the largest coefficient"
          % (diff / np.abs(draws['linear']).max()))
    assert 0. < diff <= 1e-6 * np.abs(draws['linear']).max()


# -------------------------------------------------------------- prediction

PRED_TOL = {k: O.pred_tolerance(v) for k, v in O.PRED_MEASURED.items()}


@pytest.mark.parametrize("n", (1, 257, 4099))
def test_predict_against_the_long_double_oracle(n):
    import scipy.sparse as sparse
    from bayesbridge_amd import (HipDenseDesignMatrix, HipSparseDesignMatrix,
                                 StudentTModel)
    cases = O.predict_cases()
    for S in (2, 16, 17, 33):
        X, coef, tau, y = cases[n, S]
        if n == 1:
            # (a single row makes every column constant: the raw CSR path
            # keeps them)
            Xs = sparse.csr_matrix(X)
            design = HipSparseDesignMatrix.from_csr_arrays(
                Xs.shape, Xs.indptr, Xs.indices, Xs.data, add_intercept=False,
                storage='csr')
        else:
            design = HipDenseDesignMatrix(X, add_intercept=False,
                                          center_predictor=False)
        model = StudentTModel(y, design, 4.)
        want = O.predict_explicit(X, coef, tau, y)
        rec = O.predict_recurrence(X, coef, tau, y)
        got = model.predict(coef, tau)
        for key in O.PRED_KEYS:
            e_rec, e_dev = (O.rel_err(r[key], want[key]) for r in (rec, got))
            print("n %d S %d %-11s oracle f64 vs ext %.2e  device vs ext %.2e"
                  "  tol %.0e" % (n, S, key, e_rec, e_dev, PRED_TOL[key]))
            assert e_rec <= PRED_TOL[key], key
            assert e_dev <= PRED_TOL[key], key
        assert got['waic'] == -2. * (got['lppd'] - got['p_waic'])
        # the pass size changes no bit
        for per in (1, 16):
            other = model.predict(coef, tau, _draws_per_pass=per)
            for key in O.PRED_KEYS:
                assert np.array_equal(got[key], other[key]), (key, per)
        # without an outcome: new rows, the mean alone
        plain = model.predict(coef, tau, X_new=X)
        assert set(plain) == {'mean', 'sd'}
        assert O.rel_err(plain['mean'], want['mean']) <= PRED_TOL['mean']
    # the full t-density: against scipy's at one draw pair
    from scipy.stats import t
    two = model.predict(coef[:, :2], tau[:2], return_draws=True)
    r = y[:, None] - two['draws']
    dens = t.logpdf(r * np.sqrt(tau[:2]), 4.) + .5 * np.log(tau[:2])
    assert np.abs(two['loglik_mean'] - dens.mean(axis=1)).max() \
        <= 1e-12 * np.abs(dens).max()


# ---------------------------------------------------------------- the C ABI

def test_c_abi_refusals():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    from bayesbridge_amd.device_chain import HipGibbsChain
    lib = _lib.load()
    rng = np.random.default_rng(0)
    X = rng.standard_normal((300, 8))
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    n = 300
    y = rng.standard_normal(n)
    sd = np.array([2.])

    def create(outcome, n_trial):
        c = c_void_p()
        st = lib.bbx_chain_create(hip.handle, _lib.MODEL_STUDENT_T,
                                  _ptr(outcome), _ptr(n_trial), 1, _ptr(sd),
                                  .5, 2., 0., 0., 1, byref(c))
        if st == 0:
            lib.bbx_chain_destroy(c)
        return st

    assert create(y, None) == 0
    bad = y.copy()
    bad[17] = np.nan
    assert create(bad, None) == ERR_INVALID
    assert 'outcome[17]' in _lib.last_error()
    bad[17], bad[5] = 0., -np.inf
    assert create(bad, None) == ERR_INVALID
    assert 'outcome[5]' in _lib.last_error()
    # a non-NULL n_trial
    assert create(y, np.ones(n)) == ERR_INVALID
    assert 'n_trial' in _lib.last_error()
    # a batch refuses student_t chains
    pair = [HipGibbsChain(hip, 'student_t', y, sd_unshrunk=sd, seed=s)
            for s in (1, 2)]
    import ctypes
    arr = (c_void_p * 2)(*[c.handle.value for c in pair])
    arr_p = ctypes.cast(arr, c_void_p)
    b = c_void_p()
    for create_batch in (
            lambda: lib.bbx_batch_create(hip.handle, 2, arr_p, byref(b)),
            lambda: lib.bbx_batch_create_opts(hip.handle, 2, arr_p,
                                              _lib.BATCH_ALLOW_SLOW,
                                              byref(b))):
        assert create_batch() == ERR_INVALID
        assert 'student_t' in _lib.last_error()
    # the degrees of freedom: student_t chains only, finite and positive
    h = pair[0].handle
    df = c_double()
    assert lib.bbx_chain_get_df(h, byref(df)) == 0 and df.value == 4.
    assert lib.bbx_chain_set_df(h, 7.5) == 0
    assert lib.bbx_chain_get_df(h, byref(df)) == 0 and df.value == 7.5
    for value in (0., -1., float('nan'), float('inf')):
        assert lib.bbx_chain_set_df(h, value) == ERR_INVALID
        assert 'df' in _lib.last_error()
    assert lib.bbx_chain_get_df(h, byref(df)) == 0 and df.value == 7.5
    assert lib.bbx_chain_get_df(h, None) == ERR_INVALID
    with pytest.raises(ValueError):
        pair[0].set_df(0.)
    linear = HipGibbsChain(hip, 'linear', y, sd_unshrunk=sd, seed=1)
    assert lib.bbx_chain_set_df(linear.handle, 4.) == ERR_INVALID
    assert 'student_t' in _lib.last_error()
    assert lib.bbx_chain_get_df(linear.handle, byref(df)) == ERR_INVALID
    # the weights: somewhere to put them, and not of a linear chain
    out = np.empty(n)
    assert lib.bbx_chain_get_latent(h, _ptr(out)) == 0
    assert lib.bbx_chain_get_latent(h, None) == ERR_INVALID
    assert lib.bbx_chain_get_latent(linear.handle, _ptr(out)) == ERR_INVALID
    # obs_prec is the scalar tau in the state
    tau = np.array([2.5])
    assert lib.bbx_chain_set_state(h, None, _ptr(tau), None, None) == 0
    back = np.zeros(1)
    assert lib.bbx_chain_get_state(h, None, _ptr(back), None, None) == 0
    assert back[0] == 2.5
    with pytest.raises(ValueError):
        pair[0].set_state(obs_prec=np.ones(n))
    # the three samplers
    for kind in ('cg', 'cholesky', 'woodbury'):
        pair[1].set_coef_sampler(kind)
    # the predictive summary's checks
    fn = lib.bbx_design_predictive_summary_student_t
    coef, taus = np.zeros((2, 9)), np.ones(2)
    res = [np.empty(n) for _ in range(5)]

    def call(df=4., taus=taus, y=y, n_draw=2):
        return fn(hip.handle, n_draw, df, _ptr(coef), _ptr(taus), None,
                  _ptr(y), None, 0, *[_ptr(r) for r in res], None)
    assert call() == 0
    for value in (0., float('nan')):
        assert call(df=value) == ERR_INVALID and 'df' in _lib.last_error()
    assert call(taus=None) == ERR_INVALID
    assert call(taus=np.array([1., -1.])) == ERR_INVALID
    assert 'obs_prec[1]' in _lib.last_error()
    assert call(y=bad) == ERR_INVALID and 'y[5]' in _lib.last_error()
    assert call(n_draw=1) == ERR_INVALID
    for c in pair + [linear]:
        c.close()
