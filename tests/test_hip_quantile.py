"""GPU: the quantile regression model (family='quantile') on the Gaussian
samplers -- csrc/quantile.hip (tau and the mixing weights), the quantile
branches of csrc/chain.hip, csrc/quantile_predict.hip and the Python layers
above them.

  the mixing weights against the host replay of the inverse-Gaussian draw,
    draw by draw, and the stand-alone sampler against the same replay;
  four chain iterations on three designs against the oracle: tau, zbase =
    X~^T kappa, the coefficient draw with Omega = tau w / kappa2, the weights,
    the log-likelihood;
  the three coefficient samplers against the NumPy chain
    (tests/quantile_oracle.py), with a linear chain as the negative control;
  resume, repeatability, set_quantile, the symmetry of the median, prediction
    against a long-double oracle, the C ABI's refusals.
Tolerances: tests/quantile_cases.py (measured on the CPU by
tests/test_quantile_replay_cpu.py) and tests/replay_cases.py."""
import math
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

import oracle
from oracle.summarizer import CoefSummarizer, regularized_prior_scale

import replay_cases as C
import quantile_cases as K
import quantile_oracle as O
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
    residuals, every q: the state (coef, tau) is set and the iteration counter
    put one past the stream's, so the refresh draws through the kernel an
    iteration uses.  No draw may be excluded: the CPU test shows that none of
    these can change its branch."""
    from bayesbridge_amd import _lib
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, coef, psi, y, where = K.weight_inputs(n)
    hip = _weights_design(X)
    assert hip.shape == (n, len(coef))
    chain = HipGibbsChain(hip, 'quantile', y, sd_unshrunk=[2.], seed=K.SEED)
    assert chain.get_quantile() == .5
    chain.iteration = K.ITERATION + 1
    stream = R.iter_stream(R.STREAM_QMIX, K.ITERATION)
    for q in K.QUANTILES:
        chain.set_quantile(q)
        assert chain.get_quantile() == q
        chain.set_state(coef, K.TAU, np.ones(len(coef) - 1), .1)
        tau = chain.get_state()[1]
        assert tau == K.TAU
        dev = chain.get_latent()
        rep, branch, _ = K.replayed(stream, psi, y, q)
        rel = _relative(dev, rep)
        print("n %d q %g: largest relative difference %.3g (tolerance %.3g)"
              % (n, q, rel.max(), K.WEIGHT_TOL[q]))
        assert np.all(np.isfinite(dev)) and np.all(dev > 0.)
        assert int((~(rel <= K.WEIGHT_TOL[q])).sum()) == K.WEIGHT_CAP
        if n >= 255:
            r = np.array(K.PLANTED + K.PLANTED)
            big = dev[where][np.abs(r) == 1e150]
            assert np.all(big > 0.) and np.all(np.isfinite(big))
            assert 0 < branch.sum() < n       # both roots on these inputs
        # log-likelihood of the state, against long double
        ll = chain.logp()[0]
        want = O.loglik(psi, y, tau, q)
        assert abs(ll - want) <= 1e-10 * abs(want), (ll, want)
        # the stand-alone sampler on the same m, on its own stream
        qq, lam = K.level(q)
        m = qq * np.abs(y - psi)
        out = np.empty(n)
        _lib.check(_lib.load().bbx_device_inverse_gaussian(
            hip.device, K.SEED, n, _ptr(m), lam, _ptr(out)))
        alone = R.inverse_gaussian(K.SEED, R.STREAM_LATENT, m, lam)
        assert int((~(_relative(out, alone) <= C.GAMMA_TOL)).sum()) == 0
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
            HipGibbsChain(hip, 'quantile', bad)
    chain = HipGibbsChain(hip, 'quantile', y, seed=K.SEED, quantile=.9)
    for value in (np.nan, np.inf):
        coef = K.COEF.copy()
        coef[1] = value
        chain.set_state(coef, K.TAU, np.ones(3), .1)
        assert np.all(np.isnan(chain.get_latent()))
        assert math.isnan(chain.logp()[0])
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
    y = simulate.simulate_outcome(X, beta, 'quantile', seed=seed + 1,
                                  quantile=.3)
    return X, np.asarray(y).ravel()


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


# The weights of an iteration, row by row.  Every row is held to the flat
# tolerance (CHAIN_SCALAR_TOL) unless the replay itself says that the row is
# sensitive: its weight moves by more than half of that when psi moves by
# +-CHAIN_PSI_DELTA max(1, |psi|), the product's own rounding.  A weight drawn
# from a normal near 0 is ~ 1 / (q (1 - q) |r|): |d log w| <= 2 dpsi / |r| in
# either branch, so only rows with |r| < 4 dpsi / tolerance = 8e-3 max(1,
# |psi|) can be sensitive at all, and only those whose normal is small are.
# A sensitive row is allowed the flat tolerance plus its replayed change; both
# the number of such rows and their allowance have hard caps:
SENSITIVE_ROWS_CAP = 50       # of 3000: 1.7 %, a third of the rows that the
                              # bound above lets be sensitive (density <= q (1
                              # - q) tau < .21 per unit, |r| < .12)
SENSITIVE_CHANGE_CAP = 100.   # x the flat tolerance: reached only at |r| <
                              # 4e-4 max(1, |psi|) with a normal near 0


def _weight_tolerance(seed, stream, psi, y, q, tau, flat, what):
    """(replayed weights, per-row tolerance, number of sensitive rows, their
    largest replayed change)."""
    base, branch, _ = K.replayed(stream, psi, y, q, tau, seed)
    change = np.zeros(len(psi))
    for s in (-1., 1.):
        moved = psi + s * C.CHAIN_PSI_DELTA * np.maximum(1., np.abs(psi))
        w2, b2, _ = K.replayed(stream, moved, y, q, tau, seed)
        assert np.array_equal(branch, b2), (
            "%s: a HOST fact about this test's inputs, not about the device: "
            "on the state the chain reached, %d replayed draw(s) take "
            "another root when psi moves by its rounding, so device and "
            "replay may differ there; choose another seed for this test"
            % (what, int((branch != b2).sum())))
        change = np.maximum(change, _relative(w2, base))
    sensitive = change > .5 * flat
    tol = np.where(sensitive, flat + change, flat)
    worst = float(change[sensitive].max()) if sensitive.any() else 0.
    return base, tol, int(sensitive.sum()), worst


@pytest.mark.parametrize("kind,storage", [('sparse', 'tiled'),
                                          ('sparse', 'csr'),
                                          ('dense', 'float32')])
def test_chain_iteration_equals_oracle(kind, storage):
    """Four consecutive iterations, each compared with the oracle started from
    the device state before it."""
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, y = _problem(kind)
    hip = _hip_design(X, kind, storage)
    ora = oracle.make_design(X, add_intercept=True, center_predictor=True)
    seed, shape0, rate0, q = 17, 1.5, .3, .3
    qq, theta, kappa2 = O.level(q)
    sd_unshrunk = np.array([2.])
    chain = HipGibbsChain(hip, 'quantile', y, sd_unshrunk=sd_unshrunk,
                          bridge_exponent=ALPHA, slab_size=SLAB,
                          gscale_shape=shape0, gscale_rate=rate0, seed=seed,
                          quantile=q)
    n, P_ = hip.shape
    nu = 1
    rng = np.random.default_rng(5)
    chain.set_state(np.zeros(P_), .4, np.exp(rng.normal(0., 1., P_ - nu)),
                    .07)
    atol = 10e-6 * np.sqrt(P_)
    f32 = storage == 'float32'
    lp_tol = 1e-7 if f32 else 1e-10
    scalar_tol = C.CHAIN_F32_TOL if f32 else C.CHAIN_SCALAR_TOL
    for it in range(4):
        coef_b, tau_b, ls_b, g_b = chain.get_state()
        assert isinstance(tau_b, float)
        mean_b, square_b, n_avg = chain.get_summary()
        assert n_avg == it and chain.iteration == it
        w_b = chain.get_latent()
        assert np.all(w_b > 0.) and np.all(np.isfinite(w_b))
        # ---- zbase == X~^T kappa
        zbase = chain.get_zbase()
        omega = tau_b * w_b / kappa2
        kappa = omega * y - tau_b * theta / kappa2
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
        coef_o, info_o = oracle.cg_sample(ora, omega, phi, z, x0, sd, nu,
                                          eta1, eta2, 500, atol)
        # ---- one device iteration
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
        # ---- tau: the Gamma(3n/2) variate over S, S with the OLD weights and
        # the oracle's psi of the new coefficients
        coef_a, tau_a, ls_a, g_a = chain.get_state()
        assert np.array_equal(coef_a, coef_d)
        assert tau_a == float(kept['obs_prec'][0, 0])
        psi = ora.dot(coef_a)
        S = O.tau_sum(w_b, y - psi, q)
        tau_o = R.gamma(seed, R.iter_stream(R.STREAM_OBSVAR, it),
                        1.5 * n)[0] / S
        assert abs(tau_a - tau_o) <= scalar_tol * tau_o, (it, tau_a, tau_o)
        # ---- the new weights against the replay, with the device's tau
        # (f32 storage: at the psi of the STORED operator, which the zbase
        # check above uses too.  Against the oracle's psi, 2e-7 away, most rows
        # would be sensitive: a weight is no smoother in psi than 1 / |r|.
        # tau, the draw and the log-likelihood stay against the oracle's.)
        w_a = chain.get_latent()
        psi_w = hip.dot(coef_a) if f32 else psi
        if f32:
            assert np.abs(psi_w - psi).max() <= \
                C.CHAIN_F32_TOL * max(1., np.abs(psi).max())
        rep, weight_tol, n_sens, worst = _weight_tolerance(
            seed, R.iter_stream(R.STREAM_QMIX, it), psi_w, y, q, tau_a,
            C.CHAIN_SCALAR_TOL, "%s/%s it %d" % (kind, storage, it))
        rel = _relative(w_a, rep)
        print("%s/%s it %d: n_cg %d, tau %.6g, weights within %.3g; %d "
              "sensitive rows (cap %d), their largest replayed change %.3g "
              "(cap %.3g)" % (kind, storage, it, n_cg, tau_a, rel.max(),
                              n_sens, SENSITIVE_ROWS_CAP, worst,
                              SENSITIVE_CHANGE_CAP * C.CHAIN_SCALAR_TOL))
        assert n_sens <= SENSITIVE_ROWS_CAP
        assert worst <= SENSITIVE_CHANGE_CAP * C.CHAIN_SCALAR_TOL
        assert int((~(rel <= weight_tol)).sum()) == 0
        # ---- log-likelihood and log posterior
        ll_d, lp_d = chain.logp()
        ll_o = O.loglik(psi, y, tau_a, q)
        assert abs(ll_d - ll_o) <= lp_tol * abs(ll_o), (ll_d, ll_o)
        lp_o = ll_o + _log_prior(coef_a, g_a, nu, sd_unshrunk, shape0, rate0)
        assert lp_d == float(kept['logp'][0])
        assert abs(lp_d - lp_o) <= lp_tol * abs(lp_o), (lp_d, lp_o)
    # ---- a state refresh recomputes psi, the weights, zbase and the
    # log-likelihood of the last iteration bit for bit and keeps tau
    latent, zbase, lp = chain.get_latent(), chain.get_zbase(), chain.logp()
    tau = chain.get_state()[1]
    chain.set_state()
    assert np.array_equal(chain.get_latent(), latent)
    assert np.array_equal(chain.get_zbase(), zbase)
    assert chain.logp() == lp and chain.get_state()[1] == tau
    chain.set_quantile(q)
    assert np.array_equal(chain.get_latent(), latent)
    assert chain.logp() == lp
    chain.close()


# --------------------------------- the three samplers, one posterior

N_DEV = {'cg': 6000, 'cholesky': 6000, 'woodbury': 2000}
N_BURN = 500
_cache = {}


def _posterior_problem():
    if 'problem' not in _cache:
        X, y, _ = O.skewed_scale_problem(K.POSTERIOR_DATA_SEED)
        ora = O.QuantileOracle(y, X, K.POSTERIOR_Q, ALPHA, 2., SLAB)
        # 4 x 5000 iterations of the NumPy chain, the first 500 of each dropped
        ref = [ora.run(5000, N_BURN, 100 + k) for k in range(4)]
        _cache['problem'] = (X, y, ref)
    return _cache['problem']


def _device_draws(family, sampler, X, y, seed, n_dev=None, **kw):
    """[n_sample, P + 1]: the coefficients, then tau."""
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    chain = HipGibbsChain(hip, family, y, sd_unshrunk=[2.],
                          bridge_exponent=ALPHA, slab_size=SLAB, seed=seed,
                          **kw)
    chain.set_coef_sampler(sampler)
    chain.set_state(np.zeros(hip.shape[1]), None, np.ones(hip.shape[1] - 1),
                    .1)
    chain.init_obs_prec()
    kept, n_unconv = chain.run(n_dev or N_DEV[sampler], n_burnin=N_BURN,
                               save=('coef', 'obs_prec'))
    assert n_unconv == 0
    chain.close()
    return np.hstack((kept['coef'], kept['obs_prec']))


@pytest.mark.parametrize("sampler", ('cg', 'cholesky', 'woodbury'))
def test_every_sampler_draws_the_oracles_posterior(sampler):
    """N_DEV device iterations (500 dropped) against 4 x 5000 of the oracle:
    |z| < 4.5 on every ergodic mean and variance of the 13 coefficients and of
    tau, batch-means errors."""
    X, y, ref = _posterior_problem()
    draws = _device_draws('quantile', sampler, X, y, seed=31,
                          quantile=K.POSTERIOR_Q)
    z = O.z_scores([draws], ref)
    print("%s: largest z %.2f (moment %d)" % (sampler, z.max(), z.argmax()))
    assert z.shape == (28,) and np.all(np.isfinite(z))
    assert z.max() < 4.5


def test_a_linear_chain_fails_the_same_check():
    """The negative control: the mean's intercept and first slope are not the
    0.8-quantile's."""
    X, y, ref = _posterior_problem()
    draws = _device_draws('linear', 'cg', X, y, seed=31)
    z = O.z_scores([draws], ref)
    print("linear control: largest z %.2f; intercept %.3f against %.3f"
          % (z.max(), draws[:, 0].mean(),
             np.mean([r[:, 0].mean() for r in ref])))
    assert z.max() > 4.5


def test_init_obs_prec_is_the_maximum_likelihood_scale():
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, y, _ = O.skewed_scale_problem(K.POSTERIOR_DATA_SEED)
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    chain = HipGibbsChain(hip, 'quantile', y, sd_unshrunk=[2.], seed=3,
                          quantile=.8)
    coef = np.concatenate(([.2], .1 * np.arange(12)))
    chain.set_state(coef, 5., np.ones(12), .1)
    chain.init_obs_prec()
    Xt = np.hstack([np.ones((400, 1)), X - X.mean(axis=0)])
    want = 1. / np.mean(O.check_loss(y - Xt @ coef, .8))
    tau = chain.get_state()[1]
    assert abs(tau - want) <= C.CHAIN_SCALAR_TOL * want
    ll = chain.logp()[0]
    ll_o = O.loglik(Xt @ coef, y, tau, .8)
    assert abs(ll - ll_o) <= 1e-10 * abs(ll_o)
    chain.close()


def test_the_median_is_symmetric_under_a_sign_flip():
    """q = 0.5 on (y, X) and on (-y, -X): the same posterior with the
    intercept's sign flipped (rho_.5 is even), two 'cholesky' runs at |z| <
    4.5."""
    X, y, _ = O.skewed_scale_problem(K.POSTERIOR_DATA_SEED)
    a = _device_draws('quantile', 'cholesky', X, y, seed=41, n_dev=4500,
                      quantile=.5)
    b = _device_draws('quantile', 'cholesky', -X, -y, seed=42, n_dev=4500,
                      quantile=.5)
    b[:, 0] = -b[:, 0]
    z = O.z_scores([a], [b])
    print("sign flip: largest z %.2f" % z.max())
    assert z.max() < 4.5
    # and q = .8 is NOT q = .8 on the flipped data (that is q = .2)
    c = _device_draws('quantile', 'cholesky', -X, -y, seed=42, n_dev=2500,
                      quantile=.8)
    d = _device_draws('quantile', 'cholesky', X, y, seed=41, n_dev=2500,
                      quantile=.8)
    c[:, 0] = -c[:, 0]
    assert O.z_scores([c], [d]).max() > 4.5


# ------------------------------------------- resume, repeatability, q

def _bridge(seed=2, n=500, p=30, q=.7):
    from bayesbridge_amd import (BayesBridge, RegressionCoefPrior,
                                 RegressionModel, simulate)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[:4] = [1., -1., .5, -.5]
    y = simulate.simulate_outcome(X, beta, 'quantile', seed=seed + 1,
                                  quantile=q)
    model = RegressionModel(y, X, 'quantile', quantile=q)
    assert model.name == 'quantile' and model.quantile == q
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
        assert bridge._chain.get_quantile() == .7
        runs.append((samples, bridge._chain.get_latent()))
    for key in KEYS:
        assert np.array_equal(runs[0][0][key], runs[1][0][key]), key
    assert np.array_equal(runs[0][1], runs[1][1])
    assert not np.any(runs[0][1] == runs[2][1])
    assert not np.array_equal(runs[0][0]['coef'], runs[2][0]['coef'])
    bridge = _bridge()
    samples, _ = bridge.gibbs(6, 2, thin=2, seed=5, init=dict(INIT),
                              params_to_save=KEYS + ('mixing_weight',))
    assert samples['mixing_weight'].shape == (500, 2)
    assert np.all(samples['mixing_weight'] > 0.)
    for key in KEYS:
        assert np.array_equal(samples[key], runs[0][0][key][..., [3, 5]]), key
    assert np.array_equal(samples['mixing_weight'][:, -1], runs[0][1])


def test_set_quantile_refreshes_the_state():
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, coef, psi, y, _ = K.weight_inputs(257)
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    chain = HipGibbsChain(hip, 'quantile', y, sd_unshrunk=[2.], seed=K.SEED,
                          quantile=.9)
    chain.set_state(coef, K.TAU, np.ones(3), .1)
    first = (chain.get_latent(), chain.get_zbase(), chain.logp())
    chain.set_quantile(.05)
    other = (chain.get_latent(), chain.get_zbase(), chain.logp())
    assert not np.array_equal(first[0], other[0])
    assert not np.array_equal(first[1], other[1])
    want = O.loglik(psi, y, K.TAU, .05)
    assert abs(other[2][0] - want) <= 1e-10 * abs(want)
    assert chain.get_state()[1] == K.TAU        # tau is kept
    chain.set_quantile(.9)
    back = (chain.get_latent(), chain.get_zbase(), chain.logp())
    assert np.array_equal(first[0], back[0])
    assert np.array_equal(first[1], back[1]) and first[2] == back[2]
    chain.close()


def test_unsupported_requests_name_what_is_unsupported():
    bridge = _bridge()
    for kind in ('hmc', 'nuts'):
        with pytest.raises(ValueError, match="quantile model.*'%s' sampler"
                           % kind):
            bridge.gibbs(2, seed=1, init=dict(INIT), coef_sampler_type=kind,
                         options={'rng': 'reference'})
    with pytest.raises(ValueError, match="rng='reference'"):
        bridge.gibbs(2, seed=1, init=dict(INIT), options={'rng': 'reference'})
    with pytest.raises(ValueError, match='gibbs_batch.*quantile'):
        bridge.gibbs_batch([1, 2], 2)
    with pytest.raises(ValueError, match='gibbs_multichain.*quantile'):
        bridge.gibbs_multichain(2, 2)
    # without an initial coefficient vector: the mode search, then the chain
    samples, info = bridge.gibbs(3, seed=1, init={'global_scale': .1},
                                 params_to_save=('coef', 'obs_prec'))
    assert np.all(np.isfinite(samples['coef']))
    assert np.all(samples['obs_prec'] > 0.)


# -------------------------------------------------------------- prediction

PRED_TOL = {k: O.pred_tolerance(v) for k, v in O.PRED_MEASURED.items()}


@pytest.mark.parametrize("n", (1, 257, 4099))
def test_predict_against_the_long_double_oracle(n):
    import scipy.sparse as sparse
    from bayesbridge_amd import (HipDenseDesignMatrix, HipSparseDesignMatrix,
                                 QuantileModel)
    cases = O.predict_cases()
    q = O.PRED_Q
    for S in (2, 16, 17, 33):
        X, coef, tau, y = cases[n, S]
        if n == 1:
            Xs = sparse.csr_matrix(X)
            design = HipSparseDesignMatrix.from_csr_arrays(
                Xs.shape, Xs.indptr, Xs.indices, Xs.data, add_intercept=False,
                storage='csr')
        else:
            design = HipDenseDesignMatrix(X, add_intercept=False,
                                          center_predictor=False)
        model = QuantileModel(y, design, q)
        want = O.predict_explicit(X, coef, tau, y, q)
        got = model.predict(coef, tau)
        for key in O.PRED_KEYS:
            e_dev = O.rel_err(got[key], want[key])
            print("n %d S %d %-11s device vs ext %.2e  tol %.0e"
                  % (n, S, key, e_dev, PRED_TOL[key]))
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
    # the full density: the chain's log-likelihood convention, per row
    two = model.predict(coef[:, :2], tau[:2], return_draws=True)
    r = y[:, None] - two['draws']
    dens = np.log(tau[:2]) + math.log(q * (1. - q)) \
        - tau[:2] * O.check_loss(r, q)
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
        st = lib.bbx_chain_create(hip.handle, _lib.MODEL_QUANTILE,
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
    assert create(y, np.ones(n)) == ERR_INVALID
    assert 'n_trial' in _lib.last_error()
    # a batch refuses quantile chains
    pair = [HipGibbsChain(hip, 'quantile', y, sd_unshrunk=sd, seed=s)
            for s in (1, 2)]
    import ctypes
    arr = (c_void_p * 2)(*[c.handle.value for c in pair])
    arr_p = ctypes.cast(arr, c_void_p)
    b = c_void_p()
    assert lib.bbx_batch_create(hip.handle, 2, arr_p, byref(b)) == ERR_INVALID
    assert 'quantile' in _lib.last_error()
    # the level: quantile chains only, inside (0, 1)
    h = pair[0].handle
    q = c_double()
    assert lib.bbx_chain_get_quantile(h, byref(q)) == 0 and q.value == .5
    assert lib.bbx_chain_set_quantile(h, .75) == 0
    assert lib.bbx_chain_get_quantile(h, byref(q)) == 0 and q.value == .75
    for value in (0., 1., -1., 1.5, float('nan'), float('inf')):
        assert lib.bbx_chain_set_quantile(h, value) == ERR_INVALID
        assert 'quantile' in _lib.last_error()
    assert lib.bbx_chain_get_quantile(h, byref(q)) == 0 and q.value == .75
    assert lib.bbx_chain_get_quantile(h, None) == ERR_INVALID
    with pytest.raises(ValueError):
        pair[0].set_quantile(0.)
    linear = HipGibbsChain(hip, 'linear', y, sd_unshrunk=sd, seed=1)
    assert lib.bbx_chain_set_quantile(linear.handle, .5) == ERR_INVALID
    assert 'quantile' in _lib.last_error()
    assert lib.bbx_chain_get_quantile(linear.handle, byref(q)) == ERR_INVALID
    df = c_double()
    assert lib.bbx_chain_get_df(h, byref(df)) == ERR_INVALID
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
    for kind in ('cg', 'cholesky', 'woodbury'):
        pair[1].set_coef_sampler(kind)
    # the stand-alone sampler's checks
    ig = lib.bbx_device_inverse_gaussian
    m = np.abs(y)
    assert ig(hip.device, 1, n, _ptr(m), 2., _ptr(out)) == 0
    assert ig(hip.device, 1, 0, _ptr(m), 2., _ptr(out)) == 0
    assert ig(hip.device, 1, -1, _ptr(m), 2., _ptr(out)) == ERR_INVALID
    assert ig(hip.device, 1, n, None, 2., _ptr(out)) == ERR_INVALID
    assert ig(hip.device, 1, n, _ptr(m), 2., None) == ERR_INVALID
    for lam in (0., -1., float('nan'), float('inf')):
        assert ig(hip.device, 1, n, _ptr(m), lam, _ptr(out)) == ERR_INVALID
        assert 'lambda' in _lib.last_error()
    neg = m.copy()
    neg[7] = -1.
    assert ig(hip.device, 1, n, _ptr(neg), 2., _ptr(out)) == ERR_INVALID
    assert 'm[7]' in _lib.last_error()
    # the predictive summary's checks
    fn = lib.bbx_design_predictive_summary_quantile
    coef, taus = np.zeros((2, 9)), np.ones(2)
    res = [np.empty(n) for _ in range(5)]

    def call(q=.5, taus=taus, y=y, n_draw=2):
        return fn(hip.handle, n_draw, q, _ptr(coef), _ptr(taus), None,
                  _ptr(y), None, 0, *[_ptr(r) for r in res], None)
    assert call() == 0
    for value in (0., 1., float('nan')):
        assert call(q=value) == ERR_INVALID
        assert 'quantile' in _lib.last_error()
    assert call(taus=None) == ERR_INVALID
    assert call(taus=np.array([1., -1.])) == ERR_INVALID
    assert 'obs_prec[1]' in _lib.last_error()
    assert call(y=bad) == ERR_INVALID and 'y[5]' in _lib.last_error()
    assert call(n_draw=1) == ERR_INVALID
    for c in pair + [linear]:
        c.close()
