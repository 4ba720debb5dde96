"""GPU: the probit model (family='probit') on the Gaussian samplers --
csrc/probit.hip (the truncated-normal latents), the probit branches of
csrc/chain.hip, csrc/probit_predict.hip and the Python layers above them.

  the stand-alone sampler kernel against its host replay, draw by draw;
  four chain iterations on three designs against the oracle: zbase = X~^T z,
    the coefficient draw with Omega = 1, the latents, the log-likelihood, the
    operator counters;
  the three coefficient samplers against the NumPy Albert-Chib chain
    (tests/probit_oracle.py), with a logit chain as the negative control;
  resume, repeatability, prediction against a long-double oracle, the C ABI's
    refusals.
Tolerances: tests/probit_cases.py (measured on the CPU by
tests/test_probit_replay_cpu.py) and tests/replay_cases.py."""
import math
from ctypes import byref, c_void_p

import numpy as np
import pytest

import oracle
from oracle.summarizer import CoefSummarizer, regularized_prior_scale

import probit_cases as P
import probit_oracle as O
import replay_cases as C
from bayesbridge_amd import replay as R

pytestmark = pytest.mark.gpu

ALPHA, SLAB = .5, 2.
ERR_INVALID = -1


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _device_truncated_normal(seed, psi, positive):
    from bayesbridge_amd import _lib
    out = np.empty(psi.size)
    _lib.check(_lib.load().bbx_device_truncated_normal(
        0, seed, psi.size, _ptr(psi), _ptr(positive), _ptr(out)))
    return out


# ------------------------------------------------ the stand-alone kernel

@pytest.mark.parametrize("case", P.TN_CASES,
                         ids=["n%d-%d" % c for c in P.TN_CASES])
def test_device_truncated_normal_equals_the_replay(case):
    seed = P.TN_SEEDS[case]
    psi, positive, bad = P.tn_inputs(case)
    dev = _device_truncated_normal(seed, psi, positive)
    rep, trials = R.truncated_normal(seed, R.STREAM_LATENT, psi, positive, 0,
                                     trace=True)
    assert np.all(np.isnan(dev[bad])) and np.all(np.isnan(rep[bad]))
    P.compare("truncated normal n = %d" % case[0], dev, rep, psi, positive,
              P.TN_TOL, lambda i: "psi %.17g y %d trials %d"
              % (psi[i], positive[i], trials[i]))
    ok = np.isfinite(psi)
    # support, sign and the boundary convention
    assert np.all(dev[ok & (positive != 0)] > 0.)
    assert np.all(dev[ok & (positive == 0)] <= 0.)
    # equal trial counts wherever the draw is not excluded: a draw that took
    # another number of trials is another draw altogether, so an included
    # one (within 1e-12 of the replay's) was accepted at the replay's trial --
    # shown directly by replaying every included draw's trial on its own
    d = P.difference(dev, rep, psi, positive)
    included = np.flatnonzero(ok & (d <= P.TN_TOL))
    assert included.size >= ok.sum() - C.cap(case[0])
    probe = included[np.argsort(trials[included])[-64:]]    # the longest
    for i in probe:
        u = R.uniform(seed, R.STREAM_LATENT, int(i), int(trials[i]) - 1, 2)
        if P.regime(psi[i:i + 1], positive[i:i + 1])[0]:
            lam = .5 * abs(psi[i]) + .5 * math.hypot(psi[i], 2.)
            own = -math.log(u[0]) / lam
        else:
            own = abs(psi[i] + math.sqrt(-2. * math.log(u[0]))
                      * math.cos(2. * math.pi * u[1]))
        assert abs(abs(dev[i]) - own) <= 1e-9 * max(1., abs(psi[i]), own), \
            (i, trials[i])


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
    y = simulate.simulate_outcome(X, beta, 'probit', seed=seed + 1)
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
def test_probit_chain_iteration_equals_oracle(kind, storage):
    """Four consecutive iterations, each compared with the oracle started from
    the device state before it (the pattern of test_hip_chain_pin.py)."""
    from bayesbridge_amd.device_chain import HipGibbsChain
    X, y = _problem(kind)
    hip = _hip_design(X, kind, storage)
    ora = oracle.make_design(X, add_intercept=True, center_predictor=True)
    seed, shape0, rate0 = 17, 1.5, .3
    sd_unshrunk = np.array([2.])
    chain = HipGibbsChain(hip, 'probit', y, sd_unshrunk=sd_unshrunk,
                          bridge_exponent=ALPHA, slab_size=SLAB,
                          gscale_shape=shape0, gscale_rate=rate0, seed=seed)
    n, P_ = hip.shape
    nu = 1
    rng = np.random.default_rng(5)
    chain.set_state(np.zeros(P_), None, np.exp(rng.normal(0., 1., P_ - nu)),
                    .07)
    atol = 10e-6 * np.sqrt(P_)
    f32 = storage == 'float32'
    lp_tol = 1e-7 if f32 else 1e-10
    hip.reset_matvec_count()
    # (counted from here on: the probes of this test go through the same
    # counters, so they are read right around the run below)
    for it in range(4):
        coef_b, obs_b, ls_b, g_b = chain.get_state()
        assert obs_b is None
        mean_b, square_b, n_avg = chain.get_summary()
        assert n_avg == it and chain.iteration == it
        latent_b = chain.get_latent()
        # ---- zbase == X~^T latent, to 1e-12 of the largest entry (with f32
        # storage: of the STORED operator, the centred entries rounded to 24
        # bits; the oracle's differs from it by CHAIN_F32_TOL)
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
        coef_o, info_o = oracle.cg_sample(ora, np.ones(n), phi, z, x0, sd, nu,
                                          eta1, eta2, 500, atol)
        # ---- one device iteration
        before = hip.get_dot_count()
        kept, n_unconv = chain.run(1, save=('coef', 'local_scale'))
        assert n_unconv == 0 and 'obs_prec' not in kept
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
        # ---- the new latents against the replay, from the oracle's psi
        coef_a, _, ls_a, g_a = chain.get_state()
        assert np.array_equal(coef_a, coef_d)
        psi = ora.dot(coef_a)
        latent_a = chain.get_latent()
        rep, trials = R.truncated_normal(
            seed, R.iter_stream(R.STREAM_LATENT, it), psi, y, 0, trace=True)
        P.compare("%s/%s it %d latents" % (kind, storage, it), latent_a, rep,
                  psi, y, C.CHAIN_F32_TOL if f32 else P.CHAIN_LATENT_TOL,
                  lambda i: "psi %.17g y %g trials %d"
                  % (psi[i], y[i], trials[i]))
        assert np.all(latent_a[y == 1.] > 0.) and np.all(latent_a[y == 0.] <= 0.)
        # ---- log-likelihood and log posterior
        ll_d, lp_d = chain.logp()
        ll_o = O.loglik(psi, y)
        assert abs(ll_d - ll_o) <= lp_tol * abs(ll_o), (ll_d, ll_o)
        lp_o = ll_o + _log_prior(coef_a, g_a, nu, sd_unshrunk, shape0, rate0)
        assert lp_d == float(kept['logp'][0])
        assert abs(lp_d - lp_o) <= lp_tol * abs(lp_o), (lp_d, lp_o)
    # ---- a state refresh (set_state with nothing to set) recomputes psi, the
    # latents, zbase and the log-likelihood of the last iteration bit for bit
    latent, zbase, lp = chain.get_latent(), chain.get_zbase(), chain.logp()
    chain.set_state()
    assert np.array_equal(chain.get_latent(), latent)
    assert np.array_equal(chain.get_zbase(), zbase)
    assert chain.logp() == lp
    chain.close()


# --------------------------------- the three samplers, one posterior

# device iterations per sampler, the first N_BURN dropped: 6000 as the plan
# was, but 2000 for 'woodbury', whose draw solves an n x n system (400 x 400
# here) with a host synchronisation per iteration -- 10 s at 6000
N_DEV = {'cg': 6000, 'cholesky': 6000, 'woodbury': 2000}
N_BURN = 500
_cache = {}


def _posterior_problem():
    if 'problem' not in _cache:
        from bayesbridge_amd import simulate
        rng = np.random.default_rng(12)
        X = rng.standard_normal((400, 12))
        beta = np.array([1.2, -1., .8, -.6, .4] + [0.] * 7)
        y = simulate.simulate_outcome(X, beta, 'probit', intercept=.3, seed=13)
        ora = O.ProbitOracle(y, X, ALPHA, 2., SLAB)
        # 4 x 5000 iterations of the NumPy chain, the first 500 of each dropped
        ref = [ora.run(5000, N_BURN, 100 + k) for k in range(4)]
        _cache['problem'] = (X, y, ref)
    return _cache['problem']


def _device_draws(family, sampler, X, y, seed):
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.device_chain import HipGibbsChain
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    chain = HipGibbsChain(hip, family, y, sd_unshrunk=[2.],
                          bridge_exponent=ALPHA, slab_size=SLAB, seed=seed)
    chain.set_coef_sampler(sampler)
    chain.set_state(np.zeros(hip.shape[1]), None, np.ones(hip.shape[1] - 1),
                    .1)
    chain.init_obs_prec()
    kept, n_unconv = chain.run(N_DEV[sampler], n_burnin=N_BURN)
    assert n_unconv == 0
    chain.close()
    return kept['coef']


@pytest.mark.parametrize("sampler", ('cg', 'cholesky', 'woodbury'))
def test_every_sampler_draws_the_oracles_posterior(sampler):
    """N_DEV device iterations (500 dropped) against 4 x 5000 of the oracle:
    |z| < 4.5 on every ergodic mean and variance, batch-means errors."""
    X, y, ref = _posterior_problem()
    draws = _device_draws('probit', sampler, X, y, seed=31)
    z = O.z_scores([draws], ref)
    print("%s: largest z %.2f (coefficient moment %d)"
          % (sampler, z.max(), z.argmax()))
    assert z.shape == (26,) and np.all(np.isfinite(z))
    assert z.max() < 4.5


def test_a_logit_chain_fails_the_same_check():
    """The negative control: the logit posterior's slopes are ~1.7 x larger."""
    X, y, ref = _posterior_problem()
    draws = _device_draws('logit', 'cg', X, y, seed=31)
    z = O.z_scores([draws], ref)
    print("logit control: largest z %.2f" % z.max())
    assert z.max() > 4.5
    ratio = draws.mean(axis=0)[1:6] / np.mean([r.mean(axis=0) for r in ref],
                                              axis=0)[1:6]
    print("logit / probit slopes:", np.round(ratio, 2))


# ------------------------------------------------- resume and repeatability

def _bridge(seed=2, n=500, p=30):
    from bayesbridge_amd import (BayesBridge, RegressionCoefPrior,
                                 RegressionModel, simulate)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[:4] = [1., -1., .5, -.5]
    y = simulate.simulate_outcome(X, beta, 'probit', seed=seed + 1)
    model = RegressionModel(y, X, 'probit')
    assert model.name == 'probit'
    prior = RegressionCoefPrior(bridge_exponent=ALPHA,
                                regularizing_slab_size=SLAB)
    return BayesBridge(model, prior)


INIT = {'global_scale': .1, 'coef': np.zeros(31)}
KEYS = ('coef', 'local_scale', 'global_scale', 'logp')


@pytest.mark.parametrize("sampler", ('cg', 'cholesky'))
def test_resume_is_exact(sampler):
    whole, _ = _bridge().gibbs(20, seed=5, init=dict(INIT),
                               params_to_save=KEYS, coef_sampler_type=sampler)
    bridge = _bridge()
    first, info = bridge.gibbs(10, seed=5, init=dict(INIT),
                               params_to_save=KEYS, coef_sampler_type=sampler)
    assert 'obs_prec' not in info['_markov_chain_state']
    second, _ = bridge.gibbs_resume(info, 10)
    # and from a fresh handle, as after a restart of the process
    third, _ = _bridge().gibbs_resume(info, 10)
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
        assert 'obs_prec' not in samples
        runs.append((samples, bridge._chain.get_latent()))
    for key in KEYS:
        assert np.array_equal(runs[0][0][key], runs[1][0][key]), key
    assert np.array_equal(runs[0][1], runs[1][1])
    assert not np.any(runs[0][1] == runs[2][1])
    assert not np.array_equal(runs[0][0]['coef'], runs[2][0]['coef'])


def test_unsupported_requests_name_what_is_unsupported():
    bridge = _bridge()
    for kind in ('hmc', 'nuts'):
        with pytest.raises(ValueError, match=kind):
            bridge.gibbs(2, seed=1, init=dict(INIT), coef_sampler_type=kind,
                         options={'rng': 'reference'})
    with pytest.raises(ValueError, match="rng='reference'"):
        bridge.gibbs(2, seed=1, init=dict(INIT), options={'rng': 'reference'})
    with pytest.raises(ValueError, match='gibbs_batch'):
        bridge.gibbs_batch([1, 2], 2)
    with pytest.raises(ValueError, match='gibbs_multichain'):
        bridge.gibbs_multichain(2, 2)
    with pytest.raises(ValueError, match='obs_prec'):
        bridge.gibbs(2, seed=1, init=dict(INIT, obs_prec=np.ones(500)))
    # without an initial coefficient vector: the mode search, then the chain
    samples, info = bridge.gibbs(3, seed=1, init={'global_scale': .1})
    assert info['_init_optim_info']['is_success']
    assert np.all(np.isfinite(samples['coef']))


# -------------------------------------------------------------- prediction

PRED_TOL = {k: O.pred_tolerance(v) for k, v in O.PRED_MEASURED.items()}


@pytest.mark.parametrize("n", (1, 257, 4099))
def test_predict_against_the_long_double_oracle(n):
    import scipy.sparse as sparse
    from bayesbridge_amd import (HipDenseDesignMatrix, HipSparseDesignMatrix,
                                 ProbitModel)
    cases = O.predict_cases()
    for S in (2, 16, 17, 33):
        X, coef, y = cases[n, S]
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
        model = ProbitModel(y, design)
        want = O.predict_explicit(X, coef, y)
        rec = O.predict_recurrence(X, coef, y)
        got = model.predict(coef)
        if n >= 257:
            assert got['mean'][0] == 1. and got['mean'][n - 1] == 0.
            assert abs(got['loglik_mean'][n - 2] + 804.6084420137538) < 1e-9
        for key in O.PRED_KEYS:
            e_rec, e_dev = (O.rel_err(r[key], want[key]) for r in (rec, got))
            print("n %d S %d %-11s oracle f64 vs ext %.2e  device vs ext %.2e"
                  "  tol %.0e" % (n, S, key, e_rec, e_dev, PRED_TOL[key]))
            assert e_rec <= PRED_TOL[key], key
            assert e_dev <= PRED_TOL[key], key
        assert got['waic'] == -2. * (got['lppd'] - got['p_waic'])
        # the pass size changes no bit
        for per in (1, 16):
            other = model.predict(coef, _draws_per_pass=per)
            for key in O.PRED_KEYS:
                assert np.array_equal(got[key], other[key]), (key, per)
        # without an outcome: new rows, the mean alone
        plain = model.predict(coef, X_new=X)
        assert set(plain) == {'mean', 'sd'}
        assert O.rel_err(plain['mean'], want['mean']) <= PRED_TOL['mean']


# ---------------------------------------------------------------- the C ABI

def test_c_abi_refusals():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    from bayesbridge_amd.device_chain import HipGibbsChain
    lib = _lib.load()
    rng = np.random.default_rng(0)
    X = rng.standard_normal((300, 8))
    hip = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    n = 300
    y = (rng.random(n) < .5).astype(np.float64)
    sd = np.array([2.])

    def create(outcome, n_trial):
        c = c_void_p()
        st = lib.bbx_chain_create(hip.handle, _lib.MODEL_PROBIT, _ptr(outcome),
                                  _ptr(n_trial), 1, _ptr(sd), .5, 2., 0., 0.,
                                  1, byref(c))
        if st == 0:
            lib.bbx_chain_destroy(c)
        return st

    bad = y.copy()
    bad[17] = 2.
    assert create(bad, None) == ERR_INVALID
    assert 'outcome[17]' in _lib.last_error()
    bad[17] = np.nan
    assert create(bad, None) == ERR_INVALID
    trials = np.ones(n)
    assert create(y, trials) == 0
    trials[41] = 2.
    assert create(y, trials) == ERR_INVALID
    assert 'n_trial[41]' in _lib.last_error()
    # a batch refuses probit chains
    pair = [HipGibbsChain(hip, 'probit', y, sd_unshrunk=sd, seed=s)
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
        assert 'probit' in _lib.last_error()
    # the latents: probit chains only, and somewhere to put them
    out = np.empty(n)
    assert lib.bbx_chain_get_latent(pair[0].handle, _ptr(out)) == 0
    assert lib.bbx_chain_get_latent(pair[0].handle, None) == ERR_INVALID
    assert lib.bbx_chain_get_latent(None, _ptr(out)) == ERR_INVALID
    logit = HipGibbsChain(hip, 'logit', y, sd_unshrunk=sd, seed=1)
    assert lib.bbx_chain_get_latent(logit.handle, _ptr(out)) == ERR_INVALID
    assert 'probit' in _lib.last_error()
    # no obs_prec in a probit chain's state
    assert lib.bbx_chain_get_state(pair[0].handle, None, _ptr(out), None,
                                   None) == ERR_INVALID
    assert lib.bbx_chain_set_state(pair[0].handle, None, _ptr(out), None,
                                   None) == ERR_INVALID
    with pytest.raises(ValueError):
        pair[0].set_state(obs_prec=out)
    # the stand-alone sampler
    psi, pos = np.zeros(4), np.ones(4, dtype=np.uint8)
    z = np.empty(4)
    fn = lib.bbx_device_truncated_normal
    assert fn(0, 1, 4, _ptr(psi), _ptr(pos), _ptr(z)) == 0
    assert fn(0, 1, -1, _ptr(psi), _ptr(pos), _ptr(z)) == ERR_INVALID
    assert fn(0, 1, 4, None, _ptr(pos), _ptr(z)) == ERR_INVALID
    assert fn(0, 1, 4, _ptr(psi), None, _ptr(z)) == ERR_INVALID
    assert fn(0, 1, 4, _ptr(psi), _ptr(pos), None) == ERR_INVALID
    assert fn(99, 1, 4, _ptr(psi), _ptr(pos), _ptr(z)) == ERR_INVALID
    for c in pair + [logit]:
        c.close()
