"""GPU: the 'woodbury' coefficient sampler on dense designs
(csrc/woodbury.hip): the matrix-core Gram over the columns against NumPy, the
draw with given normals against the tests' CPU statement
(tests/woodbury_oracle.py, itself checked against the explicit P x P inverse
in tests/test_woodbury_oracle.py), the device chain draw by draw, the long-run
comparison with the reference's chain, and the refusals.

Tolerance of a draw: 1e-10 * max(1, |ref|), the figure tests/test_hip_cholesky.py
holds the 'cholesky' draw to.  The oracle's own distance from the explicit
inverse is at most 9e-13 on these cases (tests/test_woodbury_oracle.py prints
it), ten times that is below the 'cholesky' figure, so the larger one holds."""
import os
import warnings

import numpy as np
import pytest

import longrun_cases as lc
from cholesky_oracle import explicit
from woodbury_oracle import (CASES, affine_map, case, explicit_posterior,
                             transposed_fisher_info, woodbury_draw)

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _design(Xt, storage='float64'):
    """The HIP design whose X~ is Xt (column 0 ones, the rest centred)."""
    from bayesbridge_amd import HipDenseDesignMatrix
    return HipDenseDesignMatrix(Xt[:, 1:].copy(), center_predictor=False,
                                add_intercept=True, storage_dtype=storage)


def _close(a, ref, tol=TOL):
    err = np.abs(a - ref).max()
    print("max|dev - oracle| = %.2e (|ref| %.2e)" % (err, np.abs(ref).max()))
    return err <= tol * max(1., np.abs(ref).max())


@pytest.mark.parametrize("storage", ['float64', 'float32'])
@pytest.mark.parametrize("shape", [(70, 333), (130, 1), (257, 2500), (64, 64)])
def test_transposed_fisher_info_matches_numpy(shape, storage, monkeypatch):
    from bayesbridge_amd import HipDenseDesignMatrix
    n, p = shape
    rng = np.random.default_rng(n + p)
    X = rng.normal(size=(n, p)) + rng.normal(size=p)
    w = rng.gamma(2., .3, p + 1)
    w[rng.random(p + 1) < .2] = 0.
    w[0] = 0.
    for centred in (True, False):
        d = HipDenseDesignMatrix(X, center_predictor=centred,
                                 add_intercept=True, storage_dtype=storage)
        Xt = explicit(d)
        for weights in (w, np.where(w == 0, .5, w)):
            ref = transposed_fisher_info(Xt, weights)
            G = d.compute_transposed_fisher_info(weights)
            assert G.shape == (n, n)
            assert np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()
            assert np.array_equal(G, G.T)
            assert np.array_equal(G, d.compute_transposed_fisher_info(weights))
    # the batched-tile path: a slab bound that holds two tiles' partials
    monkeypatch.setenv("BBX_GRAM_SLAB_BYTES", str(2 * 64 * 64 * 8))
    d.release_sampler_memory()
    G2 = d.compute_transposed_fisher_info(weights)
    assert np.abs(G2 - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(G2, d.compute_transposed_fisher_info(weights))
    assert np.array_equal(G2, G2.T)


def test_transposed_fisher_info_sparse_design_raises():
    import scipy.sparse as sp
    from bayesbridge_amd import HipSparseDesignMatrix
    d = HipSparseDesignMatrix(sp.random(50, 20, .3, format='csr',
                                        random_state=1))
    with pytest.raises(NotImplementedError):
        d.compute_transposed_fisher_info(np.ones(21))


@pytest.mark.parametrize("storage", ['float64', 'float32'])
@pytest.mark.parametrize("name", CASES)
def test_woodbury_sample_matches_oracle(name, storage):
    from bayesbridge_amd.reg_coef_sampler import woodbury_sample
    Xt, obs_prec, pps, y = case(name)
    d = _design(Xt, storage)
    Xd = explicit(d)
    if storage == 'float64':
        assert np.abs(Xd - Xt).max() <= 1e-15 * np.abs(Xt).max()
    n, P = Xt.shape
    rng = np.random.default_rng(5)
    for _ in range(2):
        delta, xi = rng.standard_normal(n), rng.standard_normal(P)
        ref = woodbury_draw(Xd, obs_prec, pps, y, delta, xi)
        out = woodbury_sample(d, obs_prec, pps, y, delta, xi)
        assert _close(out, ref)
        assert np.array_equal(
            out, woodbury_sample(d, obs_prec, pps, y, delta, xi))


def test_woodbury_sample_wider_than_the_lds_bound():
    """P = 20 001 > 19 200: the wide X~ v path inside the draw."""
    from bayesbridge_amd import HipDenseDesignMatrix
    from bayesbridge_amd.reg_coef_sampler import woodbury_sample
    rng = np.random.default_rng(11)
    n, p = 120, 20000
    X = rng.normal(size=(n, p)).astype(np.float32)
    d = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                             storage_dtype='float32')
    Xt = np.hstack((np.ones((n, 1)),
                    X.astype(np.float64) - X.astype(np.float64).mean(axis=0)))
    Xt = Xt.astype(np.float32).astype(np.float64)      # the stored values
    pps = 1 / (.02 * np.exp(rng.normal(0., 1.5, p + 1)))
    pps[0] = 0.
    obs_prec = rng.gamma(2., .15, n) + 1e-3
    y = (rng.integers(0, 2, n) - .5) / obs_prec
    delta, xi = rng.standard_normal(n), rng.standard_normal(p + 1)
    ref = woodbury_draw(Xt, obs_prec, pps, y, delta, xi)
    assert _close(woodbury_sample(d, obs_prec, pps, y, delta, xi), ref)


def test_device_draw_is_the_gaussian_posterior():
    """The affine-map check through the device entry: n + P + 1 calls."""
    from bayesbridge_amd.reg_coef_sampler import woodbury_sample
    Xt, obs_prec, pps, y = case('wide_q1_logit')
    d = _design(Xt)
    n, P = Xt.shape
    m, T = affine_map(
        lambda de, x: woodbury_sample(d, obs_prec, pps, y, de, x), n, P)
    mean, cov = explicit_posterior(explicit(d), obs_prec, pps, y)
    assert np.abs(m - mean).max() <= TOL * max(1., np.abs(mean).max())
    assert np.abs(T @ T.T - cov).max() <= TOL * np.abs(cov).max()


def _shrunk(g, ls, slab):
    sc = g * ls
    return sc / np.sqrt(1 + (sc / slab) ** 2)


def _wide_problem(model, seed=3):
    rng = np.random.default_rng(seed)
    n, p = 90, 300
    X = rng.normal(size=(n, p))
    beta = np.zeros(p)
    beta[:4] = (1., -1., .5, -.5)
    if model == 'linear':
        outcome = .5 + X @ beta + rng.normal(size=n)
    else:
        n_trial = rng.integers(1, 4, n).astype(np.float64)
        outcome = (rng.binomial(n_trial.astype(int),
                                1 / (1 + np.exp(-X @ beta))).astype(float),
                   n_trial)
    return X, outcome


@pytest.mark.parametrize("flat_intercept", [True, False])
@pytest.mark.parametrize("model", ['logit', 'linear'])
def test_device_chain_draw_by_draw(model, flat_intercept):
    """The chain's own state and bbx_chain_eta normals fed to the oracle; and
    the negative control: the same comparison fails when the oracle is given
    a perturbed input (the other normal stream, or Omega 1 % off)."""
    from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,
                                 RegressionCoefPrior, RegressionModel)
    X, outcome = _wide_problem(model)
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    kw = {} if flat_intercept else {'sd_for_intercept': 2.}
    bridge = BayesBridge(RegressionModel(outcome, design, model),
                         RegressionCoefPrior(regularizing_slab_size=1.,
                                             bridge_exponent=.25, **kw))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        s, info = bridge.gibbs(3, seed=4, coef_sampler_type='woodbury',
                               init={'global_scale': .1,
                                     'local_scale': np.ones(300)})
    assert info['options'] == dict(info['options'], rng='device',
                                   coef_sampler_type='woodbury')
    assert 'n_cg_iter' not in info['_reg_coef_sampling_info']
    chain = bridge._chain
    Xt = explicit(design)
    sd_unshrunk = bridge.prior_sd_for_unshrunk
    assert np.isinf(sd_unshrunk[0]) == flat_intercept
    summary = chain.get_summary()
    for _ in range(3):
        coef0, obs, ls, gs = chain.get_state()
        it = chain.iteration
        with np.errstate(divide='ignore'):
            pps = 1 / np.concatenate((sd_unshrunk,
                                      _shrunk(gs, ls, bridge.prior.slab_size)))
        if model == 'linear':
            omega, yy = np.full(design.shape[0], obs), outcome
        else:
            omega = obs
            yy = (outcome[0] - outcome[1] / 2) / obs
        eta1, eta2 = chain.eta(it)
        ref = woodbury_draw(Xt, omega, pps, yy, eta1, eta2)
        out, n_unconv = chain.run(1, save=('coef',))
        assert n_unconv == 0 and np.all(out['n_cg_iter'] == 0)
        coef = out['coef'][0]
        assert _close(coef, ref)
        # negative controls
        eta1_next = chain.eta(it + 1)[0]
        assert not _close(coef, woodbury_draw(Xt, omega, pps, yy, eta1_next,
                                              eta2))
        assert not _close(coef, woodbury_draw(Xt, omega * 1.01, pps, yy, eta1,
                                              eta2))
    after = chain.get_summary()
    assert all(np.array_equal(a, b) for a, b in zip(summary, after))


@pytest.mark.parametrize("model", ['logit', 'linear'])
def test_reference_rng_gibbs_and_resume(model):
    """rng='reference': the normals come from the global NumPy stream,
    randn(n) then randn(P); a resumed run continues the stream, and the option
    round-trips through mcmc_info['options']."""
    from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,
                                 RegressionCoefPrior, RegressionModel)
    X, outcome = _wide_problem(model, seed=8)
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)

    def run(split):
        bridge = BayesBridge(RegressionModel(outcome, design, model),
                             RegressionCoefPrior(regularizing_slab_size=1.))
        opts = {'coef_sampler_type': 'woodbury', 'rng': 'reference'}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if not split:
                s, info = bridge.gibbs(6, seed=2, options=opts)
                return s['coef'], info
            s1, info = bridge.gibbs(3, seed=2, options=opts)
            s2, info = bridge.gibbs_resume(info, 3)
            return np.hstack((s1['coef'], s2['coef'])), info
    whole, info = run(False)
    parts, info2 = run(True)
    assert info2['options']['coef_sampler_type'] == 'woodbury'
    assert info2['options']['rng'] == 'reference'
    assert np.all(np.isfinite(whole))
    assert np.array_equal(whole, parts)


def test_woodbury_chain_matches_reference_long_run(golden_dir):
    """tests/test_hip_longrun.py's comparison on its linear_dense case
    (n = 1 500) with the chain drawing by 'woodbury', against the reference's
    4 x 25 000 ('cg': the same posterior): its fixture, helpers, statistic and
    bounds.  KEEP = 10 000 kept iterations, not that file's 30 000: at
    6.5 ms per iteration (24 block steps of the n x n factorisation, launch
    bound) 30 000 take 204 s on an MI355X against 30 s for that file's
    slowest case.  10 000 take about 70 s; fewer were not chosen because the
    batch-means standard errors need some twenty batches of lc.BATCH = 500
    for a 4.5-sigma bound to mean what it says.  The full 30 000 were run
    once with this seed: max |z| 2.80 (means) and 2.94 (variances), rms
    1.09 / 0.94 over 84 statistics."""
    KEEP = 10000
    import test_hip_longrun as lr
    name = 'linear_dense'
    case = lc.make_case(name)
    ref = lr._fixture(golden_dir, name, case)
    bridge = lr._bridge(case)
    parts = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s, info = bridge.gibbs(
            lc.BURNIN + lr.CHUNK, n_burnin=lc.BURNIN, seed=20263,
            init=dict(case['init']), params_to_save='all',
            coef_sampler_type='woodbury')
        while True:
            parts.append(lc.series(case, s))
            if sum(len(p_) for p_ in parts) >= KEEP:
                break
            s, info = bridge.gibbs_resume(info, lr.CHUNK)
    assert info['options']['coef_sampler_type'] == 'woodbury'
    assert info['options']['rng'] == 'device'
    S = np.concatenate(parts)[:KEEP]
    zm, zv, report = lr._compare(name, lc.batch_stats([S]), ref,
                                 lc.series_names(case))
    print(report)
    assert np.all(np.isfinite(zm)) and np.all(np.isfinite(zv)), report
    assert np.abs(zm).max() < lc.Z_MAX, report
    assert np.abs(zv).max() < lc.Z_MAX, report
    assert np.sqrt((zm ** 2).mean()) < 1.5, report
    assert np.sqrt((zv ** 2).mean()) < 1.5, report


# ---- refusals: each an error code or an exception, none a fault -------------
def test_sparse_designs_refuse_woodbury():
    import scipy.sparse as sp
    from bayesbridge_amd import (BayesBridge, HipGibbsChain,
                                 HipSparseDesignMatrix, RegressionCoefPrior,
                                 RegressionModel, _lib)
    X = sp.random(60, 200, .2, format='csr', random_state=2)
    d = HipSparseDesignMatrix(X)
    y = np.random.default_rng(0).normal(size=60)
    lib = _lib.load()
    z, zn = np.zeros(201), np.zeros(60)
    ptr = lambda a: a.ctypes.data_as(_lib.c_void_p)   # noqa: E731
    st = lib.bbx_woodbury_sample(d._h, ptr(zn + 1), ptr(z + 1), ptr(zn),
                                 ptr(zn), ptr(z), ptr(z.copy()))
    assert st == -1 and 'dense design' in _lib.last_error()
    chain = HipGibbsChain(d, 'linear', y, sd_unshrunk=[np.inf], seed=1)
    with pytest.raises(_lib.BbxError, match='dense design'):
        chain.set_coef_sampler('woodbury')
    chain.close()
    bridge = BayesBridge(RegressionModel(y, d, 'linear'),
                         RegressionCoefPrior())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ValueError, match="Only 'cg' sampler"):
            bridge.gibbs(2, coef_sampler_type='woodbury')


def test_null_arrays_and_bad_inputs_are_error_codes():
    from bayesbridge_amd import _lib
    from bayesbridge_amd.reg_coef_sampler import woodbury_sample
    Xt, obs_prec, pps, y = case('wide_q1_logit')
    d = _design(Xt)
    n, P = Xt.shape
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(_lib.c_void_p)   # noqa: E731
    a_n, a_P, out = np.ones(n), np.ones(P), np.empty(P)
    full = [ptr(a_n), ptr(a_P), ptr(a_n), ptr(a_n), ptr(a_P), ptr(out)]
    for k in range(6):
        args = list(full)
        args[k] = None
        assert lib.bbx_woodbury_sample(d._h, *args) == -1
        assert lib.bbx_woodbury_sample_dev(d._h, *args) == -1
        if k > 0:
            assert lib.bbx_woodbury_sample_scalar(d._h, 1., *args[1:]) == -1
    assert lib.bbx_design_transposed_fisher_info(d._h, None, ptr(out)) == -1
    assert lib.bbx_design_transposed_fisher_info(d._h, ptr(a_P), None) == -1
    assert lib.bbx_design_transposed_fisher_info_dev(d._h, None, None) == -1
    # a negative prior_prec_sqrt, too many flat coefficients
    bad = pps.copy()
    bad[5] = -1.
    with pytest.raises(_lib.BbxError, match='negative'):
        woodbury_sample(d, obs_prec, bad, y)
    bad = pps.copy()
    bad[:33] = 0.
    with pytest.raises(_lib.BbxError, match='flat prior'):
        woodbury_sample(d, obs_prec, bad, y)
    # two identical flat columns: not positive definite, reported
    Xt2 = Xt.copy()
    Xt2[:, 2] = Xt2[:, 1]
    d2 = _design(Xt2)
    bad = pps.copy()
    bad[:3] = 0.
    with pytest.raises(np.linalg.LinAlgError, match='positive definite'):
        woodbury_sample(d2, obs_prec, bad, y)
    # a non-positive weight breaks M's factorisation: first bad pivot reported
    no_flat = np.where(pps == 0, 1., pps)
    with pytest.raises(np.linalg.LinAlgError, match='pivot'):
        woodbury_sample(d, np.full(n, np.nan), no_flat, y)
    # the design is still usable
    assert np.all(np.isfinite(woodbury_sample(d, obs_prec, pps, y)))


def test_more_rows_than_the_bound_is_refused():
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    from bayesbridge_amd.reg_coef_sampler import woodbury_sample
    n = 19201
    X = np.random.default_rng(0).normal(size=(n, 3)).astype(np.float32)
    d = HipDenseDesignMatrix(X, storage_dtype='float32')
    with pytest.raises(_lib.BbxError, match='19200'):
        woodbury_sample(d, np.ones(n), np.ones(4), np.zeros(n))
    with pytest.raises(_lib.BbxError, match='19200'):
        d.compute_transposed_fisher_info(np.ones(4))


def test_batches_and_multichain_refuse_woodbury():
    from bayesbridge_amd import (BayesBridge, HipChainBatch,
                                 HipDenseDesignMatrix, HipGibbsChain,
                                 RegressionCoefPrior, RegressionModel)
    X, outcome = _wide_problem('logit')
    design = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True)
    pair = [HipGibbsChain(design, 'logit', outcome[0], n_trial=outcome[1],
                          sd_unshrunk=[2.], slab_size=1., seed=s_)
            for s_ in (1, 2)]
    pair[1].set_coef_sampler('woodbury')
    with pytest.raises(Exception, match='BBX_SAMPLER_CG'):
        HipChainBatch(pair, allow_slow=True)
    for ch in pair:
        ch.close()
    bridge = BayesBridge(RegressionModel(outcome, design, 'logit'),
                         RegressionCoefPrior())
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with pytest.raises(ValueError, match="'cg' only"):
            bridge.gibbs_batch([1, 2], 2,
                               options={'coef_sampler_type': 'woodbury'})
        with pytest.raises(ValueError, match="'cg' only"):
            bridge.gibbs_multichain(
                2, 2, options={'coef_sampler_type': 'woodbury'})
