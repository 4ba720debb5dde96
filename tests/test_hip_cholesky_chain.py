"""GPU: the device-resident chain with the 'cholesky' coefficient draw
(bbx_chain_set_coef_sampler): draw by draw against the tests' CPU restatement
on the chain's own state and normals, and in distribution against the
long-run fixtures of the reference (the same posterior as the 'cg' chain,
tests/test_hip_longrun.py)."""
import os
import warnings

import numpy as np
import pytest

import longrun_cases as lc
from cholesky_oracle import chol_draw

pytestmark = pytest.mark.gpu


def _fixture(golden_dir, name, case):
    g = np.load(os.path.join(golden_dir, 'longrun_%s.npz' % name))
    assert np.allclose(lc.case_checksum(case), g['checksum'], rtol=1e-12), \
        "regenerated problem is not the fixture's"
    assert list(g['names']) == lc.series_names(case)
    return {k: g[k] for k in ('mean', 'mean_se', 'var', 'var_se')}


def _dense_case(name):
    case = lc.make_case(name)
    ref_case = dict(case)
    if not isinstance(case['X'], np.ndarray):
        case = dict(case, X=case['X'].toarray())
    return case, ref_case


def _bridge(case):
    from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,
                                 RegressionCoefPrior, RegressionModel)
    design = HipDenseDesignMatrix(case['X'].copy(), center_predictor=True,
                                  add_intercept=True)
    model = RegressionModel(case['outcome'], design, case['family'])
    return BayesBridge(model, RegressionCoefPrior(**case['prior_kw']))


def _shrunk(g, ls, slab):
    sc = g * ls
    return sc / np.sqrt(1 + (sc / slab) ** 2)


@pytest.mark.parametrize("model", ['logit', 'linear'])
def test_device_chain_draw_by_draw(golden_dir, model):
    g = np.load(os.path.join(golden_dir, 'chain_%s_dense_cholesky.npz' % model))
    from bayesbridge_amd import (BayesBridge, HipDenseDesignMatrix,
                                 RegressionCoefPrior, RegressionModel)
    design = HipDenseDesignMatrix(g['X'], center_predictor=True,
                                  add_intercept=True)
    outcome = g['y'] if model == 'linear' else (g['n_success'], g['n_trial'])
    bridge = BayesBridge(RegressionModel(outcome, design, model),
                         RegressionCoefPrior(sd_for_intercept=2.,
                                             regularizing_slab_size=1.,
                                             bridge_exponent=.25))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        s, info = bridge.gibbs(3, seed=4, coef_sampler_type='cholesky',
                               init={'global_scale': .1,
                                     'local_scale': np.ones(50)})
    assert info['options'] == dict(info['options'], rng='device',
                                   coef_sampler_type='cholesky')
    assert 'n_cg_iter' not in info['_reg_coef_sampling_info']
    chain = bridge._chain
    Xt = design.toarray()
    sd_unshrunk = bridge.prior_sd_for_unshrunk
    summary = chain.get_summary()
    for _ in range(4):
        coef0, obs, ls, gs = chain.get_state()
        it = chain.iteration
        pps = 1 / np.concatenate((sd_unshrunk,
                                  _shrunk(gs, ls, bridge.prior.slab_size)))
        if model == 'linear':
            omega = np.full(design.shape[0], obs)
            z = obs * (Xt.T @ g['y'])
        else:
            omega = obs
            z = Xt.T @ (g['n_success'] - g['n_trial'] / 2)
        ref = chol_draw(Xt, omega, pps, z, chain.eta(it)[1])
        out, n_unconv = chain.run(1, save=('coef',))
        assert n_unconv == 0 and np.all(out['n_cg_iter'] == 0)
        coef = out['coef'][0]
        assert np.abs(coef - ref).max() <= 1e-10 * max(1., np.abs(ref).max())
    after = chain.get_summary()
    assert all(np.array_equal(a, b) for a, b in zip(summary, after))


def _series(case, seed, keep=lc.DEV_KEEP, omega_scale=None):
    bridge = _bridge(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if omega_scale is None:
            parts = []
            s, info = bridge.gibbs(
                lc.BURNIN + 5000, n_burnin=lc.BURNIN, seed=seed,
                init=dict(case['init']), params_to_save='all',
                coef_sampler_type='cholesky')
            while True:
                parts.append(lc.series(case, s))
                if sum(len(p_) for p_ in parts) >= keep:
                    break
                s, info = bridge.gibbs_resume(info, 5000)
            assert info['options']['coef_sampler_type'] == 'cholesky'
            return np.concatenate(parts)[:keep]
        bridge.gibbs(lc.BURNIN, n_burnin=lc.BURNIN, seed=seed,
                     init=dict(case['init']), coef_sampler_type='cholesky')
        chain = bridge._chain
        rows = {k: [] for k in ('coef', 'local_scale', 'obs_prec',
                                'global_scale', 'logp')}
        for _ in range(keep):
            _, obs, _, _ = chain.get_state()
            chain.set_state(obs_prec=np.asarray(obs) * omega_scale)
            out, _ = chain.run(1, save=('coef', 'local_scale', 'obs_prec'))
            for k in rows:
                rows[k].append(out[k][0])
        s = {'coef': np.ascontiguousarray(np.array(rows['coef']).T),
             'local_scale': np.ascontiguousarray(
                 np.array(rows['local_scale']).T),
             'global_scale': np.array(rows['global_scale']),
             'logp': np.array(rows['logp']),
             'obs_prec': np.ascontiguousarray(np.array(rows['obs_prec']).T)
             if case['family'] == 'logit'
             else np.array(rows['obs_prec'])[:, 0]}
        bridge.prior.adjust_scale(s['global_scale'], s['local_scale'],
                                  to='coef_magnitude')
        return lc.series(case, s)


def _z(name, S, ref, case):
    zm, zv = lc.z_scores(lc.batch_stats([S]), ref)
    report = ("%s: max |z| mean %.2f, variance %.2f; rms %.2f / %.2f over %d"
              % (name, np.abs(zm).max(), np.abs(zv).max(),
                 np.sqrt((zm ** 2).mean()), np.sqrt((zv ** 2).mean()),
                 len(zm)))
    print(report)
    return zm, zv, report


@pytest.mark.parametrize("name", ['linear_dense', 'logit_mixed_ntrial'])
def test_cholesky_chain_matches_reference_long_run(golden_dir, name):
    """30 000 kept iterations of the device chain drawing with 'cholesky'
    against the reference's 4 x 25 000 ('cg': the same posterior), with the
    statistic and bounds of tests/test_hip_longrun.py."""
    case, ref_case = _dense_case(name)
    ref = _fixture(golden_dir, name, ref_case)
    S = _series(case, seed=20262)
    zm, zv, report = _z(name, S, ref, case)
    assert np.all(np.isfinite(zm)) and np.all(np.isfinite(zv)), report
    assert np.abs(zm).max() < lc.Z_MAX, report
    assert np.abs(zv).max() < lc.Z_MAX, report
    assert np.sqrt((zm ** 2).mean()) < 1.5, report
    assert np.sqrt((zv ** 2).mean()) < 1.5, report


def test_cholesky_negative_control_omega_scaled_by_5_percent_fails(golden_dir):
    """The same comparison FAILS when every Polya-Gamma draw is 5 % too large
    by the time the 'cholesky' draw reads it."""
    case, ref_case = _dense_case('logit_mixed_ntrial')
    ref = _fixture(golden_dir, 'logit_mixed_ntrial', ref_case)
    S = _series(case, seed=20262, keep=12000, omega_scale=1.05)
    zm, zv, report = _z('logit_mixed_ntrial [Omega x 1.05]', S, ref, case)
    assert np.abs(zm).max() > 2 * lc.Z_MAX, report
    assert (np.abs(zm) > lc.Z_MAX).sum() >= 5, report
    assert np.sqrt((zm ** 2).mean()) > 1.5, report


def test_batch_refuses_cholesky_chains(golden_dir):
    from bayesbridge_amd import HipChainBatch, HipDenseDesignMatrix, \
        HipGibbsChain
    g = np.load(os.path.join(golden_dir, 'chain_logit_dense_cholesky.npz'))
    design = HipDenseDesignMatrix(g['X'], center_predictor=True,
                                  add_intercept=True)
    pair = [HipGibbsChain(design, 'logit', g['n_success'],
                          n_trial=g['n_trial'], sd_unshrunk=[2.],
                          slab_size=1., seed=s_) for s_ in (1, 2)]
    pair[1].set_coef_sampler('cholesky')
    with pytest.raises(Exception, match='BBX_SAMPLER_CG'):
        HipChainBatch(pair, allow_slow=True)
    for ch in pair:
        ch.close()
