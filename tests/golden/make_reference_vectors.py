"""Generates the fixtures of tests/test_oracle_vs_reference.py by importing the
upstream reference (build container only; see ref_import.py).  The fixtures
are DATA: the inputs of each comparison and what the reference returned for
them, so that the tests run without the reference.  Re-run with

    python tests/golden/make_reference_vectors.py

Files written:
  reference_vectors.npz
      op_*    a simulate_design(300, 40, binary_frac=.5, format_='sparse')
              CSR matrix (np.random.seed(3)), the vectors drawn after it,
              SparseDesignMatrix.dot / .Tdot of them and one prior-
              preconditioned ConjugateGradientSampler draw (np.random.seed(7)
              before the draw)
      rng_*   the reference's Polya-Gamma draws (BasicRandom seed 5) for the
              shapes / tilts of np.random.default_rng(0) and its tilted-stable
              draws for four exponents, each after set_seed(5)
      sim<i>_* three simulate_design(400, 50, seed=11, format_='sparse')
              matrices (kwargs in reference_prior_logit.json "sim_cases")
  reference_prior_logit.json
      RegressionCoefPrior: get_info(), the global-scale hyper-parameters,
      sd_for_fixed and adjust_scale() of four priors, and which arguments it
      rejects; LogisticModel: the outcome it stores for accepted inputs and
      which inputs it rejects; the PCG64 state after the Polya-Gamma draws.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

warnings.simplefilter('ignore')
bb, refsim = ref_import.import_reference()
from bayesbridge.design_matrix import SparseDesignMatrix  # noqa: E402
from bayesbridge.model.logistic_model import LogisticModel  # noqa: E402
from bayesbridge.prior import RegressionCoefPrior  # noqa: E402
from bayesbridge.random import BasicRandom  # noqa: E402
from bayesbridge.reg_coef_sampler.cg_sampler import \
    ConjugateGradientSampler  # noqa: E402

# the cases of tests/test_oracle_vs_reference.py
PRIOR_CASES = [
    dict(),
    dict(bridge_exponent=.25, regularizing_slab_size=1.,
         global_scale_prior_hyper_param={'log10_mean': -4., 'log10_sd': 1.}),
    dict(bridge_exponent=1., n_fixed_effect=3,
         sd_for_fixed_effect=[1., 2., 3.], sd_for_intercept=2.,
         global_scale_prior_hyper_param={'log10_mean': -2., 'log10_sd': .5},
         _global_scale_parametrization='raw'),
    dict(bridge_exponent=1 / 16, n_fixed_effect=2, sd_for_fixed_effect=4.,
         global_scale_prior_hyper_param={'log10_mean': -4.,
                                         'log10_sd': .01}),
]
PRIOR_BAD = [dict(bridge_exponent=2.5),
             dict(n_fixed_effect=2, sd_for_fixed_effect=[1.]),
             dict(global_scale_prior_hyper_param={'log10_mean': 0.})]
LOGIT_OK = [([0, 1, 1, 0], None), ([0, 2, 1, 3], [1, 2, 3, 3])]
LOGIT_BAD = [([0, 2, 1, 0], None),
             ([0, 1, 1], None),
             ([0, 1, 1, 0], [1, 1, 1]),
             ([0, 1, 1, 0], [1, 0, 1, 1]),
             ([0, 2, 1, 0], [1, 1, 1, 1])]
SIM_CASES = [dict(binary_frac=1., binary_pred_freq=.05),
             dict(binary_frac=.5), dict(binary_frac=.9)]
TS_EXPONENTS = [.25, .125, .5, .9]


def jsonable(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def raised(fn):
    try:
        fn()
    except Exception as exc:      # noqa: BLE001 (the class is recorded)
        return type(exc).__name__
    return None


arrays, meta = {}, {}

# operator and CG draw
np.random.seed(3)
X = refsim.simulate_design(300, 40, binary_frac=.5, format_='sparse')
rd = SparseDesignMatrix(X, center_predictor=True, add_intercept=True)
n, P = rd.shape
v, w = np.random.randn(P), np.random.randn(n)
omega = np.random.gamma(2, 1, n)
phi = np.concatenate(([0.], 1 / np.random.gamma(1, .3, P - 1)))
z, x0 = np.random.randn(P), .1 * np.random.randn(P)
sd = 1.3 * np.ones(P)
np.random.seed(7)
coef, info = ConjugateGradientSampler(1).sample(
    rd, omega, phi, z, coef_cg_init=x0, precond_by='prior',
    coef_scaled_sd=sd, maxiter=500, atol=1e-5 * np.sqrt(P))
arrays.update(
    op_data=X.data, op_indices=X.indices, op_indptr=X.indptr,
    op_shape=np.array(X.shape), op_v=v, op_w=w, op_dot=rd.dot(v),
    op_tdot=rd.Tdot(w), op_omega=omega, op_phi=phi, op_z=z, op_x0=x0,
    op_sd=sd, op_coef=coef, op_n_iter=np.array(info['n_iter']))

# samplers
rng = np.random.default_rng(0)
n_draw = 5000
shape = (1 + rng.binomial(20, .3, n_draw)).astype(np.intc)
tilt = rng.normal(0, 3, n_draw)
tilt[:10], tilt[10:20], tilt[20:30] = 0., 40., 1e-8
tl = np.exp(rng.normal(0, 4, n_draw))
rg = BasicRandom()
rg.set_seed(5)
arrays['rng_pg'] = rg.pg.rand_polyagamma(shape, tilt)
meta['pg_state_after'] = rg.pg.get_state()['state']
ts = []
for a in TS_EXPONENTS:
    rg.set_seed(5)
    ts.append(rg.ts.sample(a, tl))
arrays['rng_ts'] = np.array(ts)
meta['ts_exponents'] = TS_EXPONENTS

# synthetic designs
for i, kw in enumerate(SIM_CASES):
    A = refsim.simulate_design(400, 50, seed=11, format_='sparse', **kw)
    A.sort_indices()
    arrays.update({'sim%d_data' % i: A.data, 'sim%d_indices' % i: A.indices,
                   'sim%d_indptr' % i: A.indptr})
meta['sim_cases'] = SIM_CASES

# prior and logit model validation
priors = []
for kw in PRIOR_CASES:
    pr = RegressionCoefPrior(**kw)
    entry = dict(
        kwargs=kw,
        info=[[k, jsonable(val)] for k, val in pr.get_info().items()],
        gscale_neg_power={h: pr.param['gscale_neg_power'][h]
                          for h in ('shape', 'rate')},
        sd_for_fixed=jsonable(np.asarray(pr.sd_for_fixed, dtype=float)),
        adjust_scale={})
    for to in ('raw', 'coef_magnitude'):
        g, ls = pr.adjust_scale(.3, np.arange(1., 5.), to)
        gv = np.array([.3, .4])
        pr.adjust_scale(gv, np.ones(2), to)
        entry['adjust_scale'][to] = dict(gscale=float(g), lscale=jsonable(ls),
                                         in_place=jsonable(gv))
    priors.append(entry)
meta['priors'] = priors
meta['prior_bad'] = [dict(kwargs=kw, raises=raised(
    lambda kw=kw: RegressionCoefPrior(**kw))) for kw in PRIOR_BAD]


class _D():
    shape = (4, 3)


def _arr(x):
    return None if x is None else np.array(x)


logit_ok = []
for ns, nt in LOGIT_OK:
    m = LogisticModel(_arr(ns), _arr(nt), _D())
    logit_ok.append(dict(n_success=ns, n_trial=nt,
                         stored_n_success=jsonable(m.n_success),
                         stored_n_trial=jsonable(m.n_trial),
                         stored_n_trial_dtype=str(m.n_trial.dtype)))
meta['logit_ok'] = logit_ok
meta['logit_bad'] = [dict(n_success=ns, n_trial=nt, raises=raised(
    lambda ns=ns, nt=nt: LogisticModel(_arr(ns), _arr(nt), _D())))
    for ns, nt in LOGIT_BAD]

np.savez_compressed(os.path.join(HERE, 'reference_vectors.npz'), **arrays)
with open(os.path.join(HERE, 'reference_prior_logit.json'), 'w') as fh:
    json.dump(meta, fh, indent=1)
    fh.write('\n')
print('wrote reference_vectors.npz, reference_prior_logit.json')
