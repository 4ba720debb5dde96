"""The oracle, the HIP-free host samplers of the product, the synthetic
generator and the prior / logit model checks against what the reference
returned for the same inputs (tests/golden/reference_vectors.npz and
reference_prior_logit.json, recorded by make_reference_vectors.py).  No GPU,
no reference needed."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sparse

import oracle


@pytest.fixture(scope="module")
def ref(golden_dir):
    arrays = np.load(os.path.join(golden_dir, "reference_vectors.npz"))
    with open(os.path.join(golden_dir, "reference_prior_logit.json")) as fh:
        meta = json.load(fh)
    return arrays, meta


def test_operator_and_sampler_equal_reference(ref):
    g, _ = ref
    X = sparse.csr_matrix((g["op_data"], g["op_indices"], g["op_indptr"]),
                          shape=tuple(g["op_shape"]))
    od = oracle.OracleSparseDesign(X, center_predictor=True,
                                   add_intercept=True)
    n, P = od.shape
    v, w = g["op_v"], g["op_w"]
    assert (n, P) == (len(w), len(v))
    assert np.array_equal(g["op_dot"], od.dot(v))
    assert np.array_equal(g["op_tdot"], od.Tdot(w))
    omega, phi, z = g["op_omega"], g["op_phi"], g["op_z"]
    x0, sd = g["op_x0"], g["op_sd"]
    # the reference's sampler drew its two Gaussian vectors after seed(7)
    np.random.seed(7)
    e1, e2 = np.random.randn(n), np.random.randn(P)
    c_o, i_o = oracle.cg_sample(od, omega, phi, z, x0, sd, 1, e1, e2, 500,
                                1e-5 * np.sqrt(P))
    assert i_o['n_iter'] == int(g["op_n_iter"])
    assert np.abs(c_o - g["op_coef"]).max() <= 1e-12


def test_host_and_oracle_samplers_equal_reference_streams(ref):
    """Same seeds => same draws and same final PCG64 state as the reference's
    Cython samplers, for the product's libbbx_hostrng and the oracle's C."""
    from bayesbridge_amd.hostrng import ReferenceRandom
    from oracle.rng import OracleRandom
    g, meta = ref
    rng = np.random.default_rng(0)
    n = 5000
    shape = (1 + rng.binomial(20, .3, n)).astype(np.intc)
    tilt = rng.normal(0, 3, n)
    tilt[:10], tilt[10:20], tilt[20:30] = 0., 40., 1e-8
    tl = np.exp(rng.normal(0, 4, n))
    ref_pg = g["rng_pg"]
    for cls in (ReferenceRandom, OracleRandom):
        mine = cls(5)
        out = mine.polya_gamma(shape, tilt)
        assert np.abs(out - ref_pg).max() <= 1e-14 * ref_pg.max()
        bg = mine.pg_bitgen if hasattr(mine, 'pg_bitgen') else mine.pg
        assert bg.state['state'] == meta["pg_state_after"]
    assert meta["ts_exponents"] == [.25, .125, .5, .9]
    assert g["rng_ts"].shape == (4, n)
    for a, ref_ts in zip(meta["ts_exponents"], g["rng_ts"]):
        for cls in (ReferenceRandom, OracleRandom):
            mine = cls(5)
            out = mine.tilted_stable(a, tl)
            assert np.array_equal(out, ref_ts)


def test_csr_generator_replays_simulate_design(ref):
    from bayesbridge_amd import simulate
    g, meta = ref
    assert meta["sim_cases"] == [dict(binary_frac=1., binary_pred_freq=.05),
                                 dict(binary_frac=.5), dict(binary_frac=.9)]
    for i, kw in enumerate(meta["sim_cases"]):
        A = sparse.csr_matrix((g["sim%d_data" % i], g["sim%d_indices" % i],
                               g["sim%d_indptr" % i]), shape=(400, 50))
        B = simulate.simulate_design_csr(400, 50, seed=11, **kw)
        assert (A != B).nnz == 0


def test_prior_and_logit_validation_equal_reference(ref):
    """The product's own RegressionCoefPrior / LogisticModel checks against the
    reference's (prior.py:7-208, logistic_model.py:10-47): same attributes,
    same get_info, same hyper-parameter solution, same accept/reject."""
    import warnings
    from bayesbridge_amd.model import LogisticModel
    from bayesbridge_amd.prior import RegressionCoefPrior
    _, meta = ref
    cases = [
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
    assert [c["kwargs"] for c in meta["priors"]] == cases
    for kw, theirs in zip(cases, meta["priors"]):
        mine = RegressionCoefPrior(**kw)
        a, b = mine.get_info(), dict(theirs["info"])
        assert list(a) == [key for key, _ in theirs["info"]]
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
        for hyp in ('shape', 'rate'):
            x = mine.param['gscale_neg_power'][hyp]
            y = theirs["gscale_neg_power"][hyp]
            assert abs(x - y) <= 1e-10 * max(abs(y), 1e-300), (kw, hyp)
        assert np.array_equal(mine.sd_for_fixed, theirs["sd_for_fixed"])
        assert mine.clone(bridge_exponent=.5).get_info()['bridge_exponent'] == .5
        for to in ('raw', 'coef_magnitude'):
            want = theirs["adjust_scale"][to]
            g1, l1 = mine.adjust_scale(.3, np.arange(1., 5.), to)
            assert g1 == want["gscale"] and np.array_equal(l1, want["lscale"])
            ga = np.array([.3, .4])
            mine.adjust_scale(ga, np.ones(2), to)
            # in place, like the reference
            assert np.array_equal(ga, want["in_place"])
    bad = [dict(bridge_exponent=2.5),
           dict(n_fixed_effect=2, sd_for_fixed_effect=[1.]),
           dict(global_scale_prior_hyper_param={'log10_mean': 0.})]
    assert [c["kwargs"] for c in meta["prior_bad"]] == bad
    for kw, theirs in zip(bad, meta["prior_bad"]):
        assert theirs["raises"] == "ValueError"
        with pytest.raises(ValueError):
            RegressionCoefPrior(**kw)

    class _D():
        shape = (4, 3)
    ok = [(np.array([0, 1, 1, 0]), None),
          (np.array([0, 2, 1, 3]), np.array([1, 2, 3, 3]))]
    bad = [(np.array([0, 2, 1, 0]), None),
           (np.array([0, 1, 1]), None),
           (np.array([0, 1, 1, 0]), np.array([1, 1, 1])),
           (np.array([0, 1, 1, 0]), np.array([1, 0, 1, 1])),
           (np.array([0, 2, 1, 0]), np.array([1, 1, 1, 1]))]

    def same_inputs(case, ns, nt):
        return case["n_success"] == ns.tolist() and \
            case["n_trial"] == (None if nt is None else nt.tolist())
    assert len(meta["logit_ok"]) == len(ok)
    assert len(meta["logit_bad"]) == len(bad)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for (ns, nt), r in zip(ok, meta["logit_ok"]):
            assert same_inputs(r, ns, nt)
            m = LogisticModel(ns, nt, _D())
            assert np.array_equal(m.n_success, r["stored_n_success"])
            assert np.array_equal(m.n_trial, r["stored_n_trial"])
            assert m.n_trial.dtype == np.dtype(r["stored_n_trial_dtype"]) \
                == np.float64
        for (ns, nt), r in zip(bad, meta["logit_bad"]):
            assert same_inputs(r, ns, nt) and r["raises"] == "ValueError"
            with pytest.raises(ValueError):
                LogisticModel(ns, nt, _D())
