"""CPU: the host side of the Poisson model -- the NumPy oracle
(tests/poisson_oracle.py) against central differences, the sampler options,
the outcome checks, the declared entry points and the register / scratch use
of the kernels in csrc/poisson.hip."""
import os
import re
import warnings

import numpy as np
import pytest

import poisson_oracle as po
from conftest import ROOT
from test_cholesky_kernel_resources import (HIPCC, _resource_table,
                                            glm_row_occupancy)


class _Design:
    shape = (50, 5)
    use_hip = True
    is_sparse = True
    intercept_added = True


class _Dense(_Design):
    is_sparse = False


def test_oracle_gradient_and_hessian_match_central_differences():
    rs = np.random.RandomState(0)
    n, p = 60, 5
    X = rs.randn(n, p) * .5
    o = np.log(rs.uniform(.5, 2., n))
    y = rs.poisson(np.exp(.3 + o)).astype(np.float64)
    D = po.design(X)
    beta, v = rs.randn(p + 1) * .3, rs.randn(p + 1)
    _, grad = po.loglik_grad(D, y, o, beta)
    h = 1e-5
    num = np.array([
        (po.loglik_grad(D, y, o, beta + h * e)[0]
         - po.loglik_grad(D, y, o, beta - h * e)[0]) / (2 * h)
        for e in np.eye(p + 1)])
    # O(h^2) truncation and eps / h rounding, both ~1e-10 of the values
    np.testing.assert_allclose(grad, num, rtol=1e-7, atol=1e-7)
    hv = po.hessian_matvec(D, y, o, beta, v)
    num = (po.loglik_grad(D, y, o, beta + h * v)[1]
           - po.loglik_grad(D, y, o, beta - h * v)[1]) / (2 * h)
    np.testing.assert_allclose(hv, num, rtol=1e-7, atol=1e-7)
    # f of the preconditioned coordinates: the chain rule and the prior
    scale, pp = np.exp(rs.randn(p + 1) * .3), np.ones(p + 1)
    f = po.precond_f(D, y, o, scale, pp)
    q = rs.randn(p + 1) * .3
    num = np.array([(f(q + h * e)[0] - f(q - h * e)[0]) / (2 * h)
                    for e in np.eye(p + 1)])
    np.testing.assert_allclose(f(q)[1], num, rtol=1e-7, atol=1e-7)


def test_oracle_overflow_and_newton():
    rs = np.random.RandomState(1)
    n, p = 80, 3
    X = rs.randn(n, p) * .5
    o = np.zeros(n)
    truth = np.array([.5, .3, -.2, .1])
    D = po.design(X)
    y = rs.poisson(np.exp(po.dot(D, truth))).astype(np.float64)
    assert po.loglik_grad(D, y, o, truth * 3000.)[0] == -np.inf
    model = po.OracleModel(D, y, o)
    assert model.compute_loglik_and_gradient(truth * 3000.) == (-np.inf, None)
    assert model.calc_intercept_mle() == pytest.approx(np.log(y.mean()))
    beta, cov = po.newton_mle(D, y, o)
    assert np.abs(po.loglik_grad(D, y, o, beta)[1]).max() < 1e-9
    assert np.all(np.abs(beta - truth) < 5 * np.sqrt(np.diag(cov)))
    # a state without a gradient ends the half-tree as unstable
    scale, pp = np.ones(p + 1), np.ones(p + 1)
    f = po.precond_f(D, y, o, scale, pp)
    q0, p0 = truth.copy(), np.full(p + 1, 40.)
    logp0, grad0 = f(q0)
    joint = logp0 - .5 * np.dot(p0, p0)
    model.nuts_begin(scale, pp, q0, p0, logp0, grad0, joint, joint - 1.)
    out = model.nuts_doubling(50., 1, 2, rs.rand(4))
    assert out['instability_detected'] and out['doubling_rejected']
    assert out['n_steps'] == 1 and out['n_uniform'] == 0
    assert out['height'] == 0 and not out['u_turn_detected']
    assert np.array_equal(model.nuts_sample()[0], q0)


@pytest.mark.parametrize('method', [None, 'hmc', 'nuts'])
def test_poisson_takes_the_hamiltonian_samplers_on_the_reference_rng(method):
    from bayesbridge_amd import SamplerOptions
    for design in (_Design(), _Dense()):
        for options in (None, {'rng': 'reference'},
                        {'global_scale_update': None}):
            opt = SamplerOptions.pick_default_and_create(
                method, options, 'poisson', design)
            assert opt.coef_sampler_type == (method or 'hmc')
            assert opt.rng == 'reference'
        if method:
            via_dict = SamplerOptions.pick_default_and_create(
                None, {'coef_sampler_type': method,
                       'global_scale_update': None}, 'poisson', design)
            assert via_dict.get_info() == opt.get_info()
        again = SamplerOptions.pick_default_and_create(
            None, opt.get_info(), 'poisson', design)
        assert again.get_info() == opt.get_info()


@pytest.mark.parametrize('method', ['cg', 'cholesky', 'woodbury'])
def test_poisson_refuses_the_gaussian_samplers_and_the_device_rng(method):
    from bayesbridge_amd import SamplerOptions
    for design in (_Design(), _Dense()):
        with warnings.catch_warnings():
            warnings.simplefilter('error')       # no warn-and-switch either
            with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
                SamplerOptions.pick_default_and_create(method, None,
                                                       'poisson', design)
            with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
                SamplerOptions.pick_default_and_create(
                    None, {'coef_sampler_type': method}, 'poisson', design)
        for ham in (None, 'hmc', 'nuts'):
            with pytest.raises(ValueError, match="rng='reference'"):
                SamplerOptions.pick_default_and_create(
                    ham, {'rng': 'device'}, 'poisson', design)
    with pytest.raises(ValueError):
        SamplerOptions.pick_default_and_create('gibbs', None, 'poisson',
                                               _Design())
    # what the other models are given stays
    opt = SamplerOptions.pick_default_and_create(None, None, 'logit',
                                                 _Design())
    assert opt.coef_sampler_type == 'cg' and opt.rng == 'device'
    with pytest.raises(ValueError):
        SamplerOptions.pick_default_and_create('hmc', None, 'linear',
                                               _Design())


def test_outcome_checks():
    from bayesbridge_amd import PoissonModel, RegressionModel
    from bayesbridge_amd.design_matrix import HipDesignMatrix

    class Design(HipDesignMatrix):       # no device: the checks come first
        shape = (6, 3)

        def __init__(self):
            self._h = None

    d = Design()
    y = np.array([0, 1, 2, 0, 7, 3])
    e = np.array([1., .5, 2., 1., 3., .25])
    m = PoissonModel(y, e, d)
    assert m.name == 'poisson' and m._ham_prefix == 'bbx_poisson_'
    assert m.y.dtype == np.float64 and np.array_equal(m.y, y)
    assert np.array_equal(m.log_exposure, np.log(e))
    assert m.calc_intercept_mle() == pytest.approx(np.log(13 / 7.75))
    assert not m._poisson                 # the handle is made on first use
    m = PoissonModel(y.astype(np.float64), None, d)   # integer-valued floats
    assert np.array_equal(m.exposure, np.ones(6))
    assert m.calc_intercept_mle() == pytest.approx(np.log(13 / 6))
    # the factory takes y or (y, exposure) and a prebuilt design
    assert np.array_equal(RegressionModel(y, d, 'poisson').exposure,
                          np.ones(6))
    assert np.array_equal(RegressionModel((y, e), d, 'poisson').exposure, e)
    for bad_y in (y[:5], np.where(np.arange(6) == 2, -1, y),
                  np.where(np.arange(6) == 2, 1.5, y),
                  np.where(np.arange(6) == 2, np.nan, y),
                  np.where(np.arange(6) == 2, np.inf, y), y.reshape(2, 3)):
        with pytest.raises(ValueError):
            PoissonModel(bad_y, None, d)
    for bad_e in (e[:5], np.where(np.arange(6) == 4, 0., e),
                  np.where(np.arange(6) == 4, -1., e),
                  np.where(np.arange(6) == 4, np.inf, e),
                  np.where(np.arange(6) == 4, np.nan, e)):
        with pytest.raises(ValueError):
            PoissonModel(y, bad_e, d)


def test_simulated_outcome_follows_the_rate():
    from bayesbridge_amd import PoissonModel
    rs = np.random.RandomState(0)
    X = rs.randn(20000, 2) * .3
    beta = np.array([.4, -.2])
    e = rs.uniform(.5, 2., 20000)
    y = PoissonModel.simulate_outcome(X, beta, exposure=e, seed=3)
    assert np.array_equal(
        y, PoissonModel.simulate_outcome(X, beta, exposure=e, seed=3))
    assert y.min() >= 0 and np.issubdtype(y.dtype, np.integer)
    rate = e * np.exp(X.dot(beta))
    # the mean of 20 000 counts: sd = sqrt(sum rate) / n
    assert abs(y.mean() - rate.mean()) < 5 * np.sqrt(rate.sum()) / 20000
    y1 = PoissonModel.simulate_outcome(X, beta, seed=3)
    assert abs(y1.mean() - np.exp(X.dot(beta)).mean()) < 5 * np.sqrt(
        np.exp(X.dot(beta)).sum()) / 20000


def test_poisson_entry_points_are_declared_and_documented():
    from bayesbridge_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_poisson_\w+)\s*\(', header))
    assert declared == {
        'bbx_poisson_create', 'bbx_poisson_destroy', 'bbx_poisson_loglik_grad',
        'bbx_poisson_loglik_grad_dev', 'bbx_poisson_set_location',
        'bbx_poisson_hessian_matvec', 'bbx_poisson_hessian_matvec_dev',
        'bbx_poisson_hmc_trajectory', 'bbx_poisson_nuts_begin',
        'bbx_poisson_nuts_doubling', 'bbx_poisson_nuts_sample'}
    lib = _lib.load()
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert getattr(lib, name).restype is not None
    # the same argument lists as the logit handle's
    sigs = _lib._declare(lib)
    for name in declared - {'bbx_poisson_create'}:
        assert sigs[name] == sigs[name.replace('bbx_poisson_', 'bbx_logit_')]
    hp = sigs['bbx_design_destroy'][0][0]
    assert sigs['bbx_poisson_create'][0][0] is hp
    assert len(sigs['bbx_poisson_create'][0]) == 4
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 109
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in declared:
        assert name in doc, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_poisson_kernels_use_no_scratch(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "poisson.hip"),
        tmp_path)
    # the three modes of the row kernel and the shared trajectory kernels
    assert sum("glm_row_kernel" in k for k in table) == 3
    # no fewer waves per SIMD than poisson_row_kernel<GRAD / LOC / HESS> had
    # before the fold onto glm_rows.hpp (80 / 66 / 50 VGPRs)
    occupancy = glm_row_occupancy(table)
    assert all(got >= was for got, was in zip(occupancy, (6, 7, 8))), occupancy
    for k in ("cox_step1_kernel", "cox_post_a_kernel", "cox_post_b_kernel",
              "cox_finish_kernel", "cox_nuts_leaf_kernel",
              "cox_nuts_merge_a_kernel", "cox_nuts_merge_b_kernel"):
        assert any(k in name for name in table), (k, sorted(table))
    for name, res in table.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= 64 * 1024, (name, res)
