"""CPU: the host side of the logit model's 'hmc' / 'nuts' coefficient samplers
-- the NumPy oracle (tests/logit_oracle.py) against the reference's recorded
values and central differences, the sampler options, the declared entry
points and the register / scratch use of the kernels in csrc/logit.hip."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sparse

import logit_oracle as lo
from conftest import ROOT
from test_cholesky_kernel_resources import (HIPCC, _resource_table,
                                            glm_row_occupancy)


class _Design:
    shape = (50, 5)
    use_hip = True
    is_sparse = True


class _Dense(_Design):
    is_sparse = False


@pytest.mark.parametrize('fmt', ['dense', 'sparse'])
def test_oracle_reproduces_the_reference_likelihood(golden_dir, fmt):
    g = np.load(os.path.join(golden_dir, 'logit_nuts_calls.npz'))
    X = g['chain_%s_X' % fmt]
    if fmt == 'sparse':
        X = sparse.csr_matrix(X)
    y, m = g['chain_%s_n_success' % fmt], g['chain_%s_n_trial' % fmt]
    assert m.max() == 3 and m.min() == 1
    D = lo.design(X)
    big = 0.
    for j in range(3):
        pre = 'lik_%s_%d_' % (fmt, j)
        beta, v = g[pre + 'beta'], g[pre + 'v']
        big = max(big, np.abs(lo.dot(D, beta)).max())
        ll, grad = lo.loglik_grad(D, y, m, beta)
        hv = lo.hessian_matvec(D, y, m, beta, v)
        # the same NumPy expressions on the same float64 data: what is left
        # is the order of the sums inside the design's products
        assert ll == pytest.approx(float(g[pre + 'loglik']), rel=1e-13)
        for got, want in ((grad, g[pre + 'grad']), (hv, g[pre + 'hv'])):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert big > 100.                # saturated probabilities are among them


def test_oracle_gradient_and_hessian_match_central_differences():
    rs = np.random.RandomState(0)
    n, p = 60, 5
    X = rs.randn(n, p)
    m = rs.randint(1, 4, n).astype(np.float64)
    y = rs.binomial(m.astype(int), .4).astype(np.float64)
    D = lo.design(X)
    beta, v = rs.randn(p + 1) * .5, rs.randn(p + 1)
    _, grad = lo.loglik_grad(D, y, m, beta)
    h = 1e-5
    num = np.array([
        (lo.loglik_grad(D, y, m, beta + h * e)[0]
         - lo.loglik_grad(D, y, m, beta - h * e)[0]) / (2 * h)
        for e in np.eye(p + 1)])
    # O(h^2) truncation and eps / h rounding, both ~1e-10 of the values
    np.testing.assert_allclose(grad, num, rtol=1e-7, atol=1e-7)
    hv = lo.hessian_matvec(D, y, m, beta, v)
    num = (lo.loglik_grad(D, y, m, beta + h * v)[1]
           - lo.loglik_grad(D, y, m, beta - h * v)[1]) / (2 * h)
    np.testing.assert_allclose(hv, num, rtol=1e-7, atol=1e-7)
    # f of the preconditioned coordinates: the chain rule and the prior
    scale, pp = np.exp(rs.randn(p + 1) * .3), np.ones(p + 1)
    f = lo.precond_f(D, y, m, scale, pp)
    q = rs.randn(p + 1) * .3
    num = np.array([(f(q + h * e)[0] - f(q - h * e)[0]) / (2 * h)
                    for e in np.eye(p + 1)])
    np.testing.assert_allclose(f(q)[1], num, rtol=1e-7, atol=1e-7)


@pytest.mark.parametrize('method', ['hmc', 'nuts'])
def test_logit_accepts_hamiltonian_samplers_with_the_reference_rng(method):
    from bayesbridge_amd import SamplerOptions
    for design in (_Design(), _Dense()):
        opt = SamplerOptions.pick_default_and_create(
            method, {'rng': 'reference'}, 'logit', design)
        assert opt.coef_sampler_type == method and opt.rng == 'reference'
        via_dict = SamplerOptions.pick_default_and_create(
            None, {'coef_sampler_type': method, 'rng': 'reference'}, 'logit',
            design)
        assert via_dict.get_info() == opt.get_info()
        again = SamplerOptions.pick_default_and_create(
            None, opt.get_info(), 'logit', design)
        assert again.get_info() == opt.get_info()


@pytest.mark.parametrize('method', ['hmc', 'nuts'])
def test_logit_refuses_them_without_the_stated_rng_and_linear_always(method):
    from bayesbridge_amd import SamplerOptions
    with pytest.raises(ValueError, match="rng"):
        SamplerOptions.pick_default_and_create(method, None, 'logit',
                                               _Design())
    with pytest.raises(ValueError, match="'rng': 'reference'"):
        SamplerOptions.pick_default_and_create(
            method, {'global_scale_update': 'sample'}, 'logit', _Design())
    with pytest.raises(ValueError):
        SamplerOptions.pick_default_and_create(method, {'rng': 'device'},
                                               'logit', _Design())
    for options in (None, {'rng': 'reference'}):
        with pytest.raises(ValueError):
            SamplerOptions.pick_default_and_create(method, options, 'linear',
                                                   _Design())
    # the default of a logit chain stays 'cg' on the device RNG
    opt = SamplerOptions.pick_default_and_create(None, None, 'logit',
                                                 _Design())
    assert opt.coef_sampler_type == 'cg' and opt.rng == 'device'


def test_logit_entry_points_are_declared_and_documented():
    from bayesbridge_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_logit_\w+)\s*\(', header))
    assert declared == {
        'bbx_logit_create', 'bbx_logit_destroy', 'bbx_logit_loglik_grad',
        'bbx_logit_loglik_grad_dev', 'bbx_logit_set_location',
        'bbx_logit_hessian_matvec', 'bbx_logit_hessian_matvec_dev',
        'bbx_logit_hmc_trajectory', 'bbx_logit_nuts_begin',
        'bbx_logit_nuts_doubling', 'bbx_logit_nuts_sample'}
    lib = _lib.load()
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert getattr(lib, name).restype is not None
    # the same argument lists as the Cox handle's
    sigs = _lib._declare(lib)
    for name in declared - {'bbx_logit_create'}:
        assert sigs[name] == sigs[name.replace('bbx_logit_', 'bbx_cox_')]
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 108
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in declared:
        assert name in doc, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_logit_kernels_use_no_scratch(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "logit.hip"), tmp_path)
    # the three modes of the row kernel and the shared trajectory kernels
    assert sum("glm_row_kernel" in k for k in table) == 3
    # no fewer waves per SIMD than logit_row_kernel<GRAD / LOC / HESS> had
    # before the fold onto glm_rows.hpp (116 / 72 / 50 VGPRs)
    occupancy = glm_row_occupancy(table)
    assert all(got >= was for got, was in zip(occupancy, (4, 7, 8))), occupancy
    for k in ("cox_step1_kernel", "cox_post_a_kernel", "cox_post_b_kernel",
              "cox_finish_kernel", "cox_nuts_leaf_kernel",
              "cox_nuts_merge_a_kernel", "cox_nuts_merge_b_kernel"):
        assert any(k in name for name in table), (k, sorted(table))
    for name, res in table.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= 64 * 1024, (name, res)
