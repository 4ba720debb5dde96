"""CPU: which designs may select the 'cholesky' coefficient sampler."""
import numpy as np
import pytest


class _Dense:
    use_hip = True
    is_sparse = False
    shape = (10, 3)


class _Sparse(_Dense):
    is_sparse = True


class _ShapeOnly:
    shape = (10, 3)


def test_cholesky_accepted_for_hip_dense_designs_only():
    from bayesbridge_amd import SamplerOptions
    opt = SamplerOptions.pick_default_and_create('cholesky', None, 'logit',
                                                 _Dense())
    assert opt.coef_sampler_type == 'cholesky'
    assert opt.get_info()['coef_sampler_type'] == 'cholesky'
    opt = SamplerOptions.pick_default_and_create(
        None, {'coef_sampler_type': 'cholesky', 'rng': 'reference'}, 'linear',
        _Dense())
    assert opt.coef_sampler_type == 'cholesky' and opt.rng == 'reference'
    for design in (_Sparse(), _ShapeOnly()):
        with pytest.raises(ValueError,
                           match="Only 'cg' sampler supported with HIP"):
            SamplerOptions.pick_default_and_create('cholesky', None, 'logit',
                                                   design)
    # the default stays 'cg', dense designs included
    assert SamplerOptions.pick_default_and_create(
        None, None, 'logit', _Dense()).coef_sampler_type == 'cg'
    with pytest.raises(ValueError):
        SamplerOptions.pick_default_and_create('hmc', None, 'logit', _Dense())


def test_cholesky_option_round_trips_through_mcmc_info():
    from bayesbridge_amd import SamplerOptions
    opt = SamplerOptions.pick_default_and_create(
        'cholesky', {'rng': 'reference'}, 'logit', _Dense())
    again = SamplerOptions.pick_default_and_create(
        None, opt.get_info(), 'logit', _Dense())
    assert again.get_info() == opt.get_info()


def test_coefficient_sampler_accepts_cholesky_method():
    from bayesbridge_amd.reg_coef_sampler import HipRegressionCoefficientSampler
    HipRegressionCoefficientSampler(4, np.array([2.]), 'cholesky')
    with pytest.raises(ValueError):
        HipRegressionCoefficientSampler(4, np.array([2.]), 'hmc')
