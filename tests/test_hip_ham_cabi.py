"""GPU: the statuses and the exact messages of the ten entry points that the
Hamiltonian likelihood handles share (bbx_cox_*, bbx_logit_*, bbx_poisson_*,
bbx_cpoisson_*; plain and stratified Cox are two kinds of bbx_cox), on the
smallest handle of each kind (tests/ham_cabi.py).  Every refusal is made on
the host before any launch.  Then one valid round: the host and the device
entry point of the likelihood agree bit for bit."""
from ctypes import byref, c_double, c_void_p

import numpy as np
import pytest

import ham_cabi as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(params=sorted(hc.KINDS))
def handle(request):
    """(calls, design, handle of the kind)."""
    from bayesbridge_amd import HipDenseDesignMatrix, _lib
    lib = _lib.load()
    design = HipDenseDesignMatrix(hc.design_matrix(), add_intercept=False)
    assert design.shape == (hc.N, hc.P)
    calls = hc.Calls(lib, hc.KINDS[request.param])
    h = hc.create(lib, request.param, design.handle)
    yield calls, design, h
    assert calls.destroy(h) == hc.OK


def test_refusals_of_a_live_handle(handle):
    calls, _, h = handle
    lib, prefix = calls.lib, 'bbx_%s_' % calls.family
    before = lib.bbx_launch_count()
    for name, required in hc.REQUIRED.items():
        if name == 'nuts_doubling':      # asks for nuts_begin first: below
            continue
        for arg in required:
            assert calls.call(name, h, **{arg: None}) == (
                hc.ERR_INVALID, 'NULL argument'), (name, arg)
    assert calls.call('hmc_trajectory', h, n_step=-1) == (
        hc.ERR_INVALID, 'n_step < 0')
    for name in ('hessian_matvec', 'hessian_matvec_dev'):
        assert calls.call(name, h) == (
            hc.ERR_STATE, prefix + 'set_location has not succeeded'), name
    for name in ('nuts_doubling', 'nuts_sample'):
        assert calls.call(name, h) == (
            hc.ERR_STATE, prefix + 'nuts_begin has not succeeded'), name
    assert lib.bbx_launch_count() == before
    assert calls.call('nuts_begin', h)[0] == hc.OK
    before = lib.bbx_launch_count()
    assert calls.call('nuts_doubling', h, uniforms=None) == (
        hc.ERR_INVALID, 'NULL argument')
    assert calls.call('nuts_doubling', h, direction=0) == (
        hc.ERR_INVALID, 'direction must be 1 or -1')
    assert calls.call('nuts_doubling', h, height=-1) == (
        hc.ERR_INVALID, 'height outside [0, 10]')
    assert lib.bbx_launch_count() == before


def test_every_entry_point_refuses_a_handle_whose_design_is_gone(handle):
    calls, design, h = handle
    before = calls.lib.bbx_launch_count()
    design.__del__()
    for name in hc.SHARED:
        assert calls.call(name, h) == (
            hc.ERR_STATE, "the %s handle's design has been destroyed"
            % calls.family), name
    assert calls.lib.bbx_launch_count() == before
    # the fixture destroys the handle: that still succeeds


def test_host_and_device_likelihood_agree_bit_for_bit(handle):
    import torch
    calls, _, h = handle
    beta = np.array([.3, -.2, .1])
    ll, ll_grad, ll_dev = c_double(), c_double(), c_double()
    grad = np.empty(hc.P)
    assert calls.call('loglik_grad', h, beta=hc._ptr(beta),
                      loglik=byref(ll))[0] == hc.OK
    assert calls.call('loglik_grad', h, beta=hc._ptr(beta),
                      loglik=byref(ll_grad), grad=hc._ptr(grad))[0] == hc.OK
    assert np.isfinite(ll.value) and ll.value == ll_grad.value
    d_beta = torch.from_numpy(beta).to('cuda:0')
    d_grad = torch.zeros(hc.P, dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    assert calls.call('loglik_grad_dev', h, d_beta=c_void_p(d_beta.data_ptr()),
                      loglik=byref(ll_dev),
                      d_grad=c_void_p(d_grad.data_ptr()))[0] == hc.OK
    assert ll_dev.value == ll.value
    assert np.array_equal(d_grad.cpu().numpy(), grad)
