"""The ten entry points every Hamiltonian likelihood handle shares
(bbx_<family>_*: include/bbx.h), callable by name with named arguments, and
the smallest handle of each kind: n = 8 rows, P = 3, the Cox kinds with 4
events, the stratified kinds with 2 strata of 4 rows.  Used by
test_ham_cabi_null.py (CPU) and test_hip_ham_cabi.py (GPU)."""
from ctypes import byref, c_double, c_void_p

import numpy as np

OK, ERR_INVALID, ERR_STATE = 0, -1, -5
N, P = 8, 3

# kind of handle -> the family its entry points and messages are named after
KINDS = {'cox': 'cox', 'strat_cox': 'cox', 'logit': 'logit',
         'poisson': 'poisson', 'cpoisson': 'cpoisson'}

# entry point -> the pointer arguments that must not be NULL
REQUIRED = {
    'loglik_grad_dev': ('d_beta', 'loglik'),
    'loglik_grad': ('beta', 'loglik'),
    'set_location': ('beta',),
    'hessian_matvec_dev': ('d_v', 'd_out'),
    'hessian_matvec': ('v', 'out'),
    'hmc_trajectory': ('precond_scale', 'prior_prec', 'q0', 'p0', 'grad0'),
    'nuts_begin': ('precond_scale', 'prior_prec', 'q0', 'p0', 'grad0'),
    'nuts_doubling': ('uniforms',),
    'nuts_sample': (),
}
SHARED = tuple(REQUIRED)      # and destroy


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


class Calls():
    """call(name, handle, **overrides) -> (status, bbx_last_error()).  The
    default arguments are valid host arrays; the `_dev` entry points take them
    only where the call is refused on the host, before any launch."""

    def __init__(self, lib, family):
        self.lib, self.family = lib, family
        self.vec, self.out = np.full(P, .1), np.empty(P)
        self.ones, self.unif = np.ones(P), np.full(1, .5)
        self.loglik = c_double()

    def defaults(self, name):
        v, one, out = _ptr(self.vec), _ptr(self.ones), _ptr(self.out)
        ll = byref(self.loglik)
        start = dict(precond_scale=one, prior_prec=one, q0=v, p0=v, logp0=0.,
                     grad0=v)
        return {
            'loglik_grad_dev': dict(d_beta=v, loglik=ll, d_grad=None),
            'loglik_grad': dict(beta=v, loglik=ll, grad=None),
            'set_location': dict(beta=v),
            'hessian_matvec_dev': dict(d_v=v, d_out=out),
            'hessian_matvec': dict(v=v, out=out),
            'hmc_trajectory': dict(
                dt=.1, n_step=1, **start, hamiltonian_tol=100., q=None, p=None,
                logp=None, grad=None, n_grad_evals=None, instability=None,
                hamiltonian=None),
            'nuts_begin': dict(**start, joint_logp0=0.,
                               joint_logp_threshold=-1., hamiltonian_tol=100.),
            'nuts_doubling': dict(
                dt=.1, direction=1, height=0, uniforms=_ptr(self.unif),
                n_uniform_used=None, n_steps=None, flags=None, tree=None,
                averages=None),
            'nuts_sample': dict(q=None, logp=None, grad=None),
        }[name]

    def call(self, name, handle, **overrides):
        args = self.defaults(name)
        assert set(overrides) <= set(args), (name, overrides)
        args.update(overrides)
        fn = getattr(self.lib, 'bbx_%s_%s' % (self.family, name))
        status = fn(handle, *args.values())
        return status, self.lib.bbx_last_error().decode()

    def destroy(self, handle):
        return getattr(self.lib, 'bbx_%s_destroy' % self.family)(handle)


def design_matrix():
    return np.random.RandomState(0).randn(N, P)


def create(lib, kind, design_handle):
    """A handle of `kind` on a design of N rows without an intercept."""
    from bayesbridge_amd.model import (cox_risk_sets,
                                       cox_stratified_risk_sets)
    inf = float('inf')
    handle = c_void_p()
    y = np.array([0., 1., 2., 0., 3., 1., 0., 2.])
    log_exposure = np.linspace(-.2, .2, N)
    sptr = np.array([0, 4, 8], dtype=np.int64)
    if kind == 'cox':
        n_event, start, end, n_app = cox_risk_sets(
            np.array([1., 2., 3., 4., inf, inf, inf, inf]),
            np.array([inf, inf, inf, inf, 5., 4.5, 3.5, 2.5]))
        assert n_event == 4
        i32 = [np.ascontiguousarray(a, dtype=np.int32)
               for a in (start, end, n_app)]
        st = lib.bbx_cox_create(design_handle, n_event,
                                *[_ptr(a) for a in i32], byref(handle))
    elif kind == 'strat_cox':
        ptr, sne, start, end, last_set = cox_stratified_risk_sets(
            np.array([1., 2., inf, inf, 1., 2., inf, inf]),
            np.array([inf, inf, 3., 1.5, inf, inf, 3., 1.5]),
            np.repeat([0, 1], 4))
        assert np.array_equal(ptr, sptr) and int(np.sum(sne)) == 4
        i32 = [np.ascontiguousarray(a, dtype=np.int32)
               for a in (sne, start, end, last_set)]
        st = lib.bbx_cox_create_stratified(
            design_handle, 2, _ptr(sptr), *[_ptr(a) for a in i32],
            byref(handle))
    elif kind == 'logit':
        n_trial = np.array([1., 1., 2., 1., 3., 1., 1., 3.])
        st = lib.bbx_logit_create(design_handle, _ptr(y), _ptr(n_trial),
                                  byref(handle))
    elif kind == 'poisson':
        st = lib.bbx_poisson_create(design_handle, _ptr(y),
                                    _ptr(log_exposure), byref(handle))
    else:
        assert kind == 'cpoisson'
        st = lib.bbx_cpoisson_create(design_handle, _ptr(y),
                                     _ptr(log_exposure), 2, _ptr(sptr),
                                     byref(handle))
    assert st == OK, lib.bbx_last_error()
    return handle
