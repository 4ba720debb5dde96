"""Writes tests/golden/glm_rows_parent_bits.npz: what the row-wise GLM handles
(logit, Poisson, negative binomial) computed on an MI355X in the build of the
commit BEFORE their three row kernels were folded onto csrc/glm_rows.hpp -- the
log-likelihood and gradient at a seeded beta, one Hessian-vector product
there, the end state of a 3-step device trajectory, the negative binomial's
dispersion sums and its gradient after set_dispersion, and the Poisson
overflow rule -- on a seeded dense float64 design with 5 columns, at the row
counts where the row kernel changes path.  tests/test_hip_glm_rows_bits.py
imports `compute` and compares bit for bit.

    python tests/golden/make_glm_rows_bits.py OUT.npz     (needs a GPU)

To write the fixture again, run this file from this tree with the package of
the parent commit's build first on PYTHONPATH: the row counts come from this
tree's headers (the parent had the same U, 4, in each of its three files)."""
import os
import re
import sys
import warnings
from ctypes import byref, c_void_p

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..',
                    'bayes-bridge_amd', 'csrc')
FAMILIES = ('logit', 'poisson', 'negbin')
P = 5                    # columns of the design: the intercept and 4 more


def _constant(name, src):
    text = open(os.path.join(CSRC, src)).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))


def rows():
    """The row counts, from the headers: row i belongs to workgroup
    (i / VEC_BLOCK) % NPART and a thread keeps GLM_ROW_U rows of consecutive
    laps in flight."""
    vec_block = _constant('VEC_BLOCK', 'common.hpp')
    lap = _constant('NPART', 'common.hpp') * vec_block
    u = _constant('GLM_ROW_U', 'glm_rows.hpp')
    return (1, vec_block - 1, vec_block + 1, lap + 1, u * lap + 3)


def _ptr(a):
    return a.ctypes.data_as(c_void_p)


def _model(family, n, rng, offset_of_row=None):
    """The family's device model on n seeded rows; offset_of_row = (row,
    value) replaces one row's offset before the handle is made."""
    from bayesbridge_amd import (HipDenseDesignMatrix, RegressionModel,
                                 design_matrix)
    X = rng.normal(size=(n, P - 1))
    # The design classes drop columns that are constant over the rows, as
    # hand-made intercepts, and every column of a single row is constant.  The
    # one-row case is about the row kernel, so it keeps its 5 columns: the
    # filter is switched off while the design is built, as the n = 1 cases of
    # tests/test_hip_poisson.py do with monkeypatch.
    keep = design_matrix.remove_intercept_indicator
    if n == 1:
        design_matrix.remove_intercept_indicator = lambda X: X
    try:
        dsn = HipDenseDesignMatrix(X, add_intercept=True,
                                   center_predictor=True,
                                   storage_dtype='float64')
    finally:
        design_matrix.remove_intercept_indicator = keep
    assert dsn.shape == (n, P)
    rate = np.exp(.2 + X.dot(rng.normal(size=P - 1) * .3))
    e = rng.uniform(.5, 2., n)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if family == 'logit':
            m = rng.integers(1, 6, n).astype(np.float64)
            y = rng.binomial(m.astype(np.int64), rate / (1. + rate))
            model = RegressionModel((y.astype(np.float64), m), dsn, 'logit')
        elif family == 'poisson':
            y = rng.poisson(rate * e).astype(np.float64)
            model = RegressionModel((y, e), dsn, 'poisson')
        else:
            y = rng.poisson(rate * e * rng.gamma(2., .5, n))
            model = RegressionModel((y.astype(np.float64), e), dsn, 'negbin',
                                    dispersion=2.)
    if offset_of_row:
        model.log_exposure[offset_of_row[0]] = offset_of_row[1]
    return model


def compute(family, n):
    """{name: float64 array} of family's handle on n rows."""
    rng = np.random.default_rng([FAMILIES.index(family), n])
    model = _model(family, n, rng)
    beta, v = rng.normal(size=P) * .3, rng.normal(size=P)
    out = {}
    ll, grad = model.hamiltonian_loglik_and_gradient(beta)
    out['loglik'], out['grad'] = np.array([ll]), grad
    out['hessian_matvec'] = model.get_hessian_matvec_operator(beta)(v)
    scale, pp = np.exp(rng.normal(size=P) * .3) * .3, np.ones(P)
    q0, p0 = beta / scale, rng.normal(size=P)
    logp0 = ll - .5 * np.sum(pp * q0 ** 2)
    grad0 = scale * grad - pp * q0
    # (the curvature grows with n: a step well inside the stability limit)
    dt = .02 / np.sqrt(n)
    tr = model.hmc_trajectory(dt, 3, scale, pp, q0, p0, logp0, grad0)
    assert tr['n_steps'] == 3 and not tr['instability'], (family, n, tr)
    out.update({'traj_q': tr['q'], 'traj_p': tr['p'],
                'traj_logp': np.array([tr['logp']]), 'traj_grad': tr['grad']})
    if family == 'negbin':
        out['disp_k1'] = np.array([model.dispersion_loglik(beta, .7)])
        out['disp_k3'] = model.dispersion_loglik(None, np.array([.05, 3., 1e4]))
        model.dispersion = 7.
        ll, grad = model.hamiltonian_loglik_and_gradient(beta)
        out['loglik_r7'], out['grad_r7'] = np.array([ll]), grad
    return out


def compute_poisson_overflow(n):
    """The overflow rows of a Poisson handle on n rows: an offset that puts
    eta + o past exp's range (709.79) -- (loglik, gradient) as the model
    returns them; an infinite intercept, eta = +inf in every row, where ll_i is
    NaN (y eta - mu = inf - inf, or 0 inf) and only the test mu == inf raises
    the flag; and an offset of +inf, which create refuses: its status and
    whether it left a handle."""
    from bayesbridge_amd import _lib
    rng = np.random.default_rng([len(FAMILIES), n])
    model = _model('poisson', n, rng, offset_of_row=(n // 3, 800.))
    beta = rng.normal(size=P) * .3
    got = model.compute_loglik_and_gradient(beta)
    inf_beta = beta.copy()
    inf_beta[0] = np.inf
    got_inf = model.compute_loglik_and_gradient(inf_beta)
    inf_o = model.log_exposure.copy()
    inf_o[n // 2] = np.inf
    h = c_void_p()
    status = _lib.load().bbx_poisson_create(
        model.design.handle, _ptr(model.y), _ptr(inf_o), byref(h))
    return {'overflow': got, 'inf_eta': got_inf, 'inf_offset_status': status,
            'inf_offset_handle': bool(h.value),
            'inf_offset_error': _lib.last_error()}


if __name__ == "__main__":
    out = {}
    for family in FAMILIES:
        for n in rows():
            for key, val in compute(family, n).items():
                out['%s_%d_%s' % (family, n, key)] = val
    over = compute_poisson_overflow(rows()[2])
    assert over['overflow'] == (-np.inf, None), over
    assert over['inf_eta'] == (-np.inf, None), over
    assert not over['inf_offset_handle'], over
    assert 'log_exposure' in over['inf_offset_error'], over
    out['poisson_inf_offset_status'] = np.array([over['inf_offset_status']],
                                                dtype=np.float64)
    np.savez(sys.argv[1], **out)
    print('wrote', sys.argv[1], len(out), 'arrays',
          sum(v.size for v in out.values()), 'doubles')
