"""CPU: the host side of the conditional Poisson model -- the NumPy oracle
(tests/cpoisson_oracle.py) against central differences, against the
unconditional Poisson oracle with profiled stratum intercepts and under shifts
of eta per stratum, cpoisson_preprocess, the factory's rules, the declared
entry points and the register / scratch use of the kernels in
csrc/cpoisson.hip."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import scipy.sparse as sparse

import cpoisson_oracle as cpo
import poisson_oracle as po
from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "bayes-bridge_amd", "csrc", "cpoisson.hip")


def _problem(seed=0, n_strata=25, p=5, exposure=True):
    rs = np.random.RandomState(seed)
    sizes = rs.randint(2, 7, n_strata)
    sptr = cpo.stratum_ptr_of(sizes)
    n = int(sptr[-1])
    X = rs.randn(n, p) * .5
    o = np.log(rs.uniform(.5, 2., n)) if exposure else np.zeros(n)
    alpha = np.repeat(rs.randn(n_strata) * 2., sizes)
    y = rs.poisson(np.exp(alpha + o + .3)).astype(np.float64)
    for s in range(n_strata):                 # every stratum has a count
        if y[sptr[s]:sptr[s + 1]].sum() == 0:
            y[sptr[s]] = 1.
    return cpo.design(X, False, False), X, y, o, sptr


def test_oracle_gradient_and_hessian_match_central_differences():
    D, X, y, o, sptr = _problem()
    p = X.shape[1]
    rs = np.random.RandomState(1)
    beta, v = rs.randn(p) * .3, rs.randn(p)
    ll, grad = cpo.loglik_grad(D, y, o, sptr, beta)
    assert ll <= 0.
    h = 1e-5
    num = np.array([
        (cpo.loglik_grad(D, y, o, sptr, beta + h * e)[0]
         - cpo.loglik_grad(D, y, o, sptr, beta - h * e)[0]) / (2 * h)
        for e in np.eye(p)])
    # O(h^2) truncation and eps / h rounding, both ~1e-10 of the values
    np.testing.assert_allclose(grad, num, rtol=1e-7, atol=1e-7)
    hv = cpo.hessian_matvec(D, y, o, sptr, beta, v)
    num = (cpo.loglik_grad(D, y, o, sptr, beta + h * v)[1]
           - cpo.loglik_grad(D, y, o, sptr, beta - h * v)[1]) / (2 * h)
    np.testing.assert_allclose(hv, num, rtol=1e-7, atol=1e-7)
    # f of the preconditioned coordinates: the chain rule and the prior
    scale, pp = np.exp(rs.randn(p) * .3), np.ones(p)
    f = cpo.precond_f(D, y, o, sptr, scale, pp)
    q = rs.randn(p) * .3
    num = np.array([(f(q + h * e)[0] - f(q - h * e)[0]) / (2 * h)
                    for e in np.eye(p)])
    np.testing.assert_allclose(f(q)[1], num, rtol=1e-7, atol=1e-7)
    # a centred design: the centring is a constant per column, which every
    # stratum's likelihood ignores
    Dc = cpo.design(X, True, False)
    llc, gradc = cpo.loglik_grad(Dc, y, o, sptr, beta)
    np.testing.assert_allclose(llc, ll, rtol=1e-12)
    np.testing.assert_allclose(gradc, grad, rtol=1e-9, atol=1e-11)


def test_profile_identity_with_the_unconditional_poisson_oracle():
    """With S_s = sum_{j in s} exp(a_j), the unconditional Poisson
    log-likelihood of poisson_oracle (sum y eta' - mu, its constant sum y o -
    log y! dropped) with a free intercept alpha_s per stratum, eta' = eta +
    alpha_s, is maximal over alpha at alpha_s = log(N_s / S_s), where the
    means of a stratum sum to N_s:

        U = sum_i y_i (eta_i + alpha_s) - sum_s N_s
          = sum_i y_i eta_i + sum_s N_s (log N_s - log S_s) - sum_s N_s.

    The conditional log-likelihood is

        C = sum_i y_i (a_i - log S_s) = sum_i y_i eta_i + sum_i y_i o_i
            - sum_s N_s log S_s,

    so C = U + sum_s (N_s - N_s log N_s) + sum_i y_i o_i (the offset term
    enters with a plus: the unconditional oracle dropped it).  At the profile
    the gradient of U in alpha is 0 and its gradient in beta is that of C."""
    for exposure in (True, False):
        D, X, y, o, sptr = _problem(seed=3, exposure=exposure)
        n, p = X.shape
        n_strata = len(sptr) - 1
        code = np.repeat(np.arange(n_strata), np.diff(sptr))
        Z = np.zeros((n, n_strata))
        Z[np.arange(n), code] = 1.
        D_aug = po.design(np.hstack((X, Z)), False, False)
        rs = np.random.RandomState(4)
        for beta in (rs.randn(p) * .3, rs.randn(p) * 1.5):
            a = X @ beta + o
            S = np.array([np.exp(a[sptr[s]:sptr[s + 1]]).sum()
                          for s in range(n_strata)])
            N = np.array([y[sptr[s]:sptr[s + 1]].sum()
                          for s in range(n_strata)])
            alpha = np.log(N / S)
            U, gU = po.loglik_grad(D_aug, y, o, np.concatenate((beta, alpha)))
            C, gC = cpo.loglik_grad(D, y, o, sptr, beta)
            const = np.sum(N - N * np.log(N)) + np.sum(y * o)
            print('conditional', C, 'profiled', U + const)
            np.testing.assert_allclose(C, U + const, rtol=1e-12)
            scale = np.abs(gC).max()
            np.testing.assert_allclose(gU[:p], gC, rtol=1e-10,
                                       atol=1e-12 * scale)
            assert np.abs(gU[p:]).max() < 1e-10 * N.max()


def test_invariance_to_a_constant_per_stratum():
    D, X, y, o, sptr = _problem(seed=5)
    p = X.shape[1]
    rs = np.random.RandomState(6)
    beta, v = rs.randn(p) * .4, rs.randn(p)
    ll, grad = cpo.loglik_grad(D, y, o, sptr, beta)
    hv = cpo.hessian_matvec(D, y, o, sptr, beta, v)
    for spread in (1., 300.):
        shift = np.repeat(rs.randn(len(sptr) - 1) * spread, np.diff(sptr))
        ll2, grad2 = cpo.loglik_grad(D, y, o + shift, sptr, beta)
        # a_i - L_s is formed from numbers of size |shift|: eps * spread
        tol = 1e-13 * max(spread, 1.)
        np.testing.assert_allclose(ll2, ll, rtol=tol * 10)
        np.testing.assert_allclose(grad2, grad, rtol=1e-9,
                                   atol=tol * 10 * np.abs(y).sum())
        hv2 = cpo.hessian_matvec(D, y, o + shift, sptr, beta, v)
        np.testing.assert_allclose(hv2, hv, rtol=1e-9,
                                   atol=tol * 10 * np.abs(y).sum())
    # the mutant with one global max loses the stratum shifted far down
    shift = np.repeat(np.where(np.arange(len(sptr) - 1) == 2, -800., 0.),
                      np.diff(sptr))
    ll3, grad3 = cpo.loglik_grad(D, y, o + shift, sptr, beta)
    np.testing.assert_allclose(ll3, ll, rtol=1e-11)
    bad = cpo.loglik_grad_global_max(D, y, o + shift, sptr, beta)
    assert not np.isfinite(bad[0])
    same = cpo.loglik_grad_global_max(D, y, o, sptr, beta)
    np.testing.assert_allclose(same[0], ll, rtol=1e-12)
    np.testing.assert_allclose(same[1], grad, rtol=1e-9, atol=1e-11)


def test_oracle_newton_and_model():
    D, X, y, o, sptr = _problem(seed=7, n_strata=120, p=3)
    beta, cov = cpo.newton_mle(D, y, o, sptr)
    assert np.abs(cpo.loglik_grad(D, y, o, sptr, beta)[1]).max() < 1e-9
    assert np.all(np.linalg.eigvalsh(cov) > 0)
    # y was simulated with no covariate effect
    assert np.all(np.abs(beta) < 5 * np.sqrt(np.diag(cov)))
    model = cpo.OracleModel(D, y, o, sptr)
    assert model.name == 'poisson' and not model.intercept_added
    assert model.n_pred == 3
    ll, none = model.compute_loglik_and_gradient(beta, loglik_only=True)
    assert none is None and ll == cpo.loglik_grad(D, y, o, sptr, beta)[0]
    v = np.arange(3.)
    assert np.array_equal(model.get_hessian_matvec_operator(beta)(v),
                          cpo.hessian_matvec(D, y, o, sptr, beta, v))
    scale, pp = np.ones(3), np.ones(3)
    f = cpo.precond_f(D, y, o, sptr, scale, pp)
    q0, p0 = beta.copy(), np.array([.3, -.2, .1])
    logp0, grad0 = f(q0)
    out = model.hmc_trajectory(.01, 5, scale, pp, q0, p0, logp0, grad0)
    want = cpo.trajectory(f, .01, 5, q0, p0, logp0, grad0)
    assert np.array_equal(out['q'], want[0]) and out['n_steps'] == 5


def _catch(fn, *args):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = fn(*args)
    return out, [str(w.message) for w in caught]


def test_preprocess_sorts_stably_and_drops_uninformative_strata():
    from bayesbridge_amd import cpoisson_preprocess
    #          0    1    2    3    4    5    6    7    8    9
    lab = np.array(['b', 'a', 'c', 'b', 'a', 'd', 'c', 'b', 'e', 'e'])
    y = np.array([1., 0., 0., 2., 3., 4., 0., 0., 1., 0.])
    e = np.arange(1., 11.)
    X = np.arange(20.).reshape(10, 2)
    (y2, e2, lab2, X2, keep), msgs = _catch(cpoisson_preprocess, y, e, lab, X)
    # 'c' has no count, 'd' is a single row; the others in np.unique order,
    # rows of a stratum in their original order
    assert keep.tolist() == [1, 4, 0, 3, 7, 8, 9]
    assert lab2.tolist() == ['a', 'a', 'b', 'b', 'b', 'e', 'e']
    assert np.array_equal(y2, y[keep]) and np.array_equal(e2, e[keep])
    assert np.array_equal(X2, X[keep])
    assert len(msgs) == 3
    assert 'sorted by stratum' in msgs[0]
    assert 'no positive count' in msgs[1] and 'removed' in msgs[1]
    assert 'single observation' in msgs[2] and 'removed' in msgs[2]
    # sparse X, no exposure
    (y3, e3, lab3, X3, keep3), _ = _catch(cpoisson_preprocess, y, None, lab,
                                          sparse.csr_matrix(X))
    assert e3 is None and np.array_equal(keep3, keep)
    assert sparse.issparse(X3) and np.array_equal(X3.toarray(), X[keep])
    # already in order with nothing to drop: no warning, nothing moves
    out, msgs = _catch(cpoisson_preprocess, y2, e2, lab2, X2)
    assert msgs == [] and np.array_equal(out[4], np.arange(7))
    assert out[3] is X2
    # each warning alone
    _, msgs = _catch(cpoisson_preprocess, [1., 1., 1., 1.], None,
                     [1, 0, 1, 0])
    assert len(msgs) == 1 and 'sorted' in msgs[0]
    _, msgs = _catch(cpoisson_preprocess, [1., 1., 0., 0.], None,
                     [0, 0, 1, 1])
    assert len(msgs) == 1 and 'no positive count' in msgs[0]
    (_, _, _, _, k), msgs = _catch(cpoisson_preprocess, [1., 1., 5.], None,
                                   [0, 0, 1])
    assert len(msgs) == 1 and 'single observation' in msgs[0]
    assert k.tolist() == [0, 1]
    # a single row without a count is dropped under the first reason only
    _, msgs = _catch(cpoisson_preprocess, [1., 1., 0.], None, [0, 0, 1])
    assert len(msgs) == 1 and 'no positive count' in msgs[0]
    with pytest.raises(ValueError):
        cpoisson_preprocess(y, e, lab[:9])
    with pytest.raises(ValueError):
        cpoisson_preprocess(y, e[:9], lab)


def _fake_design(n, p, intercept=False):
    from bayesbridge_amd.design_matrix import HipDesignMatrix

    class Design(HipDesignMatrix):       # no device: the checks come first
        shape = (n, p)
        intercept_added = intercept

        def __init__(self):
            self._h = None

    return Design()


def test_factory_and_model_rules():
    from bayesbridge_amd import PoissonModel, RegressionModel
    y = np.array([1., 0., 2., 0., 0., 3., 1.])
    e = np.array([1., .5, 2., 1., 3., .25, 1.])
    lab = np.array([3, 3, 5, 5, 5, 9, 9])
    d = _fake_design(7, 3)
    with warnings.catch_warnings():
        warnings.simplefilter('error')           # nothing to warn about
        m = RegressionModel((y, e, lab), d, 'poisson')
    assert m.name == 'poisson' and m._ham_prefix == 'bbx_cpoisson_'
    assert m.design is d and not m._poisson       # the handle: on first use
    assert np.array_equal(m.strata, lab)
    assert m.stratum_ptr.tolist() == [0, 2, 5, 7]
    assert m.stratum_ptr.dtype == np.int64
    assert m.stratum_total.tolist() == [1., 2., 4.]
    assert np.array_equal(m.log_exposure, np.log(e))
    m = RegressionModel((y, None, lab), d, 'poisson')
    assert np.array_equal(m.exposure, np.ones(7))
    m = PoissonModel(y, e, d, strata=lab)
    assert m.stratum_ptr.tolist() == [0, 2, 5, 7]
    # the one- and two-argument forms are the unstratified model
    for outcome in (y, (y, e)):
        plain = RegressionModel(outcome, d, 'poisson')
        assert plain.strata is None and plain._ham_prefix == 'bbx_poisson_'
    assert PoissonModel(y, e, d).strata is None
    # asking for an intercept warns and adds none (checked before any upload)
    with pytest.warns(UserWarning, match='Intercept is not identifiable'):
        m = RegressionModel((y, e, lab), d, 'poisson', add_intercept=True)
    assert not m.intercept_added
    # a prebuilt design: rows in order, nothing to drop, no intercept column
    with pytest.raises(ValueError, match='intercept'):
        RegressionModel((y, e, lab), _fake_design(7, 4, True), 'poisson')
    with pytest.raises(ValueError, match='prebuilt'):
        RegressionModel((y, e, lab[::-1]), d, 'poisson')          # not sorted
    with pytest.raises(ValueError, match='prebuilt'):
        RegressionModel((np.where(lab == 5, 0., y), e, lab), d, 'poisson')
    with pytest.raises(ValueError, match='prebuilt'):              # one row
        RegressionModel((y, e, np.array([3, 3, 5, 5, 5, 9, 10])), d, 'poisson')
    # the class itself refuses what its handle could not take
    with pytest.raises(ValueError, match='sorted by stratum'):
        PoissonModel(y, e, d, strata=lab[::-1])
    with pytest.raises(ValueError, match='no positive count'):
        PoissonModel(np.where(lab == 5, 0., y), e, d, strata=lab)
    with pytest.raises(ValueError, match='intercept'):
        PoissonModel(y, e, _fake_design(7, 4, True), strata=lab)
    with pytest.raises(ValueError):
        PoissonModel(y, e, d, strata=lab[:6])
    with pytest.raises(ValueError):
        PoissonModel(np.where(lab == 9, -1., y), e, d, strata=lab)


def test_stratified_poisson_keeps_the_poisson_sampler_rules():
    from bayesbridge_amd import SamplerOptions
    d = _fake_design(7, 3)
    d.is_sparse = False
    opt = SamplerOptions.pick_default_and_create(None, None, 'poisson', d)
    assert opt.coef_sampler_type == 'hmc' and opt.rng == 'reference'
    for method in ('cg', 'cholesky', 'woodbury'):
        with pytest.raises(ValueError, match="'hmc' or 'nuts'"):
            SamplerOptions.pick_default_and_create(method, None, 'poisson', d)


NAMES = ('create', 'destroy', 'loglik_grad', 'loglik_grad_dev',
         'set_location', 'hessian_matvec', 'hessian_matvec_dev',
         'hmc_trajectory', 'nuts_begin', 'nuts_doubling', 'nuts_sample')


def test_cpoisson_entry_points_are_declared_and_documented():
    from ctypes import c_int64
    from bayesbridge_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_cpoisson_\w+)\s*\(', header))
    assert declared == {'bbx_cpoisson_' + name for name in NAMES}
    lib = _lib.load()
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert getattr(lib, name).restype is not None
    # the same argument lists as the logit handle's
    sigs = _lib._declare(lib)
    for name in declared - {'bbx_cpoisson_create'}:
        assert sigs[name] == sigs[name.replace('bbx_cpoisson_', 'bbx_logit_')]
    hp = sigs['bbx_design_destroy'][0][0]
    create = sigs['bbx_cpoisson_create'][0]
    assert create[0] is hp and len(create) == 6 and create[3] is c_int64
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 111
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in declared:
        assert name in doc, name
    from bayesbridge_amd import cpoisson_preprocess, model
    assert cpoisson_preprocess is model.cpoisson_preprocess


def test_geometry_is_readable_and_consistent():
    text = open(SRC).read()
    geo = {name: int(re.search(r'constexpr int %s = (\d+);' % name,
                               text).group(1))
           for name in ('CP_G', 'CP_BLOCK', 'CP_E', 'CP_TILE', 'CP_U')}
    assert geo['CP_TILE'] == geo['CP_BLOCK'] * geo['CP_E']
    assert geo['CP_BLOCK'] % 64 == 0 and geo['CP_G'] % 64 == 0
    assert 'fp contract(off)' in text
    assert 'atomicAdd' not in text
    makefile = open(os.path.join(os.path.dirname(SRC), 'Makefile')).read()
    assert 'cpoisson.hip' in re.search(r'SRCS := (.*)', makefile).group(1)


def _resource_table(src, tmp_path):
    """The helper of test_cholesky_kernel_resources.py."""
    out = subprocess.run(
        [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950",
         "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
         str(tmp_path / "t.o")],
        capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    current, table = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            current = m.group(1)
            table[current] = {}
            continue
        m = re.search(
            r"remark:\s+([A-Za-z][A-Za-z ]*?(?: \[[^\]]*\])?): (\d+)", line)
        if m and current:
            table[current][m.group(1)] = int(m.group(2))
    return table


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cpoisson_kernels_use_no_scratch(tmp_path):
    table = _resource_table(SRC, tmp_path)
    # both operators of the two scan passes, the three modes of the row
    # kernel and the shared trajectory kernels
    assert sum("cp_agg_kernel" in k for k in table) == 2
    assert sum("cp_out_kernel" in k for k in table) == 2
    assert sum("cp_row_kernel" in k for k in table) == 3
    for k in ("cox_step1_kernel", "cox_post_a_kernel", "cox_post_b_kernel",
              "cox_finish_kernel", "cox_nuts_leaf_kernel",
              "cox_nuts_merge_a_kernel", "cox_nuts_merge_b_kernel"):
        assert any(k in name for name in table), (k, sorted(table))
    for name, res in table.items():
        print(name, res)
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= 64 * 1024, (name, res)
