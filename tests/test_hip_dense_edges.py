"""GPU: the dense design's kernels (csrc/dense.hip) where an off-by-one stays
silent at comfortable shapes -- one to five rows, one column, a column group
with two live threads, workgroups with no row, one row or an odd number of
rows, chunks without rows, the switches between the register kernel, the ring
kernel and the two separate passes, the ingest's second grid-stride trip.

Two kinds of case, both from tests/dense_ld_oracle.py (whose host side
tests/test_dense_ld_oracle.py checks on the CPU):
  * integer cases: every partial sum in every order is an integer below 2^53,
    so the device result must EQUAL the int64 result;
  * Gaussian cases on a centred design with intercept: compared with the
    long-double product of stored(...) -- the host statement of the ingest
    kernel, never toarray(), which goes through the dot under test -- under
    bounds that are derived (gamma_k of a k-term sum in any order), per
    component, not measured.
LABNOTES, "Dense products at kernel edges", has the case table and the
observed error / bound ratios."""
import numpy as np
import pytest

import dense_ld_oracle as dlo
import oracle
from helpers import cg_inputs
from test_hip_cg_sampler import _assert_close

pytestmark = pytest.mark.gpu

STORAGES = ('float32', 'float64')


def _design(X, in_dtype, storage, centred, intercept):
    """The HIP design of the predictors X given as `in_dtype`.  Constant
    columns (every column when n = 1, or by chance in a few integer rows)
    would be dropped by the constructor: such an X is adopted from device
    memory instead, with the offsets the constructor would have formed."""
    from bayesbridge_amd import HipDenseDesignMatrix
    X = np.ascontiguousarray(np.asarray(X).astype(in_dtype))
    n, p = X.shape
    P = p + bool(intercept)
    small = n <= 8 or p == 1
    if not (small and np.any(np.var(X, axis=0) < n * 2. ** -52)):
        d = HipDenseDesignMatrix(X, center_predictor=centred,
                                 add_intercept=intercept,
                                 storage_dtype=storage)
        if centred:
            assert np.array_equal(d.column_offset,
                                  dlo.column_offset(X, in_dtype))
    else:
        import torch
        t = torch.from_numpy(X).cuda()
        off = (torch.from_numpy(dlo.column_offset(X, in_dtype)).cuda()
               if centred else None)
        d = HipDenseDesignMatrix.from_device_array(
            n, p, t.data_ptr(), off.data_ptr() if centred else None,
            add_intercept=intercept, in_dtype=in_dtype, storage_dtype=storage)
        torch.cuda.synchronize()
    assert d.shape == (n, P)
    return d


def _int_design(c, storage):
    return _design(c.X, 'float32', storage, False, c.intercept)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _gram(d, omega, v):
    """gram_matvec, counted as one dot and one Tdot, the same bits twice."""
    before = d.get_dot_count()
    g = d.gram_matvec(omega, v)
    after = d.get_dot_count()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 1)
    assert np.array_equal(d.gram_matvec(omega, v), g)
    return g


def _within(out, ref, bound, what):
    r = dlo.ratio(out, ref, bound)
    print("ratio %s: %.2e of the bound" % (what, r))
    return r <= 1.


# ---- a. the ingest, bit for bit ---------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("in_dtype", ['float32', 'float64'])
def test_ingest_stores_what_the_host_statement_stores(in_dtype, storage):
    for n, p in ((3, 7), (5, 9), (67, 17)):
        X = dlo.gauss_case(n, p + 1).X
        for centred in (False, True):
            for intercept in (False, True):
                want = dlo.stored(X, in_dtype, storage, centred, intercept)
                d = _design(X, in_dtype, storage, centred, intercept)
                assert np.array_equal(d.toarray(), want), (
                    n, p, centred, intercept)
                # (a float32 array given to the constructor IS float32 input)
                assert (want.astype(np.float32) == want).all() == (
                    storage == 'float32' or (in_dtype == 'float32'
                                             and not centred))


# ---- b. dot and Tdot --------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("P", dlo.DOT_P)
def test_dot_and_tdot_are_exact_on_integer_cases(P, storage):
    for n in dlo.DOT_N:
        c = dlo.int_case(n, P)
        d = _int_design(c, storage)
        assert np.array_equal(d.dot(c.v), _f64(c.t)), (n, P)
        assert np.array_equal(d.Tdot(c.w), _f64(c.g)), (n, P)
        # a unit vector returns a stored column: the ingest at this shape
        e = np.zeros(P)
        e[P - 1] = 1.
        assert np.array_equal(d.dot(e), _f64(c.Xi[:, P - 1])), (n, P)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("P", dlo.GAUSS_P)
@pytest.mark.parametrize("n", dlo.GAUSS_N)
def test_dot_and_tdot_keep_the_derived_bounds(n, P, storage):
    c = dlo.gauss_case(n, P)
    Xt = dlo.stored(c.X, 'float64', storage, True, True)
    d = _design(c.X, 'float64', storage, True, True)
    t, g = d.dot(c.v), d.Tdot(c.w)
    assert _within(t, dlo.dot_ld(Xt, c.v), dlo.dot_bound(Xt, c.v),
                   "dot %dx%d %s" % (n, P, storage))
    assert _within(g, dlo.tdot_ld(Xt, c.w), dlo.tdot_bound(Xt, c.w),
                   "Tdot %dx%d %s" % (n, P, storage))
    assert np.array_equal(d.dot(c.v), t)
    assert np.array_equal(d.Tdot(c.w), g)


# ---- c. the single-pass operator --------------------------------------------
def _gauss_operator(n, P, storage):
    c = dlo.gauss_case(n, P)
    Xt = dlo.stored(c.X, 'float64', storage, True, True)
    d = _design(c.X, 'float64', storage, True, True)
    return _within(_gram(d, c.omega, c.v), dlo.op_ld(Xt, c.omega, c.v),
                   dlo.op_bound(Xt, c.omega, c.v),
                   "operator %dx%d %s" % (n, P, storage))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n", dlo.OP_ROW_N)
def test_operator_at_row_edges(n, storage):
    P = dlo.OP_ROW_P
    c = dlo.int_case(n, P)
    assert np.array_equal(_gram(_int_design(c, storage), c.omega, c.v),
                          _f64(c.op))
    assert (n, P) in dlo.op_gauss_cases()
    assert _gauss_operator(n, P, storage)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("n", dlo.LDS_N)
def test_operator_at_the_ring_lds_limit(n, storage):
    """2008 rows per workgroup: the last that the ring's LDS holds; 2009: back
    to the register kernel.  (16 MB of f32: the ingest takes four grid-stride
    trips.)"""
    c = dlo.int_case(n, dlo.LDS_P, intercept=True)
    d = _int_design(c, storage)
    assert np.array_equal(_gram(d, c.omega, c.v), _f64(c.op))
    assert np.array_equal(d.Tdot(c.w), _f64(c.g))
    assert np.array_equal(d.dot(c.v), _f64(c.t))


@pytest.mark.parametrize("P", dlo.OP_COL_P)
@pytest.mark.parametrize("n", dlo.OP_COL_N)
def test_operator_at_column_edges(n, P):
    """Both storage types on one integer case (building it is most of the
    time).  P = 8193 (ld 8200) is past the single pass: dot, then Tdot, the
    same answer and the same count."""
    c = dlo.int_case(n, P)
    for storage in STORAGES:
        d = _int_design(c, storage)
        assert np.array_equal(_gram(d, c.omega, c.v), _f64(c.op)), storage
        del d
        if (n, P) in dlo.op_gauss_cases():
            assert _gauss_operator(n, P, storage)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("P", [9, 4097])
def test_operator_on_both_sides_of_the_row_threshold(P, storage):
    """n = 4096: the single pass; the same columns without the last row: two
    kernels.  Both exact."""
    hi, lo = dlo.THRESHOLD_N[1], dlo.THRESHOLD_N[0]
    c = dlo.int_case(hi, P)
    assert np.array_equal(_gram(_int_design(c, storage), c.omega, c.v),
                          _f64(c.op))
    cut = dlo.int_products(c.Xi[:lo], c.v, c.w[:lo], c.omega[:lo],
                           c.addend[:lo])
    d = _design(c.X[:lo], 'float32', storage, False, c.intercept)
    assert np.array_equal(_gram(d, c.omega[:lo], c.v), _f64(cut.op))
    assert not np.array_equal(cut.op, c.op)


# ---- d. what only the CG loop reaches: twt_part and addend ------------------
@pytest.mark.parametrize("n,p,dtype", dlo.CG_CASES)
def test_cg_draw_with_a_warm_start_at_operator_edges(n, p, dtype):
    """One CG draw from a non-zero warm start (the initial residual runs the
    single pass with `addend`, every iteration takes <t, Omega t> from
    `twt_part`) against oracle.cg_sample, by the criteria of
    test_hip_cg_sampler.py: a single-row workgroup (4098), the ring with
    n_blk = 1 (16129), two f32 column groups (ld 4104), four f64 ones.  The
    matrix is exactly representable in f32.

    Local scales with log-sd .3 (as in the fold tests of
    test_hip_cg_sampler.py), not cg_inputs' default 1.5: with 1.5 the ORACLE's
    own stopping iteration on the 16129 x 40 problem moves over 80-84 between
    two hosts and under 2e-16 relative perturbations of Omega -- more than the
    3 the criterion allows there -- while with .3 it is the same in every such
    run (10, 21, 46, 45 iterations on the four problems): LABNOTES."""
    from bayesbridge_amd import HipCGSampler, HipDenseDesignMatrix
    rng = np.random.default_rng(n + p)
    X = rng.standard_normal((n, p)).astype(np.float32).astype(np.float64)
    inp = cg_inputs(n, p + 1, seed=3, lam_log_sd=.3)
    assert np.any(inp['coef_cg_init'] != 0)
    ora = oracle.OracleDenseDesign(X, center_predictor=False,
                                   add_intercept=True)
    atol = 10e-6 * np.sqrt(p + 1)
    c_o, i_o = oracle.cg_sample(
        ora, inp['obs_prec'], inp['prior_prec_sqrt'], inp['z'],
        inp['coef_cg_init'], inp['coef_scaled_sd'], inp['n_unshrunk'],
        inp['randn_n'], inp['randn_P'], 500, atol)
    hip = HipDenseDesignMatrix(X, center_predictor=False, add_intercept=True,
                               storage_dtype=dtype)

    class _Replay:
        def __init__(self, vecs): self.vecs = list(vecs)
        def __call__(self, size): return self.vecs.pop(0)
    orig = np.random.randn
    np.random.randn = _Replay([inp['randn_n'], inp['randn_P']])
    try:
        c_h, i_h = HipCGSampler(inp['n_unshrunk']).sample(
            hip, inp['obs_prec'], inp['prior_prec_sqrt'], inp['z'],
            coef_cg_init=inp['coef_cg_init'], precond_by='prior',
            coef_scaled_sd=inp['coef_scaled_sd'], maxiter=500, atol=atol)
    finally:
        np.random.randn = orig
    print("cg %dx%d %s: n_iter %d (oracle %d), max|dev - oracle| = %.2e "
          "(|coef| %.2e)" % (n, p, dtype, i_h['n_iter'], i_o['n_iter'],
                             np.abs(c_h - c_o).max(), np.abs(c_o).max()))
    _assert_close(c_h, i_h, c_o, i_o)
    assert hip.get_dot_count()[0] == hip.get_dot_count()[1] == i_h['n_iter'] + 1
