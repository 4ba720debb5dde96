"""GPU: the products of a mixed design -- stored split by value, X = B + D + S
(csrc/spmv_tiled.hip HybridParts) -- at the edges of its parts, every form of
launch_dot_hybrid / launch_tdot_hybrid with the form ASSERTED from
hybrid_info ('dot_form', 'tdot_form') and tiled_info.

Designs come from mixed_ld_oracle.py through from_csr_arrays (constant columns
kept).  Integer flavour: X~ v, X~^T w and X~^T (Omega X~ v) equal the int64
products bit for bit.  Gaussian flavour: within twice the derived
componentwise bound of the long-double reference (observed / bound is
printed per test; the largest seen is in LABNOTES.md).  Every product is run
twice: same bits.

Which form runs (spmv_tiled.hip, launch_dot_hybrid):
    epi, fused_wave<gw>, fused_wg<g>   inside an operator application only
        (gram_matvec, the CG loop), no valued rest, B in one column group and
        at most 256 panels, and v[intercept:] 16-byte aligned: a design
        WITHOUT intercept through gram_matvec; with an intercept only the CG
        loop, whose internal vector starts one element in
    separate          everything else with B in one column group, <= 256 panels
    separate_slabs    B in several column groups, or more than 256 panels
A plain dot() is never inside an operator application: `separate` or
`separate_slabs`, and the Tdot that follows makes its own pass over D."""
import warnings

import numpy as np
import pytest

import mixed_ld_oracle as mo
from helpers import tiled_part_info

pytestmark = pytest.mark.gpu

NPART = 256


def _same_bits(a, b):
    return a.tobytes() == b.tobytes()


def _products(c, hip, dot_form, gram_forms):
    """dot, Tdot, gram_matvec (twice each) of one case with the forms asserted;
    returns the largest observed / derived-bound ratio (0 for integer cases,
    which must be exact)."""
    info = hip.hybrid_info
    assert info is not None, (c.n, c.kd, c.s)
    assert (info['ones_nnz'], info['dense_nnz'], info['rest_nnz'],
            info['dense_cols']) == (c.ones_nnz, c.dense_nnz, c.rest_nnz, c.kd)
    assert info['dot_form'] is None and info['tdot_form'] is None
    t = hip.dot(c.v)
    assert hip.hybrid_info['dot_form'] == dot_form, (c.n, c.kd, c.s)
    tw = hip.Tdot(c.w)
    assert hip.hybrid_info['tdot_form'] == 'tdot_separate'
    g = hip.gram_matvec(c.omega, c.v)
    info = hip.hybrid_info
    assert (info['dot_form'], info['tdot_form']) == gram_forms, (c.n, c.kd, c.s)
    # a product after an operator application must not reuse its partials
    tw2 = hip.Tdot(c.w)
    assert hip.hybrid_info['tdot_form'] == 'tdot_separate'
    assert _same_bits(tw2, tw)
    assert _same_bits(hip.dot(c.v), t)
    assert _same_bits(hip.gram_matvec(c.omega, c.v), g)
    if c.flavour == 'int':
        rt, rtw, rg = mo.int_reference(c)
        assert np.array_equal(t, rt), ('dot', c.n, c.kd, c.s)
        assert np.array_equal(tw, rtw), ('Tdot', c.n, c.kd, c.s)
        assert np.array_equal(g, rg), ('gram', c.n, c.kd, c.s)
        return 0.
    r = (mo.ratio(t, mo.dot_ref(c, c.v), mo.dot_bound(c, c.v)),
         mo.ratio(tw, mo.tdot_ref(c, c.w), mo.tdot_bound(c, c.w)),
         mo.ratio(g, mo.gram_ref(c, c.omega, c.v),
                  mo.gram_bound(c, c.omega, c.v)))
    assert max(r) <= mo.ALLOW, (r, c.n, c.kd, c.s, c.intercept, c.center)
    return max(r)


def _one_group_few_panels(hip):
    b = hip.tiled_info()['X']
    return b['G'] == 1 and b['grid'] <= NPART


SEPARATE = ('separate', ('separate', 'tdot_separate'))


# ---- separate: addend kernel + direct epilogue ---------------------------------
@pytest.mark.parametrize("n", mo.SEP_N)
@pytest.mark.parametrize("flavour", ["int", "gauss"])
def test_separate_kernels_at_the_addend_unroll_and_chunk_edges(flavour, n):
    """kd in {0, 1, 3, 4, 5, 8, 9} (the addend kernel's four-column unroll and
    its tail; kd = 0: null D, 8 bytes of LDS) x S absent / one step / two
    slices, n around one panel and around 2 x 256 row chunks of D^T w (odd n:
    the 8-byte path; even n: 16-byte loads and the single-row tail)."""
    top = 0.
    for c in mo.separate_cases(flavour, n):
        hip = mo.design(c)
        assert _one_group_few_panels(hip)
        if c.s is not None:
            s = tiled_part_info(hip, 6)
            assert s['G'] == 1
            if c.s == 'quad':
                assert (s['n_quad'], s['n_slice']) == (1, 1)
            elif n > 128:
                assert s['n_slice'] >= 2
        top = max(top, _products(c, hip, *SEPARATE))
    print("separate %s n=%d: largest observed / bound = %.3f" % (flavour, n, top))


@pytest.mark.parametrize("flavour", ["int", "gauss"])
def test_the_shape_of_the_recorded_fault_with_its_flag_combinations(flavour):
    """130 x 65 without a dense column, S of one step in one slice and an
    empty second panel (mixed case [8] of test_hip_operator.py): the second
    workgroup of S's launch has no step at all, and its ring's dummy loads
    read the 16 / 64 bytes behind the id / value streams -- which the layout
    now pads (tiled_layout.cpp)."""
    top = 0.
    for c in mo.case8_cases(flavour):
        hip = mo.design(c)
        s = tiled_part_info(hip, 6)
        assert (s['PR'], s['G'], s['n_quad'], s['n_slice']) == (128, 1, 1, 1)
        assert _one_group_few_panels(hip) and c.kd == 0
        top = max(top, _products(c, hip, *SEPARATE))
    print("case-8 shape %s: largest observed / bound = %.3f" % (flavour, top))


def test_second_lap_of_the_addend_kernels_grid():
    """n = 262 145 = 1024 x 256 + 1: the last row is the second trip of one
    thread of hyb_addend_kernel."""
    c = mo.mixed_case(262145, 4, 2, None, 'int', True, False)
    hip = mo.design(c)
    # (more than 256 panels of B: the slab form, the same addend kernel)
    form = 'separate' if _one_group_few_panels(hip) else 'separate_slabs'
    _products(c, hip, form, (form, 'tdot_separate'))


# ---- separate_slabs ---------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["int", "gauss"])
def test_slabs_with_two_column_groups_in_both_parts(flavour):
    c = mo.mixed_case(130, 16130, 0, 'two', flavour, True, flavour == 'gauss', 11)
    hip = mo.design(c)
    assert hip.tiled_info()['X']['G'] == 2
    assert tiled_part_info(hip, 6)['G'] == 2
    r = _products(c, hip, 'separate_slabs', ('separate_slabs', 'tdot_separate'))
    print("slabs G=2 %s: observed / bound = %.3f" % (flavour, r))


def test_more_panels_than_partial_slots_fall_to_the_slab_form(monkeypatch):
    """BBX_TILED_PR=128: 32 768 rows are 256 panels, the last size at which the
    operator application keeps the dense epilogue; 32 769 rows are 257."""
    monkeypatch.setenv("BBX_TILED_PR", "128")
    for n, forms in ((32768, ('epi', 'dw_reused')),
                     (32769, ('separate_slabs', 'tdot_separate'))):
        c = mo.mixed_case(n, 63, 2, None, 'int', False, False)
        hip = mo.design(c)
        b = hip.tiled_info()['X']
        assert b['PR'] == 128 and b['G'] == 1 and b['grid'] == -(-n // 128)
        _products(c, hip, 'separate' if n == 32768 else 'separate_slabs', forms)


# ---- epi: the dense block in the value-free kernel's epilogue ------------------------
@pytest.mark.parametrize("kd", mo.EPI_KD)
@pytest.mark.parametrize("flavour", ["int", "gauss"])
def test_dense_epilogue(flavour, kd):
    top = 0.
    for n in mo.EPI_N:
        c = mo.mixed_case(n, 40, kd, None, flavour, False, False)
        hip = mo.design(c)
        assert _one_group_few_panels(hip)
        top = max(top, _products(c, hip, 'separate', ('epi', 'dw_reused')))
    print("epi %s kd=%d: largest observed / bound = %.3f" % (flavour, kd, top))


# ---- fused_wave / fused_wg: one pass over the row-major block ---------------------------
def _wave_width(kd):
    ldp = (kd + 1) // 2
    return 1 if ldp <= 64 else 2 if ldp <= 128 else 4 if ldp <= 256 else 8


def _wg_width(kd):
    ldp = (kd + 1) // 2
    return 1 if ldp <= 1024 else 2 if ldp <= 2048 else 4


@pytest.mark.parametrize("kd", mo.WAVE_KD)
@pytest.mark.parametrize("flavour", ["int", "gauss"])
def test_fused_wave_per_row(flavour, kd):
    top = 0.
    form = 'fused_wave%d' % _wave_width(kd)
    for n in mo.WAVE_N:
        c = mo.mixed_case(n, 40, kd, None, flavour, False, False)
        hip = mo.design(c)
        assert _one_group_few_panels(hip)
        top = max(top, _products(c, hip, 'separate', (form, 'dw_reused')))
    print("%s %s kd=%d: largest observed / bound = %.3f" % (form, flavour, kd, top))


@pytest.mark.parametrize("n", mo.WAVE_LAP_N)
def test_fused_wave_one_lap_of_its_grid(n):
    """256 workgroups x 16 waves x 4 rows = 16 384 rows a lap."""
    c = mo.mixed_case(n, 40, 9, None, 'int', False, False)
    hip = mo.design(c)
    assert _one_group_few_panels(hip)
    _products(c, hip, 'separate', ('fused_wave1', 'dw_reused'))


@pytest.mark.parametrize("kd", mo.WG_KD)
def test_fused_workgroup_per_row_block(kd):
    top = 0.
    form = 'fused_wg%d' % _wg_width(kd)
    for n in mo.WG_N:
        for flavour in ('int',) + (('gauss',) if n == 5 else ()):
            c = mo.mixed_case(n, 40, kd, None, flavour, False, False)
            hip = mo.design(c)
            assert _one_group_few_panels(hip)
            top = max(top, _products(c, hip, 'separate', (form, 'dw_reused')))
    print("%s kd=%d: largest observed / bound = %.3f" % (form, kd, top))


# ---- with an intercept ---------------------------------------------------------------------
@pytest.mark.parametrize("kd,form", [(3, 'epi'), (9, 'fused_wave1'),
                                     (1025, 'fused_wg1')])
def test_with_an_intercept_only_the_cg_loop_reaches_the_one_pass_forms(kd, form):
    """launch_tiled: "inside the CG loop x is an internal buffer placed
    accordingly; a caller's v + 1 of a design with intercept is not, and takes
    the 8-byte path".  So gram_matvec of a caller's vector runs the separate
    kernels (bbx.h, bbx_design_gram_matvec), and a CG solve -- whose direction
    vector starts one element into its buffer -- the one-pass form."""
    from bayesbridge_amd import HipCGSampler
    c = mo.mixed_case(65, 40, kd, None, 'int', True, False)
    hip = mo.design(c)
    _products(c, hip, *SEPARATE)
    rng = np.random.default_rng(kd)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # the solve is cut at 2 steps
        HipCGSampler(1).sample(hip, c.omega, np.ones(c.P), rng.standard_normal(c.P),
                               maxiter=2, atol=1e-300, seed=kd)
    info = hip.hybrid_info
    assert (info['dot_form'], info['tdot_form']) == (form, 'dw_reused')
    # ... and the products after the solve are the exact ones again
    assert np.array_equal(hip.Tdot(c.w), mo.int_reference(c)[1])
    assert hip.hybrid_info['tdot_form'] == 'tdot_separate'


# ---- batches: K right-hand sides ---------------------------------------------------------
def _batch(hip, c, K):
    from bayesbridge_amd import HipChainBatch, HipGibbsChain
    chains = []
    for sd in range(K):
        ch = HipGibbsChain(hip, 'linear', c.w, sd_unshrunk=[np.inf],
                           bridge_exponent=.5, slab_size=2., seed=sd)
        ch.set_state(np.zeros(c.P), None, np.ones(c.P - 1), .07)
        ch.init_obs_prec()
        chains.append(ch)
    return HipChainBatch(chains, allow_slow=True)


@pytest.mark.parametrize("K,s", [(2, None), (4, None), (2, 'quad')])
@pytest.mark.parametrize("n", mo.BATCH_N)
def test_batched_products_of_split_designs(n, K, s):
    """hyb_addend_k_kernel, hyb_dense_tdot_k_kernel, hyb_dense_scatter_k_kernel
    (K = 2, 4 without S; K = 2 with S): every column is its int64 product, and
    permuted inputs give permuted outputs."""
    for kd in mo.BATCH_KD:
        if kd == 0 and s is None:
            continue                      # a binary design: not a split one
        c = mo.mixed_case(n, mo.P_BIN, kd, s, 'int', True, False)
        hip = mo.design(c)
        assert hip.hybrid_info['dense_cols'] == kd
        assert (hip.hybrid_info['rest_nnz'] > 0) == (s is not None)
        batch = _batch(hip, c, K)
        rng = np.random.default_rng([n, K, kd])
        v = rng.integers(-8, 9, (K, c.P)).astype(np.float64)
        w = rng.integers(-8, 9, (K, c.n)).astype(np.float64)
        got_v, got_w = batch.dot(v), batch.Tdot(w)
        for k in range(K):
            rt, rtw, _ = mo.int_reference(c, v[k], w[k])
            assert np.array_equal(got_v[k], rt), (kd, k)
            assert np.array_equal(got_w[k], rtw), (kd, k)
        perm = np.roll(np.arange(K), 1)
        assert np.array_equal(batch.dot(v[perm]), got_v[perm])
        assert np.array_equal(batch.Tdot(w[perm]), got_w[perm])
        assert _same_bits(batch.dot(v), got_v)
        assert _same_bits(batch.Tdot(w), got_w)
