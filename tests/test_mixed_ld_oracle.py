"""The oracle of the mixed-design edge tests (mixed_ld_oracle.py) notices
faults: CPU only.  The device tests (test_hip_mixed_edges.py) compare against
these references within these bounds, so what has to be shown here is that a
kernel that drops a single entry cannot hide inside them."""
import numpy as np
import pytest

import mixed_ld_oracle as mo

GAUSS = mo.gaussian_cases()


def test_the_case_list_is_what_the_device_tests_run():
    assert len(GAUSS) == len(set(id(c) for c in GAUSS)) > 250
    assert all(c.flavour == 'gauss' for c in GAUSS)
    # every case carries a dense block or a valued rest: it IS a mixed design
    assert all(c.kd > 0 or c.rest_nnz > 0 for c in GAUSS)
    # the expected split adds up, and some dense-column entries are ones
    for c in GAUSS:
        assert c.ones_nnz + c.dense_nnz + c.rest_nnz == len(c.vals)
        if c.kd and c.n >= 64:
            assert c.ones_nnz > 4 * c.n and c.dense_nnz >= c.kd * (c.n // 2)


def test_planted_faults_clear_a_hundred_bounds_on_every_case():
    """Three faults in the REFERENCE -- an entry of S dropped, one row of one D
    column dropped, the last row of a hyb_dense_tdot chunk lost -- move the
    result by at least 100 allowed bounds (the allowed bound is twice the
    derived one).  Every Gaussian case carries at least one of them, every
    case with a dense block the two D faults, every case with S the S fault."""
    worst = {}
    for c in GAUSS:
        faults = mo.planted_faults(c)
        assert ('S entry' in faults) == (c.rest_nnz > 0), (c.n, c.kd, c.s)
        assert ('D row' in faults) == (c.kd > 0)
        assert ('chunk tail' in faults) == (c.kd > 0)
        assert faults
        ref = {'dot': mo.dot_ref(c, c.v), 'tdot': mo.tdot_ref(c, c.w)}
        bound = {'dot': mo.dot_bound(c, c.v), 'tdot': mo.tdot_bound(c, c.w)}
        for name, (prod, k) in faults.items():
            fn = mo.dot_ref if prod == 'dot' else mo.tdot_ref
            bad = fn(c, c.v if prod == 'dot' else c.w, drop=k)
            r = mo.ratio(bad.astype(np.float64), ref[prod],
                         mo.ALLOW * bound[prod])
            assert r >= mo.FAULT_SHARPNESS, (name, c.n, c.kd, c.s, r)
            worst[name] = min(worst.get(name, np.inf), r)
    print("smallest distance of a planted fault, in allowed bounds:", worst)


@pytest.mark.parametrize("order", ["stored", "reversed"])
def test_float64_sums_in_two_orders_stay_inside_the_derived_bound(order):
    """The bound is derived, not measured; this only checks that it is not
    wrong: plain float64 products in the stored and in the reversed order of
    the triplets lie within ONE bound of the long-double reference."""
    top = 0.
    for c in GAUSS[::7]:
        cc = c
        if order == "reversed":
            from types import SimpleNamespace
            cc = SimpleNamespace(**vars(c))
            cc.rows, cc.cols, cc.vals = c.rows[::-1], c.cols[::-1], c.vals[::-1]
        for got, ref, bound in (
                (mo.dot_ref(cc, c.v, np.float64), mo.dot_ref(c, c.v),
                 mo.dot_bound(c, c.v)),
                (mo.tdot_ref(cc, c.w, np.float64), mo.tdot_ref(c, c.w),
                 mo.tdot_bound(c, c.w)),
                (mo.gram_ref(cc, c.omega, c.v, np.float64),
                 mo.gram_ref(c, c.omega, c.v), mo.gram_bound(c, c.omega, c.v))):
            r = mo.ratio(got, ref, bound)
            assert r <= 1., (c.n, c.kd, c.s, r)
            top = max(top, r)
    print("largest float64 / bound ratio (%s order): %.3f" % (order, top))


def test_integer_references_are_exact_and_agree_with_long_double():
    for n in (2, 130, 257):
        for c in mo.separate_cases('int', n):
            t, tw, g = mo.int_reference(c)
            assert np.array_equal(t, mo.dot_ref(c, c.v).astype(np.float64))
            assert np.array_equal(tw, mo.tdot_ref(c, c.w).astype(np.float64))
            assert np.array_equal(
                g, mo.gram_ref(c, c.omega, c.v).astype(np.float64))
    big = mo.mixed_case(5, 40, 8192, None, 'int', False, False)
    mo.int_reference(big)                      # (asserts its head-room)


def test_chunk_tails_follow_the_kernels_even_rounding():
    # n = 513: ceil(513 / 256) = 3 rows, rounded to 4: chunks end at 3, 7, ...
    assert list(mo.tdot_chunk_last_rows(513)[:3]) == [3, 7, 11]
    assert mo.tdot_chunk_last_rows(513)[-1] == 512
    assert list(mo.tdot_chunk_last_rows(2)) == [1]
    assert list(mo.tdot_chunk_last_rows(1)) == [0]
    assert list(mo.tdot_chunk_last_rows(257)) == list(range(1, 257, 2)) + [256]
