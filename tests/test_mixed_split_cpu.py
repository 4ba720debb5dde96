"""The split of a mixed design by value, X = B + D + S, on the CPU: the
decision (plan_hybrid) at equality and one off, and the parts (split_rows)
against SciPy.  Both are the code csrc/spmv_tiled.hip calls when it builds
HybridParts, reached through libbbx_layout.so (csrc/tiled_layout.cpp).

The rule (tiled_layout.hpp): a column is dense when it stores at least
max(n / 2, 1) values other than 1.0; at most HYB_FUSED_MAX_KD dense columns,
else none; the design is split when 2 (ones + dense) >= nnz, ones > 0 and
4 ones >= nnz - dense."""
import numpy as np
import pytest
from scipy import sparse

import mixed_ld_oracle as mo
from helpers import MixedSplitCpu, TiledLayoutCpu


@pytest.fixture(scope="module")
def cpu():
    return MixedSplitCpu()


def _entries(*groups):
    """(cols, vals) from (column, count, value) groups."""
    cols = np.concatenate([np.full(k, j, np.int32) for j, k, _ in groups])
    vals = np.concatenate([np.full(k, v, np.float64) for _, k, v in groups])
    return cols, vals


@pytest.mark.parametrize("n", [1, 2, 3, 130, 131])
def test_dense_rule_at_equality_and_one_below(cpu, n):
    """Column 1 stores exactly max(n / 2, 1) values other than 1.0, column 2
    one fewer (none at n <= 3); column 0 holds enough ones to split."""
    dense_min = max(n // 2, 1)
    cols, vals = _entries((0, 4 * n + 4, 1.), (1, dense_min, 2.5),
                          (2, dense_min - 1, -.5))
    got = cpu.plan(n, 3, cols, vals)
    assert got['dense_cols'] == [1]
    assert got['split']
    assert (got['ones_nnz'], got['dense_nnz'], got['rest_nnz']) == \
        (4 * n + 4, dense_min, dense_min - 1)
    # ones inside a dense column do not count towards the rule, and are B's
    cols, vals = _entries((0, 4 * n + 4, 1.), (1, dense_min - 1, 2.5),
                          (1, n, 1.))
    got = cpu.plan(n, 3, cols, vals)
    assert got['dense_cols'] == [] and got['dense_nnz'] == 0
    assert got['ones_nnz'] == 5 * n + 4 and got['rest_nnz'] == dense_min - 1


def _rest_groups(n, rest, first_col):
    """`rest` values other than 1.0 that stay OUTSIDE a dense block: spread
    over columns with fewer than max(n / 2, 1) each where that is possible
    (n >= 4); below that every valued column is a dense one, and the only
    valued rest is that of a block given up for its width -- more than
    HYB_FUSED_MAX_KD dense columns."""
    groups = []
    if n >= 4:
        per = n // 2 - 1
        j = first_col
        while rest > 0:
            k = min(per, rest)
            groups.append((j, k, -2.))
            rest -= k
            j += 1
        return groups, j
    width = 8193
    assert rest >= width
    for k in range(width):
        groups.append((first_col + k, 1 + (1 if k < rest - width else 0), -2.))
    assert rest - width <= width
    return groups, first_col + width


@pytest.mark.parametrize("n", [1, 2, 3, 130, 131])
def test_first_inequality_at_equality_and_one_entry_less(cpu, n):
    """2 (ones + dense) == nnz splits, one 1.0 fewer does not."""
    rest = 9000 if n < 4 else 40
    groups, p = _rest_groups(n, rest, 1)
    for ones, want in ((rest, True), (rest - 1, False)):
        cols, vals = _entries((0, ones, 1.), *groups)
        got = cpu.plan(n, p, cols, vals)
        assert got['dense_cols'] == [] and got['rest_nnz'] == rest, got
        assert 2 * (got['ones_nnz'] + got['dense_nnz']) - len(cols) == \
            (0 if want else -1)
        assert got['split'] is want, (n, ones, got)


@pytest.mark.parametrize("n", [130, 131])
def test_second_inequality_at_equality_and_one_entry_less(cpu, n):
    """4 ones == nnz - dense splits; one valued entry more (4 ones one short)
    or one 1.0 fewer does not (a full dense column keeps the first inequality
    satisfied)."""
    for ones, rest, short in ((10, 30, 0), (10, 31, -1), (9, 30, -3)):
        groups, p = _rest_groups(n, rest, 2)
        cols, vals = _entries((0, ones, 1.), (1, n, .25), *groups)
        got = cpu.plan(n, p, cols, vals)
        assert got['dense_cols'] == [1] and got['dense_nnz'] == n
        assert got['rest_nnz'] == rest
        assert 2 * (got['ones_nnz'] + got['dense_nnz']) >= len(cols)
        assert 4 * got['ones_nnz'] - (len(cols) - got['dense_nnz']) == short
        assert got['split'] is (short == 0), (n, ones, rest, got)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_below_four_rows_every_valued_column_is_a_dense_one(cpu, n):
    """max(n / 2, 1) = 1 for n <= 3: one stored value makes its column dense,
    so the second inequality (4 ones >= nnz - dense = ones) cannot fail there
    and has no equality case of its own."""
    cols, vals = _entries((0, 1, 1.), (1, 1, 3.), (2, 1, -1.), (3, 2, .5))
    got = cpu.plan(n, 4, cols, vals)
    assert got['dense_cols'] == [1, 2, 3] and got['rest_nnz'] == 0
    assert got['split']


@pytest.mark.parametrize("n", [1, 2, 3, 130, 131])
def test_a_design_without_a_single_one_is_not_split(cpu, n):
    """(A first version of the rule split such designs: the value-free part
    was empty and the build aborted.)"""
    cols, vals = _entries((0, n, .5), (1, n, -1.5), (2, max(n // 3, 1), 2.))
    got = cpu.plan(n, 3, cols, vals)
    assert got['ones_nnz'] == 0 and not got['split']
    # ... and one 1.0 is enough when the dense block carries the rest
    cols, vals = _entries((0, n, .5), (1, n, -1.5), (2, 1, 1.))
    got = cpu.plan(n, 3, cols, vals)
    assert got['split'] and got['ones_nnz'] == 1


def test_widest_dense_block_and_one_column_more(cpu):
    n = 2
    kd_max = cpu.plan(n, 1, [0], [1.])['max_kd']
    assert kd_max == 8192
    for kd, kept in ((kd_max, True), (kd_max + 1, False)):
        cols = np.concatenate((np.repeat(np.arange(kd, dtype=np.int32), n),
                               np.full(2 * n * kd, kd, np.int32)))
        vals = np.concatenate((np.full(n * kd, 1.5), np.ones(2 * n * kd)))
        got = cpu.plan(n, kd + 1, cols, vals)
        if kept:
            assert got['dense_cols'] == list(range(kd))
            assert got['dense_nnz'] == n * kd and got['rest_nnz'] == 0
        else:
            # the block is given up as a whole: its entries are valued rest
            assert got['dense_cols'] == []
            assert got['dense_nnz'] == 0 and got['rest_nnz'] == n * kd
        assert got['split']            # 2 ones >= nnz and 4 ones >= nnz


def _design_with_awkward_parts():
    """9 x 7: duplicates in every part, a dense column (4) whose 1.0 entries
    go to B, rows and columns that are empty in B but not in S (row 8, column
    6) and the other way round (row 7, column 0), an all-empty row (5)."""
    rows = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 6, 6, 7, 7, 8, 8, 8]
    cols = [0, 0, 2, 4, 1, 4, 4, 2, 4, 6, 0, 3, 4, 4, 4, 1, 4, 0, 4, 4, 6, 6]
    vals = [1, 1, .5, 2., 1, 1., 3., 1, -1., 7., 1, 1, 1., .25, .25, 1, 4.,
            1, 1., -2., 9., -9.]
    # (CSR by hand: the COO constructor would add the duplicates up)
    order = np.lexsort((cols, rows))
    indptr = np.zeros(10, np.int64)
    np.add.at(indptr, np.array(rows) + 1, 1)
    X = sparse.csr_matrix((np.array(vals, float)[order],
                           np.array(cols, np.int32)[order],
                           np.cumsum(indptr)), shape=(9, 7))
    assert X.nnz == len(vals)
    return X


def _transpose_keeping_duplicates(X):
    coo = X.tocoo()
    order = np.lexsort((coo.row, coo.col))      # stable counting-sort order
    indptr = np.zeros(X.shape[1] + 1, np.int64)
    np.add.at(indptr, coo.col + 1, 1)
    return sparse.csr_matrix((coo.data[order], coo.row[order].astype(np.int32),
                              np.cumsum(indptr)), shape=X.shape[::-1])


def test_parts_of_an_awkward_design_against_scipy(cpu):
    X = _design_with_awkward_parts()
    n, p = X.shape
    plan = cpu.plan(n, p, X.indices, X.data)
    # column 4: 7 values other than 1.0 (a duplicate pair among them) >= 9 / 2
    assert plan['dense_cols'] == [4] and plan['split']
    assert plan['ones_nnz'] == int((X.data == 1.).sum()) == 11
    assert plan['dense_nnz'] == 7 and plan['rest_nnz'] == 4
    Xt = _transpose_keeping_duplicates(X)
    D = np.zeros((n, p))
    m = (X.indices == 4) & (X.data != 1.)
    np.add.at(D, (np.repeat(np.arange(n), np.diff(X.indptr))[m], 4), X.data[m])
    for A, transpose in ((X, False), (Xt, True)):
        B, S = cpu.split(A, plan['dense_cols'], transpose, p)
        assert B.nnz == plan['ones_nnz'] and S.nnz == plan['rest_nnz']
        assert np.all(B.data == 1.) and not np.any(S.data == 1.)
        Dm = D.T if transpose else D
        assert np.array_equal(B.toarray() + S.toarray() + Dm, A.toarray())
        # duplicates stay separate stored entries, in stored order
        Bd, Sd = B.toarray(), S.toarray()
        if not transpose:
            assert Bd[0, 0] == 2. and B[0].nnz == 2
            assert Sd[8, 6] == 0. and S[8].nnz == 2          # 9 + (-9)
            assert list(S[8].data) == [9., -9.]
            # the dense column's ones are B's, its values nobody's here
            assert Bd[1, 4] == 1. and Bd[3, 4] == 1. and Sd[:, 4].sum() == 0.
            # empty in B but not in S, and the other way round
            assert B[8].nnz == 0 and S[8].nnz > 0
            assert B[:, 6].nnz == 0 and S[:, 6].nnz > 0
            assert S[7].nnz == 0 and B[7].nnz > 0
            assert S[:, 0].nnz == 0 and B[:, 0].nnz > 0
            assert B[5].nnz == 0 and S[5].nnz == 0


def test_valued_rest_is_empty_in_the_orientation_that_knows_the_dense_rows(cpu):
    """Every value other than 1.0 sits in dense columns: S is empty.  For X^T
    the dense columns of X are ROWS; the same arrays split as if they were an
    untransposed design would put those values into S."""
    c = mo.mixed_case(130, 20, 3, None, 'gauss', False, False)
    X = sparse.csr_matrix((c.vals, c.indices, c.indptr.astype(np.int64)),
                          shape=(c.n, c.p))
    Xt = _transpose_keeping_duplicates(X)
    plan = cpu.plan(c.n, c.p, c.indices, c.vals)
    assert plan['dense_cols'] == c.dense_cols and plan['rest_nnz'] == 0
    B, S = cpu.split(Xt, plan['dense_cols'], True, c.p)
    assert S.nnz == 0 and B.nnz == c.ones_nnz
    assert B[c.p_bin:].nnz > 0            # the dense columns' ones are B's rows
    _, S_wrong = cpu.split(Xt, plan['dense_cols'], False, c.n)
    assert S_wrong.nnz > 0


@pytest.mark.parametrize("flavour", ["int", "gauss"])
def test_oracle_cases_split_as_they_say_and_add_up_through_the_layout(cpu, flavour):
    """The cases of the device tests: the plan finds the split the oracle
    states, and B v + D v + S v through the tiled layout's CPU emulator is X v
    (both orientations)."""
    layout = TiledLayoutCpu()
    cases = (mo.separate_cases(flavour, 130) + mo.separate_cases(flavour, 257)
             + mo.separate_cases(flavour, 2) + mo.case8_cases(flavour)
             + [mo.mixed_case(5, 40, 1025, None, flavour, False, False),
                mo.mixed_case(130, 16130, 0, 'two', flavour, True,
                              flavour == 'gauss', 11)])
    for c in cases:
        plan = cpu.plan(c.n, c.p, c.indices, c.vals)
        assert plan['split'], (c.n, c.kd, c.s)
        assert plan['dense_cols'] == c.dense_cols
        assert (plan['ones_nnz'], plan['dense_nnz'], plan['rest_nnz']) == \
            (c.ones_nnz, c.dense_nnz, c.rest_nnz)
        X = sparse.csr_matrix((c.vals, c.indices, c.indptr.astype(np.int64)),
                              shape=(c.n, c.p))
        a = int(c.intercept)
        for A, transpose, x in ((X, False, c.v[a:]),
                                (_transpose_keeping_duplicates(X), True, c.w)):
            B, S = cpu.split(A, plan['dense_cols'], transpose, c.p)
            got = layout.matvec(B, x)[0]
            if S.nnz:
                got = got + layout.matvec(S, x)[0]
            Dm = sparse.csr_matrix(A - B - S)
            got = got + Dm @ x
            ref = A @ x
            assert np.abs(got - ref).max() <= 1e-12 * max(1., np.abs(ref).max())


def test_case_8_shape_has_an_empty_last_panel_in_its_valued_rest(cpu):
    """The shape the suite once faulted on: S of one step in one slice, two
    panels of 128 rows, nothing in the second -- a workgroup without a single
    step at the very end of the id and value streams (its dummy loads are
    what tiled_layout_selftest.cpp walks under AddressSanitizer)."""
    layout = TiledLayoutCpu()
    for c in mo.case8_cases('gauss'):
        X = sparse.csr_matrix((c.vals, c.indices, c.indptr.astype(np.int64)),
                              shape=(c.n, c.p))
        B, S = cpu.split(X, [], False, c.p)
        assert c.kd == 0 and S.nnz == c.rest_nnz > 0
        assert np.diff(S.indptr)[126:].sum() == 0
        _, meta = layout.matvec(S, c.v[int(c.intercept):])
        assert (meta['PR'], meta['G'], meta['n_quad'], meta['n_slice']) == \
            (128, 1, 1, 1)
