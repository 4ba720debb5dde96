"""CPU: the host side of the batched dense edge tests (dense_batch_oracle.py)
checked on its own -- every constant of the geometry against the text of the
sources, the property each case is listed for, the padding condition of every
case, the 2^53 condition of the integer cases, the derived bounds against a
float64 replay of the kernels' blocking in three orders, and that replay with
one row, one slot, one unit or one chain's rowscale wrong against the same
bounds."""
import os
import re

import numpy as np
import pytest

import dense_batch_oracle as dbo
import dense_ld_oracle as dlo
from conftest import ROOT

CSRC = os.path.join(ROOT, "bayes-bridge_amd", "csrc")
F32, F64 = dbo.STORAGES


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) >= 1, pattern
    assert len(set(found)) == 1, (pattern, found)
    return found[0]


# ---- the geometry, from the sources -----------------------------------------
def test_geometry_constants_are_those_of_the_sources():
    src, common = _text("dense_batch.hip"), _text("common.hpp")
    flat = re.sub(r"\s+", " ", src)
    for name in ("DKT_D", "DKT_D2", "DKT_D2_F64"):
        assert int(_one(r"#define %s (\d+)\b" % name, src)) \
            == getattr(dbo, name), name
    for name in ("DK_TDOT_CHUNKS", "DK_DOT_WGS", "DKD_WAVES"):
        assert int(_one(r"constexpr int %s = (\d+);" % name, src)) \
            == getattr(dbo, name), name
    for name in ("DENSE_PAD_ROWS", "DENSE_BATCH_ROW_PAD", "NPART", "WAVE"):
        assert int(_one(r"constexpr int %s = (\d+);" % name, common)) \
            == getattr(dbo, name), name
    assert int(_one(r"constexpr int DENSE_BATCH_STRIDE = (\d+);", common)) \
        == dbo.DK_KS
    assert "constexpr int DK_KS = DENSE_BATCH_STRIDE;" in src
    # units per sweep and ring depth: the functions, as text and by value
    m = re.search(r"constexpr int dkd_cw\(int NG, int E\) \{ return NG \* E "
                  r"<= (\d+) \? (\d+) : (\d+); \}", flat)
    assert m, "dkd_cw"
    lim, wide, narrow = (int(a) for a in m.groups())
    for NG in (1, 2):
        for E in (2, 4):
            assert dbo.dkd_cw(NG, E) == (wide if NG * E <= lim else narrow)
    assert ("return NG == 1 ? DKT_D : (sizeof(T) == 8 ? DKT_D2_F64 : DKT_D2);"
            in flat)
    assert [dbo.depth(s, K) for s in dbo.STORAGES for K in (16, 32)] == [
        dbo.DKT_D, dbo.DKT_D2, dbo.DKT_D, dbo.DKT_D2_F64]
    assert set(dbo.depth(s, K) for s in dbo.STORAGES for K in dbo.WIDTHS) \
        == set(dbo.DEPTHS)
    # E, U
    assert "static constexpr int E = 16 / (int)sizeof(T);" in src
    assert "static constexpr int U = 16 * E;" in src
    assert [(dbo.elems(s), dbo.unit(s)) for s in dbo.STORAGES] == [
        (4, 64), (2, 32)]
    # a slot is four rows; a sweep issues D slots, then periods of D
    assert "sa += 4 * ldm;" in src and "sb += 4 * KS;" in src
    assert "const int n_period = (n_slot + D - 1) / D;" in src
    assert len(re.findall(r"for \(int kk = 0; kk < D; \+\+kk\) DKD_ISSUE\(kk\);",
                          src)) == 1
    assert "const int64_t r_ring = n_slot > 0 ? r_begin : 0;" in src
    assert dbo.SLOT_ROWS == 4
    # X^T W: the parts and the column blocks
    assert "const int64_t parts = (int64_t)DK_TDOT_CHUNKS * DKD_WAVES;" in src
    assert ("const int64_t rows_per_wave = ((h->n + parts - 1) / parts + 3) "
            "/ 4 * 4;") in flat
    assert ("const int n_colblk = (int)((h->dense_ld + unit * cw - 1) / "
            "(unit * cw));") in flat
    assert "const int chunk = (int)(blockIdx.x % DK_TDOT_CHUNKS);" in src
    assert ("((int64_t)chunk * DKD_WAVES + wave) * rows_per_wave;") in flat
    assert ("const int n_slot = r_end > r_begin ? (int)((r_end - r_begin + 3) "
            "/ 4) : 0;") in flat
    # X V: quarters of P, units of ldn over the workgroups, the tails
    assert ("const int64_t rows_per_wave = ((P + DKD_WAVES - 1) / DKD_WAVES "
            "+ 3) / 4 * 4;") in flat
    assert "const int64_t n_unit = ldn / DkT<T>::U;" in src
    assert ("const int64_t base = n_unit / gridDim.x, extra = n_unit % "
            "gridDim.x;") in flat
    assert "dim3(DK_DOT_WGS)" in src
    assert "for (; u + CW <= u1; u += CW) DKD_UNITS(CW);" in src
    assert sorted(re.findall(r"if \(u1 - u == (\d)\) DKD_UNITS\((\d)\);",
                             src)) == [('1', '1'), ('1', '1'), ('2', '2'),
                                       ('3', '3')]
    # the allocations the padding condition speaks about
    assert ("const int64_t ldn = (h->n + %d) / %d * %d;"
            % (dbo.LDN_ROUND - 1, dbo.LDN_ROUND, dbo.LDN_ROUND)) in src
    assert ("const int64_t rows = (h->dense_ld + %d) / %d * %d + "
            "DENSE_PAD_ROWS;" % (dbo.XT_ROW_ROUND - 1, dbo.XT_ROW_ROUND,
                                 dbo.XT_ROW_ROUND)) in src
    assert ("h->dense.alloc(el_out * (size_t)(n + DENSE_PAD_ROWS) * "
            "(size_t)h->dense_ld)") in re.sub(r"\s+", " ", _text("dense.hip"))
    batch = re.sub(r"\s+", " ", _text("batch.hip"))
    assert ": (size_t)(h->dense_ld + DENSE_BATCH_ROW_PAD + 2);" in batch
    assert ": (size_t)(h->n + DENSE_BATCH_ROW_PAD);" in batch
    assert ("n_chain != 2 && n_chain != 4 && n_chain != 8 && n_chain != 16 && "
            "n_chain != 32") in batch
    assert dbo.WIDTHS == (2, 4, 8, 16, 32)
    assert "h->dense_ld = (h->P + 7) / 8 * 8;" in _text("dense.hip")


def test_the_geometry_functions_on_hand_computed_shapes():
    g = dbo.tdot_geometry(200003, 38, F32, 16)
    assert g.rows_per_wave == 6252 and g.n_slot == [1563] * 31 + [1548]
    assert (g.ld, g.block, g.n_colblk, g.last_block_cols) == (40, 256, 1, 40)
    g = dbo.tdot_geometry(129, 257, F32, 32)
    assert (g.ld, g.block, g.n_colblk, g.last_block_cols) == (264, 128, 3, 8)
    h = dbo.dot_geometry(200003, 38, F32, 16)
    assert h.ldn == 200064 and h.n_unit == 3126
    assert sorted(set(h.counts)) == [12, 13] and h.widths == {4, 1}
    assert h.rows_per_wave == 12 and h.n_slot == [3, 3, 3, 1]
    assert h.quarter_rows == [12, 12, 12, 2]
    h = dbo.dot_geometry(65, 9, F64, 32)
    assert h.n_unit == 4 and h.unit_live_rows == [32, 32, 1, 0]
    assert h.widths == {1} and h.n_slot == [1, 1, 1, 0]


# ---- gap 1 of the record: what the older shapes reach -----------------------
def test_the_older_batch_shapes_never_run_the_three_unit_f32_tail():
    """test_hip_batch.py's dense shapes (and the 6000-, 3000- and 2500-row
    problems of its chain tests) give a workgroup of f32 X V 1, 2, 4 k or
    4 k + 1 units: dkd_dot_units<float, 3, 1> and the 4 + 2 split never ran
    before the unit cases of this module."""
    old = (37, 64, 4097, 5000, 20000, 140000, 200003, 263000, 6000, 3000, 2500)
    widths, counts = set(), set()
    for n in old:
        h = dbo.dot_geometry(n, 9, F32, 16)
        widths |= h.widths
        counts |= set(c % 4 for c in h.counts if c > 4)
    assert 3 not in widths and counts <= {0, 1}
    assert 3 in dbo.dot_geometry(49153, 9, F32, 16).widths


# ---- the cases have the properties they are listed for ----------------------
def _tdot(n, storage=F32, K=16, P=dbo.EDGE_P):
    return dbo.tdot_geometry(n, P, storage, K)


def test_tdot_row_cases():
    for storage in dbo.STORAGES:
        for K in dbo.TEST_K:
            s = {n: _tdot(n, storage, K) for n in dbo.TDOT_ROW_N}
            assert s[1].n_slot == [1] + 31 * [0] and s[1].last_part_rows == 1
            assert s[4].n_slot == [1] + 31 * [0] and s[4].last_part_rows == 4
            assert s[5].n_slot == [1, 1] + 30 * [0]
            assert s[5].last_part_rows == 1          # one row, then empty parts
            assert s[127].n_slot == 32 * [1] and s[127].last_part_rows == 3
            assert s[128].n_slot == 32 * [1] and s[128].last_part_rows == 4
            assert s[129].rows_per_wave == 8
            assert s[129].n_slot == 16 * [2] + [1] + 15 * [0]
            assert s[129].last_part_rows == 1


def test_tdot_ring_cases():
    assert dbo.RING_S == (4, 5, 6, 7, 10, 11, 12, 13)
    for storage in dbo.STORAGES:
        for K in dbo.TEST_K:
            D = dbo.depth(storage, K)
            assert D in dbo.DEPTHS
            for s in dbo.RING_S:
                assert 128 * s in dbo.TDOT_RING_N
                assert _tdot(128 * s, storage, K).n_slot == 32 * [s]
            # around one and two periods of THIS instantiation's ring
            assert {D - 1, D, D + 1, 2 * D, 2 * D + 1} <= set(dbo.RING_S)
            periods = {s: -(-s // D) for s in dbo.RING_S}
            assert periods[D] == 1 and periods[D + 1] == 2
            assert periods[2 * D] == 2 and periods[2 * D + 1] == 3
            lo, hi = _tdot(128 * D - 1, storage, K), _tdot(128 * D + 1, storage, K)
            assert lo.n_slot == 32 * [D] and lo.last_part_rows % 4 == 3
            assert hi.n_slot[hi.last_part] == -(-hi.last_part_rows // 4)
            assert hi.last_part_rows % 4 == 1 and hi.last_part < 31


def test_tdot_column_cases():
    want = {F32: {16: 256, 32: 128}, F64: {16: 128, 32: 128}}
    seen = {128: set(), 256: set()}
    for storage in dbo.STORAGES:
        for K in dbo.TEST_K:
            U = dbo.unit(storage)
            geo = {P: _tdot(dbo.TDOT_COL_N, storage, K, P)
                   for P in dbo.TDOT_COL_P}
            block = geo[1].block
            assert block == want[storage][max(K, 16)]
            lds = {g.ld for g in geo.values()}
            assert {8, U, U + 8, block - 8, block, block + 8} <= lds
            for g in geo.values():
                assert g.n_colblk == -(-g.ld // block)
                assert 0 < g.last_block_cols <= block
            assert geo[1].last_block_cols == 8
            over = [g for g in geo.values() if g.ld == block + 8][0]
            assert over.n_colblk == 2 and over.last_block_cols == 8
            full = [g for g in geo.values() if g.ld == block][0]
            assert full.n_colblk == 1 and full.last_block_cols == block
            seen[block].add(storage)
    assert seen[256] == {F32} and seen[128] == {F32, F64}


def test_dot_contraction_cases():
    n = dbo.DOT_CONTR_N
    for storage in dbo.STORAGES:
        for K in dbo.TEST_K:
            D = dbo.depth(storage, K)
            geo = {P: dbo.dot_geometry(n, P, storage, K)
                   for P in dbo.DOT_CONTR_P}
            assert geo[1].quarter_rows == [1, 0, 0, 0]
            assert geo[4].quarter_rows == [4, 0, 0, 0]
            assert geo[5].quarter_rows == [4, 1, 0, 0]
            assert geo[16].n_slot == [1, 1, 1, 1]
            assert geo[17].n_slot == [2, 2, 1, 0]
            assert geo[17].quarter_rows == [8, 8, 1, 0]
            for s in dbo.RING_S:
                assert geo[16 * s].n_slot == 4 * [s]
            one_more = geo[16 * D + 1]
            assert one_more.n_slot[0] == D + 1 and one_more.quarter_rows[3] < 4 * D
            h = geo[1]
            assert h.widths == {1} and max(h.counts) == 1
            live = [r for r in h.unit_live_rows]
            assert live == ([64, 1] if storage == F32 else [32, 32, 1, 0])


def test_dot_unit_cases_run_every_instantiated_width():
    """Per storage and number of groups: the union of the sweep widths over the
    unit cases is every width the kernel instantiates -- with the two
    storages, the two group counts and the two products, all eight kernel
    instantiations and every dkd_dot_units<T, C, NG> within them."""
    ran = {}
    for storage in dbo.STORAGES:
        for K in (2, 32):
            widths = set()
            for n in dbo.DOT_UNIT_N:
                assert K in dbo.case_widths(n)
                widths |= dbo.dot_geometry(n, dbo.EDGE_P, storage, K).widths
            CW = dbo.cw(storage, K)
            assert widths == set(range(1, CW + 1)), (storage, K, widths)
            ran[storage, dbo.groups(K)] = widths
    assert ran[F32, 1] == {1, 2, 3, 4} and ran[F32, 2] == {1, 2}
    assert ran[F64, 1] == ran[F64, 2] == {1, 2, 3, 4}
    # which case runs which (LABNOTES has this table)
    w = {(s, n): dbo.dot_geometry(n, 9, s, 2).widths
         for s in dbo.STORAGES for n in dbo.DOT_UNIT_N}
    assert [w[F32, n] for n in (16385, 49153, 81921)] == [
        {2, 1}, {4, 3}, {4, 2, 1}]
    assert [w[F64, n] for n in (8193, 24577, 40961)] == [
        {2, 1}, {4, 3}, {4, 2, 1}]
    assert [sorted(set(dbo.dot_geometry(n, 9, F32, 2).counts))
            for n in (16385, 49153, 81921)] == [[1, 2], [3, 4], [5, 6]]
    assert dbo.BIG_N == (40961, 49153, 81921)
    assert max(dbo.DOT_UNIT_N) * dlo.ld_of(dbo.EDGE_P) == 81921 * 16


def test_every_case_meets_the_padding_condition():
    cases = dbo.all_cases()
    assert len(cases) == len(set(cases)) >= 45
    for n, P in cases:
        for storage in dbo.STORAGES:
            for K in dbo.WIDTHS:
                dbo.assert_padding(n, P, storage, K)
    # the condition has teeth: a ring twice as deep would leave X's padding
    # at the narrowest rows (ld 8: a 256-column load spans 32 rows)
    D = 6
    assert dbo.rows_read_end(0, 1, D) == 4 * 2 * D
    assert dbo.issued_slots(1, D) - 1 == 2 * D - 1
    assert dbo.issued_slots(D, D) - D == D
    assert dbo.issued_slots(0, D) == D
    end = dbo.rows_read_end(0, 1, 4 * dbo.DENSE_PAD_ROWS)
    assert (end - 1) * 8 + 256 > (1 + dbo.DENSE_PAD_ROWS) * 8


# ---- the integer cases ------------------------------------------------------
def test_every_small_integer_case_meets_the_2_53_condition():
    """int_batch asserts it when a case is built; here for every case but the
    six unit cases, and for those by the bound on their inputs: entries and
    vectors <= 8, rowscales <= 4, so |t| <= 64 ld and sum omega t^2 <=
    4 n (64 ld)^2."""
    worst = 0
    for n, P in dbo.all_cases():
        if n in dbo.DOT_UNIT_N:
            assert 4 * n * (64 * dlo.ld_of(P)) ** 2 < 2 ** 53
            continue
        for K in dbo.TEST_K:
            b = dbo.int_batch(n, P, K)
            worst = max(worst, b.abs_max)
        assert np.array_equal(b.T[1], b.Xi.astype(np.float64) @ b.V[1])
        assert np.array_equal(b.G[0], b.W[0] @ b.Xi.astype(np.float64))
        assert np.array_equal(b.TWT, (b.OM * b.T * b.T).sum(axis=1))
    assert worst < 2 ** 53
    b = dbo.int_batch(129, 33, 32)
    assert b.V.shape == (32, 33) and b.OM.min() == 1 and b.OM.max() == 4
    assert len({row.tobytes() for row in b.V}) == 32


# ---- the bounds against a float64 replay of the kernels' blocking -----------
NEG_CASES = ((129, 129), (641, 9), (65, 97))


def _ratios(b, T, TS, TWT):
    return (dlo.ratio(T, b.T, b.T_bound), dlo.ratio(TS, b.TS, b.TS_bound),
            dlo.ratio(TWT, b.TWT, b.TWT_bound))


@pytest.mark.parametrize("storage", dbo.STORAGES)
def test_the_replay_keeps_the_bounds_in_three_orders(storage):
    worst = 0.
    for n, P in NEG_CASES + ((5, 9), (1664, 9), (8193, 9)):
        b = dbo.gauss_batch(n, P, 2, storage)
        for order in dbo.ORDERS:
            r = _ratios(b, *dbo.replay_dot(b.Xt, b.V, b.OM, storage, order))
            g = dlo.ratio(dbo.replay_tdot(b.Xt, b.W, storage, order), b.G,
                          b.G_bound)
            assert max(r) <= 1. and g <= 1., (n, P, order, r, g)
            worst = max(worst, g, *r)
    print("float64 replays: at most %.1e of a bound" % worst)
    assert worst <= .5


@pytest.mark.parametrize("storage", dbo.STORAGES)
def test_a_wrong_replay_breaks_the_bounds(storage):
    """One row dropped, one slot of one part dropped, one unit's columns in
    another unit's place, one chain's rowscale skipped: each leaves its
    bound, and the untouched chain / product stays inside."""
    for n, P in NEG_CASES:
        b = dbo.gauss_batch(n, P, 2, storage)
        U = dbo.unit(storage)
        g = dbo.tdot_geometry(n, P, storage, 2)
        h = dbo.dot_geometry(n, P, storage, 2)

        def tdot(**kw):
            return dlo.ratio(dbo.replay_tdot(b.Xt, b.W, storage, **kw), b.G,
                             b.G_bound)

        def dot(**kw):
            return _ratios(b, *dbo.replay_dot(b.Xt, b.V, b.OM, storage, **kw))
        assert tdot() <= 1. and max(dot()) <= 1.
        assert tdot(drop_row=n - 1) > 1.
        assert tdot(drop_slot=(g.last_part, g.n_slot[g.last_part] - 1)) > 1.
        assert tdot(drop_slot=(0, 0)) > 1.
        if g.ld >= 2 * U:
            assert tdot(swap_units=(0, 1)) > 1.
        t, ts, twt = dot(drop_row=P - 1)
        assert t > 1. and ts > 1. and twt > 1.
        q = max(k for k in range(4) if h.n_slot[k])
        t, ts, twt = dot(drop_slot=(q, h.n_slot[q] - 1))
        assert t > 1. and ts > 1. and twt > 1.
        t, ts, twt = dot(swap_units=(0, 1))
        assert t > 1. and ts > 1.
        t, ts, twt = dot(skip_rowscale=1)
        assert t <= 1. and ts > 1. and twt > 1.
        # ... in chain 1 only
        T, TS, TWT = dbo.replay_dot(b.Xt, b.V, b.OM, storage, skip_rowscale=1)
        assert dlo.ratio(TS[0], b.TS[0], b.TS_bound[0]) <= 1.
        assert dlo.ratio(TWT[:1], b.TWT[:1], b.TWT_bound[:1]) <= 1.


def test_gauss_cases_are_within_the_cap_and_reach_every_table():
    cases = dbo.gauss_cases()
    assert all(n * dlo.ld_of(P) <= dlo.GAUSS_MAX_ENTRIES for n, P in cases)
    assert set(cases) == set(dbo.all_cases()) - {(dbo.TDOT_COL_N, 1),
                                                 (dbo.DOT_CONTR_N, 1)}
    assert (dbo.TDOT_COL_N, 8) in cases and max(cases) == (81921, 9)
