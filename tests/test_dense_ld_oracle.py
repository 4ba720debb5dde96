"""CPU: the host side of the dense-edge tests (dense_ld_oracle.py) checked on
its own -- the ingest statement against a per-entry one, the long-double
products against exact arithmetic, the derived bounds against float64 sums in
three orders (and against a sum with one term missing), the 2^53 condition of
every integer case, and the kernel geometry the edge lists are derived from
against the text of the sources."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import dense_ld_oracle as dlo
from conftest import ROOT

CSRC = os.path.join(ROOT, "bayes-bridge_amd", "csrc")


# ---- stored() ---------------------------------------------------------------
@pytest.mark.parametrize("in_dtype", ['float32', 'float64'])
@pytest.mark.parametrize("storage", ['float32', 'float64'])
@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("intercept", [False, True])
def test_stored_is_the_per_entry_statement(in_dtype, storage, centred,
                                           intercept):
    rng = np.random.default_rng(5)
    X = rng.normal(size=(5, 3)) * 1e3 + rng.normal(size=3)
    got = dlo.stored(X, in_dtype, storage, centred, intercept)
    tin = np.dtype(in_dtype).type
    tout = np.dtype(storage).type
    src = [[tin(X[i, j]) for j in range(3)] for i in range(5)]
    offset = []
    for j in range(3):      # row after row, in float64, then one division
        s = np.float64(0.)
        for i in range(5):
            s = s + np.float64(src[i][j])
        offset.append(s / np.float64(5))
    assert got.shape == (5, 3 + intercept) and got.dtype == np.float64
    for i in range(5):
        for c in range(3 + intercept):
            if intercept and c == 0:
                want = 1.
            else:
                j = c - intercept
                val = np.float64(src[i][j])
                if centred:
                    val = val - offset[j]
                want = np.float64(tout(val))
            assert got[i, c] == want, (i, c)
    if centred:
        assert np.array_equal(dlo.column_offset(X, in_dtype), offset)
    if in_dtype == storage == 'float64' and not centred:
        assert np.array_equal(got[:, intercept:], X)
    if storage == 'float32':
        assert np.array_equal(got, got.astype(np.float32))


# ---- long double against exact arithmetic -----------------------------------
def _exact(c):
    """Python-int products of an integer case."""
    X = [[int(a) for a in row] for row in c.Xi]
    v, w, om, ad = ([int(a) for a in x] for x in (c.v, c.w, c.omega, c.addend))
    n, P = c.Xi.shape
    t = [sum(X[i][j] * v[j] for j in range(P)) for i in range(n)]
    g = [sum(X[i][j] * w[i] for i in range(n)) for j in range(P)]
    op = [sum(X[i][j] * om[i] * t[i] for i in range(n)) for j in range(P)]
    opa = [sum(X[i][j] * (om[i] * t[i] + ad[i]) for i in range(n))
           for j in range(P)]
    return t, g, op, opa


@pytest.mark.parametrize("n,P", [(1, 1), (5, 9), (67, 17), (257, 8)])
def test_long_double_and_int64_products_are_exact_on_integer_cases(n, P):
    c = dlo.int_case(n, P)
    t, g, op, opa = _exact(c)
    Xt = c.Xi.astype(np.float64)
    assert c.intercept == (P % 2 == 1 and P > 1)
    if c.intercept:
        assert np.all(c.Xi[:, 0] == 1) and c.X.shape == (n, P - 1)
    assert [int(a) for a in c.t] == t and [int(a) for a in c.g] == g
    assert [int(a) for a in c.op] == op and [int(a) for a in c.op_add] == opa
    for got, want in ((dlo.dot_ld(Xt, c.v), t), (dlo.tdot_ld(Xt, c.w), g),
                      (dlo.op_ld(Xt, c.omega, c.v), op),
                      (dlo.op_ld(Xt, c.omega, c.v, c.addend), opa)):
        assert got.dtype == dlo.LD
        assert [int(a) for a in got] == want


def test_long_double_products_against_fractions():
    """Non-integers: within a few long-double roundings of the exact rational
    result (which a float64 sum is not)."""
    c = dlo.gauss_case(3, 7)
    Xt = dlo.stored(c.X, 'float64', 'float64', True, True)
    F = [[Fraction(float(a)) for a in row] for row in Xt]
    v = [Fraction(float(a)) for a in c.v]
    om = [Fraction(float(a)) for a in c.omega]
    ad = [Fraction(float(a)) for a in c.addend]
    t = [sum(F[i][j] * v[j] for j in range(7)) for i in range(3)]
    op = [sum(F[i][j] * (om[i] * t[i] + ad[i]) for i in range(3))
          for j in range(7)]
    absop = [sum(abs(F[i][j]) * (om[i] * sum(abs(F[i][k] * v[k])
                                              for k in range(7)) + abs(ad[i]))
                 for i in range(3)) for j in range(7)]
    eps = Fraction(float(np.finfo(dlo.LD).eps))
    got = dlo.op_ld(Xt, c.omega, c.v, c.addend)
    for j in range(7):
        hi, lo = np.float64(got[j]), np.float64(got[j] - np.float64(got[j]))
        err = abs(Fraction(float(hi)) + Fraction(float(lo)) - op[j])
        assert err <= 32 * eps * absop[j]
    got_t = dlo.dot_ld(Xt, c.v)
    for i in range(3):
        hi = np.float64(got_t[i])
        lo = np.float64(got_t[i] - hi)
        err = abs(Fraction(float(hi)) + Fraction(float(lo)) - t[i])
        assert err <= 16 * eps * sum(abs(F[i][k] * v[k]) for k in range(7))


# ---- the bounds against float64 sums in three orders ------------------------
def _sum64(T, axis, order):
    """float64 sum of the terms T along `axis`: 'forward' and 'reversed' are
    strict chains, 'chunks' adds 64 consecutive parts as chains, then those."""
    T = np.moveaxis(T, axis, 0)
    if order == 'reversed':
        T = T[::-1]
    if order == 'chunks':
        parts = np.array_split(T, 64, axis=0)
        T = np.stack([np.cumsum(p, axis=0)[-1] if len(p) else
                      np.zeros(T.shape[1:]) for p in parts])
    return np.cumsum(T, axis=0)[-1]


ORDERS = ('forward', 'reversed', 'chunks')


@pytest.mark.parametrize("storage", ['float32', 'float64'])
def test_float64_sums_in_three_orders_keep_the_dot_and_tdot_bounds(storage):
    worst = {}
    for n in dlo.GAUSS_N:
        for P in dlo.GAUSS_P:
            c = dlo.gauss_case(n, P)
            Xt = dlo.stored(c.X, 'float64', storage, True, True)
            rd, bd = dlo.dot_ld(Xt, c.v), dlo.dot_bound(Xt, c.v)
            rt, bt = dlo.tdot_ld(Xt, c.w), dlo.tdot_bound(Xt, c.w)
            for order in ORDERS:
                d = dlo.ratio(_sum64(Xt * c.v[None, :], 1, order), rd, bd)
                t = dlo.ratio(_sum64(Xt * c.w[:, None], 0, order), rt, bt)
                worst[n, P, order] = (d, t)
                assert d <= 1. and t <= 1., (n, P, order, d, t)
    print("forward, %d x %d: %.1e of the dot bound, %.1e of the Tdot bound"
          % ((4097, 1025) + worst[4097, 1025, 'forward']))
    # a correct sum is far inside: what the bounds leave room for is the
    # worst case of ld or n roundings that all point the same way
    assert max(max(v) for v in worst.values()) <= .5


@pytest.mark.parametrize("storage", ['float32', 'float64'])
def test_float64_sums_in_three_orders_keep_the_operator_bound(storage):
    worst = 0.
    for n, P in dlo.op_gauss_cases():
        c = dlo.gauss_case(n, P)
        Xt = dlo.stored(c.X, 'float64', storage, True, True)
        ref = dlo.op_ld(Xt, c.omega, c.v, c.addend)
        bound = dlo.op_bound(Xt, c.omega, c.v, c.addend)
        for order in ORDERS:
            t = _sum64(Xt * c.v[None, :], 1, order)
            s = c.omega * t + c.addend
            r = dlo.ratio(_sum64(Xt * s[:, None], 0, order), ref, bound)
            assert r <= 1., (n, P, order, r)
            worst = max(worst, r)
    print("operator: at most %.1e of the bound" % worst)
    assert worst <= .5


def test_operator_gauss_cases_are_the_small_ones():
    cases = dlo.op_gauss_cases()
    assert all(n * dlo.ld_of(P) <= 10 ** 7 for n, P in cases)
    assert set((n, dlo.OP_ROW_P) for n in dlo.OP_ROW_N) <= set(cases)
    assert (4097, 2) in cases and (16129, 2) in cases
    assert (4097, 4089) not in cases


@pytest.mark.parametrize("storage", ['float32', 'float64'])
def test_a_single_missing_term_breaks_the_bounds(storage):
    """A kernel that drops one term -- a lane masked by an off-by-one, the
    tail row of a chunk -- is caught even where the term is the smallest of
    its sum: in these cases the smallest term of EVERY row (column) is above
    the bound of that row (column) -- by 1e2 at the least (a column of 4097
    terms), and for the typical row of every case by more than 1e6."""
    for n in dlo.GAUSS_N:
        for P in dlo.GAUSS_P:
            c = dlo.gauss_case(n, P)
            Xt = dlo.stored(c.X, 'float64', storage, True, True)
            for what, T, ref, bound in (
                    ('dot', dlo._ld(Xt) * dlo._ld(c.v)[None, :],
                     dlo.dot_ld(Xt, c.v), dlo.dot_bound(Xt, c.v)),
                    ('Tdot', (dlo._ld(Xt) * dlo._ld(c.w)[:, None]).T,
                     dlo.tdot_ld(Xt, c.w), dlo.tdot_bound(Xt, c.w))):
                k = np.abs(T).argmin(axis=1)
                small = T[np.arange(len(T)), k]
                short = np.asarray(ref - small, dtype=np.float64)
                assert np.all(np.abs(dlo._ld(short) - ref) > bound), (n, P)
                margin = np.abs(small) / bound
                assert margin.min() > 1., (n, P, float(margin.min()))
                if what == 'dot':
                    assert np.median(margin) > 1e6, (n, P)


# ---- the integer cases of the GPU module ------------------------------------
def test_every_small_integer_case_meets_the_2_53_condition():
    """int_case asserts it; here for every case of the dot / Tdot cross and of
    the operator's row edges (the large column edges assert it when the GPU
    module builds them: the worst of those is bounded below)."""
    worst = 0
    for n in dlo.DOT_N:
        for P in dlo.DOT_P:
            worst = max(worst, dlo.int_case(n, P).abs_max)
    for n in dlo.OP_ROW_N + dlo.THRESHOLD_N:
        worst = max(worst, dlo.int_case(n, dlo.OP_ROW_P).abs_max)
    assert worst < 2 ** 53
    # entries <= 8, omega <= 4: sum |terms| of an operator component is at
    # most n * 8 * (4 * ld * 64 + 8), for every case of the lists
    for n, P in ([(n, P) for n in dlo.OP_COL_N for P in dlo.OP_COL_P]
                 + [(n, dlo.LDS_P) for n in dlo.LDS_N]):
        assert n * 8 * (4 * dlo.ld_of(P) * 64 + 8) < 2 ** 53


# ---- the geometry, from the sources -----------------------------------------
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) >= 1, pattern
    assert len(set(found)) == 1, (pattern, found)
    return found[0]


def test_geometry_constants_are_those_of_the_sources():
    dense = _text("dense.hip")
    assert int(_one(r"constexpr int DENSE_ROW_CHUNKS = (\d+);", dense)) \
        == dlo.ROW_CHUNKS
    k = int(_one(r"if \(h->n < (\d+) \* DENSE_ROW_CHUNKS\) "
                 r"h->dense_chunks = 1;", dense))
    assert k * dlo.ROW_CHUNKS == dlo.SINGLE_CHUNK_BELOW
    assert int(_one(r"const int64_t ld_max = (\d+);", dense)) \
        == dlo.FUSED_MAX_LD
    assert int(_one(r"h->dense_ld > ld_max \|\| h->n < (\d+)\)", dense)) \
        == dlo.FUSED_MIN_N
    assert int(_one(r"ring_env > 0 \|\| rows_per_wg >= (\d+)\)", dense)) \
        == dlo.RING_MIN_ROWS
    assert int(_one(r"const int wgs = (\d+);", dense)) == dlo.FUSED_WGS
    assert _one(r"rows_per_wg = \(h->n \+ wgs - 1\) / wgs;", dense)
    assert int(_one(r"fused_ring_lds\(2, 2, 2, rows_per_wg\) <= (\d+) \* 1024",
                    dense)) * 1024 == dlo.RING_LDS_LIMIT
    # the default f32 launches: RB = 2 rows per block, ring depth 2
    assert set(re.findall(r"BBX_RING_LAUNCH\((\d), (\d), (\d)\);", dense)) \
        == {('1', str(dlo.FUSED_RB), '2'), ('2', str(dlo.FUSED_RB), '2')}
    assert set(re.findall(r"BBX_FUSED_LAUNCH\(float, (\d), (\d)\);", dense)) \
        == {('1', str(dlo.FUSED_RB)), ('2', str(dlo.FUSED_RB))}
    assert _one(r"constexpr int RB = (\d);", dense) == str(dlo.FUSED_RB)
    # ... of FUSED_THREADS threads, one workgroup per slab
    launches = re.findall(r"dim3\(wgs\),\s*\\?\s*dim3\((\d+)\)", dense)
    assert len(launches) == 4 and set(launches) == {str(dlo.FUSED_THREADS)}
    # the ring's LDS: the formula, as text
    flat = re.sub(r"\s+", " ", dense)
    assert ("static size_t fused_ring_lds(int KQ, int RB, int D, int64_t "
            "rows_per_wg) { return (size_t)D * RB * KQ * 1024 * 16 + "
            "sizeof(double) * 2 * RB * 16 + 2 * sizeof(double) * "
            "(size_t)(rows_per_wg + 8); }") in flat
    # the dot: (n + 3) / 4 blocks of 4 waves, capped
    assert _one(r"int64_t nb = \(h->n \+ 3\) / (\d+);", dense) \
        == str(dlo.DOT_WAVES)
    m = re.search(r"if \(nb > (\d+)\) nb = (\d+);   // 4 rows in flight", dense)
    assert m and int(m.group(1)) == int(m.group(2)) == dlo.DOT_MAX_BLOCKS
    assert 256 // 64 == dlo.DOT_WAVES
    assert _one(r"dense_dot_kernel<float>, dim3\(\(unsigned\)nb\), "
                r"dim3\((\d+)\)", dense) == "256"
    # the ingest: a fixed grid, grid-stride beyond it
    m = re.search(r"const dim3 grid\((\d+)\), block\((\d+)\);", dense)
    assert int(m.group(1)) * int(m.group(2)) == dlo.INGEST_THREADS
    # padded row length
    assert _one(r"h->dense_ld = \(h->P \+ 7\) / 8 \* 8;", dense)
    assert dlo.ld_of(1) == 8 and dlo.ld_of(8) == 8 and dlo.ld_of(9) == 16
    # one slab per workgroup = one partial per workgroup
    assert int(_one(r"constexpr int NPART = (\d+);", _text("common.hpp"))) \
        == dlo.FUSED_WGS
    # gram_matvec: the single pass where it applies, else dot and Tdot
    api = re.sub(r"\s+", " ", _text("api.hip"))
    assert ("const int st = launch_operator_dense_fused(h, d_v, d_obs_prec, "
            "ep, d_out); if (st <= 0) return st;") in api
    assert "if (!dense_fused_applies(h)) return 1;" in dense


def test_row_edges_have_the_properties_they_are_listed_for():
    wg = dlo.wg_rows
    assert wg(4096) == (16, 256, 16)               # every workgroup full
    assert wg(4097) == (17, 241, 17)               # odd rows, 241-255 empty
    assert 17 % dlo.FUSED_RB == 1
    assert wg(4098) == (17, 242, 1)                # a single-row workgroup
    assert wg(16128) == (63, 256, 63)
    assert wg(16129) == (64, 253, 1)               # 252 has one row: n_blk 1
    assert wg(16400) == (65, 253, 20)
    assert 65 % dlo.FUSED_RB == 1                  # last block half clamped
    kern = dlo.operator_kernel
    for n in (4096, 4097, 4098, 16128):
        assert kern(n, 9, 'float32') == kern(n, 9, 'float64') == 'register'
    for n in (16129, 16400):
        assert kern(n, 9, 'float32') == 'ring'
        assert kern(n, 9, 'float64') == 'register'
    assert kern(4095, 9, 'float32') == 'two'
    assert dlo.rows_per_wg(16128) == dlo.RING_MIN_ROWS - 1
    # the LDS limit
    assert dlo.rows_per_wg(514048) == 2008
    assert dlo.fused_ring_lds(2, 2, 2, 2008) == dlo.RING_LDS_LIMIT
    assert kern(514048, 8, 'float32') == 'ring'
    assert dlo.rows_per_wg(514049) == 2009
    assert kern(514049, 8, 'float32') == 'register'
    assert dlo.ld_of(dlo.LDS_P) == 8
    assert 514049 * 8 > dlo.INGEST_THREADS         # the ingest's second trip
    assert 16129 * dlo.ld_of(4089) > dlo.INGEST_THREADS


def test_column_edges_have_the_properties_they_are_listed_for():
    def live(P, per_thread):
        """Live threads of each group of a row of ld(P) / per_thread units."""
        units = dlo.ld_of(P) // per_thread
        return [min(dlo.FUSED_THREADS, units - k)
                for k in range(0, units, dlo.FUSED_THREADS)]
    assert live(2, 4) == [2] and live(2, 2) == [4]
    for P in (4089, 4096):                         # KQ = 1, G = 2 exactly full
        assert live(P, 4) == [1024] and live(P, 2) == [1024, 1024]
    assert live(4097, 4) == [1024, 2]              # second f32 group: 2
    assert live(4097, 2) == [1024, 1024, 4]        # third f64 group: 4
    assert live(6145, 2) == [1024, 1024, 1024, 4]  # fourth f64 group: 4
    assert live(6145, 4) == [1024, 514]
    for P in (8185, 8192):
        assert live(P, 4) == [1024, 1024] and live(P, 2) == 4 * [1024]
    for n in dlo.OP_COL_N:
        for P in dlo.OP_COL_P:
            want = 'two' if P == 8193 else (
                'ring' if n == 16129 else 'register')
            assert dlo.operator_kernel(n, P, 'float32') == want
    # the CG and forced-ring cases: two f32 groups, four f64 groups
    # (n, p predictors, storage; P = p + 1 with the intercept): rows of the
    # last workgroup that has some, padded row length
    wg = dlo.wg_rows
    assert [(wg(n)[2], dlo.ld_of(p + 1), s) for n, p, s in dlo.CG_CASES] == [
        (1, 16, 'float32'), (1, 48, 'float32'), (17, 4104, 'float32'),
        (17, 4104, 'float64')]
    assert [(wg(n)[2], dlo.ld_of(p + 1), s) for n, p, s in dlo.RING_CASES] == [
        (17, 16, 'float32'), (1, 4104, 'float32'), (17, 4096, 'float64'),
        (1, 8192, 'float64')]
    assert all(wg(n)[1] < dlo.FUSED_WGS for n, _, _ in dlo.RING_CASES)


def test_dot_and_tdot_edges_have_the_properties_they_are_listed_for():
    ch = dlo.chunk_rows
    assert ch(255) == (1, 255, 1, 255)
    assert ch(256) == (64, 4, 64, 4)
    assert ch(257) == (64, 5, 52, 2)               # chunk 51: 2 rows; 52+: none
    assert ch(321) == (64, 6, 54, 3)               # an odd 3-row tail chunk
    assert ch(4097) == (64, 65, 64, 2)
    assert dlo.DOT_MAX_BLOCKS * dlo.DOT_WAVES == 4096 < 4097
    quads = {P: dlo.ld_of(P) // 4 for P in dlo.DOT_P}
    assert quads[1] == quads[7] == quads[8] == 2   # two live lanes
    assert quads[1024] == 4 * 64                   # exactly one unrolled trip
    assert quads[1024] == 256                      # one full Tdot block
    assert quads[1025] == 256 + 2                  # two threads in the second
    assert quads[9] == 4 and quads[257] == 66 and quads[2049] == 514
