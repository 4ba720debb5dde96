"""Host statements of what the dense design (csrc/dense.hip) stores and
computes, the rounding bounds its float64 products must keep, and the edge
cases that the CPU tests (test_dense_ld_oracle.py) and the GPU tests
(test_hip_dense_edges.py) share.  Plain NumPy; products in long double (80-bit,
eps 1.08e-19) through NumPy's generic loops, so nothing here shares a
summation order or a code path with the device kernels or with BLAS.

The bounds.  A sum of k floating-point numbers, added in ANY order (a tree, a
chain, slabs added afterwards), is off by at most gamma_{k-1} sum|terms| with
gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability, 4.2);
a product in front of each term adds one rounding, gamma_k, and none when it
is fused into the addition.  1 / (1 - k u) and the second-order terms of a
product of two such sums stay below the slack that each count carries:
  dot, row i     : ld terms (the padding's zeros included)        ld + 2
  Tdot, column j : a chunk of at most n rows, then 64 slabs       n + 66
  operator, col j: t_i within gamma_ld, omega_i t_i and + addend_i one
                   rounding each, at most n rows in a workgroup's range, 256
                   slabs                                          ld + n + 300
each times u times the same product formed with absolute values.

The integer cases need no bound: every entry is an integer that f32 storage
holds exactly, and the sum of the absolute values of all terms of a result is
below 2^53, so every partial sum in every order (with or without FMA) is an
integer that float64 holds exactly and the device must return the int64
result bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
U = 2. ** -53

# ---- kernel geometry (test_dense_ld_oracle.py compares these with the text
# of csrc/dense.hip, api.hip and common.hpp) ----------------------------------
FUSED_WGS = 256            # workgroups of the single-pass operator kernels
FUSED_THREADS = 1024       # threads of each
FUSED_RB = 2               # rows per block of a workgroup's row range
ROW_CHUNKS = 64            # DENSE_ROW_CHUNKS: slabs of the Tdot
SINGLE_CHUNK_BELOW = 256   # rows below which the Tdot has one chunk
FUSED_MIN_N = 4096         # the single pass applies for n >= this ...
FUSED_MAX_LD = 8192        # ... and ld <= this
RING_MIN_ROWS = 64         # f32: ring kernel from this many rows per workgroup
RING_LDS_LIMIT = 160 * 1024
DOT_MAX_BLOCKS = 1024      # blocks of the dot ...
DOT_WAVES = 4              # ... of this many waves, one row per wave and trip
INGEST_THREADS = 4096 * 256


def ld_of(P):
    """Padded row length: P rounded up to 8."""
    return (P + 7) // 8 * 8


def fused_ring_lds(KQ, RB, D, rows_per_wg):
    """Bytes of LDS of dense_fused_ring_kernel<KQ, RB, D>."""
    return D * RB * KQ * 1024 * 16 + 8 * 2 * RB * 16 + 2 * 8 * (rows_per_wg + 8)


def rows_per_wg(n):
    return -(-n // FUSED_WGS)


def wg_rows(n):
    """(rows per workgroup, the first workgroup without rows [FUSED_WGS: none],
    rows of the last workgroup that has some)."""
    r = rows_per_wg(n)
    first_empty = -(-n // r)
    return r, first_empty, n - (first_empty - 1) * r


def chunk_rows(n):
    """(chunks, rows per chunk, the first chunk without rows, rows of the last
    chunk that has some) of the Tdot."""
    chunks = 1 if n < SINGLE_CHUNK_BELOW else ROW_CHUNKS
    r = -(-n // chunks)
    first_empty = -(-n // r)
    return chunks, r, first_empty, n - (first_empty - 1) * r


def operator_kernel(n, P, storage):
    """Which kernel gram_matvec runs by default: 'two' (dot, then Tdot),
    'register' or 'ring'."""
    if n < FUSED_MIN_N or ld_of(P) > FUSED_MAX_LD:
        return 'two'
    r = rows_per_wg(n)
    if (storage == 'float32' and r >= RING_MIN_ROWS
            and fused_ring_lds(2, 2, 2, r) <= RING_LDS_LIMIT):
        return 'ring'
    return 'register'


# ---- what the ingest kernel stores ------------------------------------------
def column_offset(X, in_dtype):
    """The centring offsets as HipDenseDesignMatrix forms them: column means
    of the array in its input type, accumulated in float64."""
    X = np.ascontiguousarray(np.asarray(X).astype(in_dtype))
    return np.mean(X, axis=0, dtype=np.float64)


def stored(X, in_dtype, storage, centred, intercept):
    """dense_ingest_kernel on the host: X~ (n x P, float64 values) as the
    device holds it.  Each entry is (double)src - offset in float64, then
    rounded to the storage type; the intercept column holds ones."""
    src = np.asarray(X).astype(in_dtype).astype(np.float64)
    if centred:
        src = src - column_offset(X, in_dtype)[None, :]
    if intercept:
        src = np.hstack((np.ones((src.shape[0], 1)), src))
    return np.ascontiguousarray(src.astype(storage).astype(np.float64))


# ---- long-double products ---------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=LD)


def dot_ld(Xt, v):
    return _ld(Xt) @ _ld(v)


def tdot_ld(Xt, w):
    return _ld(w) @ _ld(Xt)


def op_ld(Xt, omega, v, addend=None):
    """Xt^T (omega .* (Xt v) + addend)."""
    X = _ld(Xt)
    s = _ld(omega) * (X @ _ld(v))
    if addend is not None:
        s = s + _ld(addend)
    return s @ X


# ---- the bounds (long double) -----------------------------------------------
def dot_bound(Xt, v):
    P = Xt.shape[1]
    return LD(ld_of(P) + 2) * LD(U) * (np.abs(_ld(Xt)) @ np.abs(_ld(v)))


def tdot_bound(Xt, w):
    n = Xt.shape[0]
    return LD(n + 66) * LD(U) * (np.abs(_ld(w)) @ np.abs(_ld(Xt)))


def op_bound(Xt, omega, v, addend=None):
    n, P = Xt.shape
    A = np.abs(_ld(Xt))
    s = np.abs(_ld(omega)) * (A @ np.abs(_ld(v)))
    if addend is not None:
        s = s + np.abs(_ld(addend))
    return LD(ld_of(P) + n + 300) * LD(U) * (s @ A)


def ratio(out, ref, bound):
    """max_j |out_j - ref_j| / bound_j (0 / 0 counts as 0), in long double."""
    err = np.abs(_ld(out) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, LD(0), err / bound)
    return float(r.max())


# ---- Gaussian cases ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauss_case(n, P):
    """Predictors X (n x (P - 1): N(0, 1) plus a per-column shift N(0, 3^2),
    so that centring has something to remove), v[P], w[n], omega[n] > 0;
    meant for a centred design with intercept."""
    rng = np.random.default_rng([77, n, P])
    X = rng.normal(size=(n, P - 1)) + 3. * rng.normal(size=P - 1)
    c = SimpleNamespace(X=X, v=rng.normal(size=P), w=rng.normal(size=n),
                        omega=rng.gamma(2., .5, n), addend=rng.normal(size=n))
    for a in vars(c).values():
        a.setflags(write=False)
    return c


# ---- integer cases ----------------------------------------------------------
def int_products(Xi, v, w, omega, addend):
    """int64 results of an integer case (Xi: int8):
    t = Xi v, g = Xi^T w, op = Xi^T (omega .* t), op_add = Xi^T (omega .* t +
    addend), and `abs_max`, the largest sum of absolute values of the terms
    of any of these results' components."""
    n, P = Xi.shape
    v, w, omega, addend = (np.asarray(a, dtype=np.int64)
                           for a in (v, w, omega, addend))
    A = np.abs(Xi)

    def right(M, x):     # M x; einsum widens the int8 entries as it goes
        return np.einsum('ij,j->i', M, x, dtype=np.int64)

    def left(x, M):      # M^T x
        return np.einsum('i,ij->j', x, M, dtype=np.int64)
    t, ta = right(Xi, v), right(A, np.abs(v))
    g, ga = left(w, Xi), left(np.abs(w), A)
    op, op_add = left(omega * t, Xi), left(omega * t + addend, Xi)
    opa = left(omega * ta + np.abs(addend), A)
    abs_max = int(max(ta.max(), ga.max(), opa.max()))
    return SimpleNamespace(t=t, g=g, op=op, op_add=op_add, abs_max=abs_max)


def int_case(n, P, intercept=None, amp=8):
    """An integer case: Xi (n x P int8, entries in [-amp, amp], column 0 ones
    with an intercept), v[P], w[n], addend[n] in [-amp, amp], omega[n] in
    [1, 4], their int64 products, and X, the float32 predictors to build the
    design from (centring off).  The 2^53 condition is asserted here, on the
    inputs alone.  intercept None: on for odd P > 1."""
    if intercept is None:
        intercept = P > 1 and P % 2 == 1
    rng = np.random.default_rng([78, n, P, amp])
    Xi = rng.integers(-amp, amp + 1, size=(n, P), dtype=np.int8)
    if intercept:
        Xi[:, 0] = 1
    v = rng.integers(-amp, amp + 1, size=P)
    w = rng.integers(-amp, amp + 1, size=n)
    omega = rng.integers(1, 5, size=n)
    addend = rng.integers(-amp, amp + 1, size=n)
    c = int_products(Xi, v, w, omega, addend)
    assert c.abs_max < 2 ** 53, (n, P, c.abs_max)
    c.Xi, c.intercept = Xi, bool(intercept)
    c.X = np.ascontiguousarray(Xi[:, 1:] if intercept else Xi,
                               dtype=np.float32)
    c.v, c.w, c.omega, c.addend = (a.astype(np.float64)
                                   for a in (v, w, omega, addend))
    return c


# ---- the edge lists (derived from the geometry above) -----------------------
# dot / Tdot.  n: below, at and above a wave's share of rows; 255 / 256 / 257
# around the single chunk (257: 5 rows per chunk, chunk 51 has 2, 52-63 none);
# 321: 6 rows per chunk and an odd 3-row tail chunk; 4097: one row past the
# dot's single grid pass of 1024 blocks x 4 waves.
DOT_N = (1, 2, 3, 4, 5, 255, 256, 257, 321, 4097)
# P: ld 8 (two live lanes) for 1, 7, 8; 16; 256 and 264; 1024 (exactly one
# 4x-unrolled trip of the dot, one full Tdot column block), 1032 (two live
# threads in the second block); 2056.
DOT_P = (1, 7, 8, 9, 256, 257, 1024, 1025, 2049)
GAUSS_N = (3, 257, 4097)
GAUSS_P = (7, 257, 1025)

# the single pass, rows (at P = 9, ld 16)
OP_ROW_P = 9
OP_ROW_N = (4096, 4097, 4098, 16128, 16129, 16400)
# ring <-> register at the LDS limit (p = 7 with intercept: ld 8)
LDS_P = 8
LDS_N = (514048, 514049)
# the single pass, columns
OP_COL_N = (4097, 16129)
OP_COL_P = (2, 4089, 4096, 4097, 6145, 8185, 8192, 8193)
THRESHOLD_N = (4095, 4096)
GAUSS_MAX_ENTRIES = 10 ** 7      # n ld of a Gaussian operator case


def op_gauss_cases():
    """(n, P) of the operator's Gaussian cases: those of the row and column
    edges with n ld <= GAUSS_MAX_ENTRIES."""
    cases = [(n, OP_ROW_P) for n in OP_ROW_N]
    cases += [(n, P) for n in OP_COL_N for P in OP_COL_P]
    return [(n, P) for n, P in cases if n * ld_of(P) <= GAUSS_MAX_ENTRIES]


# one CG draw with a warm start: (n, p predictors, storage)
CG_CASES = ((4098, 9, 'float32'), (16129, 40, 'float32'),
            (4097, 4097, 'float32'), (4097, 4099, 'float64'))
# forced ring (BBX_DENSE_FUSED_RING=22) at edges: (n, p predictors, storage)
RING_CASES = ((4097, 8, 'float32'), (4098, 4100, 'float32'),
              (4097, 4095, 'float64'), (4098, 8190, 'float64'))
