"""Host statements of the batched dense products (csrc/dense_batch.hip: the two
K-column products of a dense design on the f64 matrix cores): the geometry of
the kernels as functions of (n, P, storage, K), the condition their register
rings' read-ahead puts on the allocations, the edge cases derived from that
geometry, and the rounding bounds of the Gaussian cases.  Shared by the CPU
tests (test_dense_batch_oracle.py) and the GPU tests
(test_hip_dense_batch_edges.py); the long-double products, `stored`, `ratio`
and the integer design come from dense_ld_oracle.py.

The bounds.  As in dense_ld_oracle.py: a sum of k floating-point numbers added
in ANY order is off by at most gamma_{k-1} sum|terms|, a product rounded in
front of its addition adds one rounding.  How the matrix core orders and
rounds the four products and the accumulator of one v_mfma_f64_16x16x4_f64 is
not documented and has not been measured here.  THE ASSUMPTION: every addition
and every product inside the instruction is rounded no worse than an IEEE
operation (relative error <= u = 2^-53), in whatever order.  Under it the
any-order bound holds with these counts (k u sum|terms| each; the `+ 2` is the
slack for 1 / (1 - k u) and second-order terms):
  X V, row i      : ld contracted terms (the padding's zeros included: at
                    least the rows a wave quarter chains through its
                    accumulator, in any order within and across MFMAs), 1 for
                    a product rounded before its addition, 3 additions of the
                    four-wave fold                                  ld + 4 + 2
  X^T W, column j : n rows, 1 product rounding, 3 fold additions, 7 additions
                    of the eight chunk slabs                        n + 11 + 2
  scaled output   : rowscale_i * t_i, one more rounding             ld + 5 + 2
  <t, Omega t>    : term i is fma(w_i, t_i, .), w_i = fl(omega_i t_i): t_i
                    within B_i (the X V bound) twice, the rounding of w_i; then
                    at most n additions inside a lane, 2 shuffles, 4 waves and
                    256 partials on the host                       n + 262 + 2
None of this is tuned to what the device returns.

The integer cases need no bound (dense_ld_oracle.py): every partial sum in
every order is an integer below 2^53, <t, Omega t> included, so the device
must return the int64 results bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np

import dense_ld_oracle as dlo
from dense_ld_oracle import LD, _ld, ld_of

# ---- constants of csrc/dense_batch.hip and common.hpp -----------------------
# (test_dense_batch_oracle.py reads each from the source text)
WAVE = 64
DKD_WAVES = 4              # waves of a workgroup: quarters of the rows
DK_TDOT_CHUNKS = 8         # row chunks (slabs) of X^T W
DK_DOT_WGS = 256           # persistent workgroups of X V
DKT_D = 5                  # ring depth, one group of chains
DKT_D2 = 6                 # ... two groups, f32 storage
DKT_D2_F64 = 5             # ... two groups, f64 storage
DK_KS = 16                 # chains of one group (DENSE_BATCH_STRIDE)
DENSE_PAD_ROWS = 256       # zero rows behind X and behind its transposed copy
DENSE_BATCH_ROW_PAD = 320  # zero rows behind the batch's interleaved vectors
NPART = 256                # partials per chain
SLOT_ROWS = 4              # rows of a ring slot
XT_ROW_ROUND = 64          # the transposed copy holds ld rounded up to this
LDN_ROUND = 64             # ... and rows of n rounded up to this

STORAGES = ('float32', 'float64')
WIDTHS = (2, 4, 8, 16, 32)  # chains a batch may hold (bbx_batch_create_opts)
TEST_K = (2, 16, 32)


def _ceil(a, b):
    return -(-a // b)


def elems(storage):
    """E: elements of a lane's 16 bytes."""
    return 16 // np.dtype(storage).itemsize


def unit(storage):
    """U: columns of a unit (one load instruction: 4 rows x 16 lanes x E)."""
    return 16 * elems(storage)


def groups(K):
    """NG: groups of 16 chains."""
    return 1 if K <= DK_KS else 2


def stride(K):
    return DK_KS * groups(K)


def dkd_cw(NG, E):
    """CW: units per sweep (the accumulators have to fit 128 VGPRs)."""
    return 4 if NG * E <= 4 else 2


def cw(storage, K):
    return dkd_cw(groups(K), elems(storage))


def depth(storage, K):
    """D: slots of the register ring of one instantiation."""
    if groups(K) == 1:
        return DKT_D
    return DKT_D2_F64 if np.dtype(storage).itemsize == 8 else DKT_D2


def _parts(total, rows_per_part, n_part):
    """n_slot of each of n_part consecutive parts of rows_per_part rows."""
    out = []
    for q in range(n_part):
        lo = q * rows_per_part
        hi = min(total, lo + rows_per_part)
        out.append(_ceil(hi - lo, SLOT_ROWS) if hi > lo else 0)
    return out


def tdot_geometry(n, P, storage, K):
    """dense_tdot_kd_kernel: rows per wave, n_slot of each of the 32 row parts
    (chunk-major: part = 4 chunk + wave), rows of the last part that has some,
    the column blocks and the live (col < ld) columns of the last one."""
    parts = DK_TDOT_CHUNKS * DKD_WAVES
    rpw = SLOT_ROWS * _ceil(_ceil(n, parts), SLOT_ROWS)
    n_slot = _parts(n, rpw, parts)
    last = max(q for q in range(parts) if n_slot[q])
    block = unit(storage) * cw(storage, K)
    ld = ld_of(P)
    n_colblk = _ceil(ld, block)
    return SimpleNamespace(
        rows_per_wave=rpw, n_slot=n_slot, last_part=last,
        last_part_rows=n - last * rpw, block=block, n_colblk=n_colblk,
        last_block_cols=ld - (n_colblk - 1) * block, ld=ld)


def dot_geometry(n, P, storage, K):
    """dense_dot_kd_kernel: n_slot of the four wave quarters of the P
    contracted rows, the units of result rows, the units each workgroup owns
    and the set of sweep widths C that some workgroup runs."""
    rpw = SLOT_ROWS * _ceil(_ceil(P, DKD_WAVES), SLOT_ROWS)
    n_slot = _parts(P, rpw, DKD_WAVES)
    ldn = _ceil(n, LDN_ROUND) * LDN_ROUND
    U = unit(storage)
    n_unit = ldn // U
    base, extra = divmod(n_unit, DK_DOT_WGS)
    counts = [base + (b < extra) for b in range(DK_DOT_WGS)]
    CW = cw(storage, K)
    widths = set()
    for cnt in set(counts):
        if cnt >= CW:
            widths.add(CW)
        if cnt % CW:
            widths.add(cnt % CW)
    live = [max(0, min(U, n - u * U)) for u in range(n_unit)]
    return SimpleNamespace(rows_per_wave=rpw, n_slot=n_slot, ldn=ldn,
                           n_unit=n_unit, counts=counts, widths=widths,
                           unit_live_rows=live, quarter_rows=[
                               max(0, min(P, (q + 1) * rpw) - q * rpw)
                               for q in range(DKD_WAVES)])


# ---- the padding condition --------------------------------------------------
# Derived from the loop of dkd_sweep, not from a comment: the ring is primed
# with D slots, then ceil(n_slot / D) periods each retire and RE-ISSUE D
# slots, so a wave issues D + D ceil(n_slot / D) slots of 4 rows from its first
# row on (from row 0 when it owns none).  The last of them lies
# D + D ceil(s / D) - s <= 2 D - 1 slots past the wave's own s slots.  Every
# load of A is 4 rows x (units of the sweep) wide and carries no condition, a
# load of B is 4 rows x the whole stride: what is stated below is that all of
# them fall inside the ALLOCATIONS (dense.hip, ensure_dense_transpose_t,
# bbx_batch_create_opts), which is what keeps the kernel from faulting; that
# the rows are ZERO where it matters is what the products' tests show.
def issued_slots(n_slot, D):
    return D + D * _ceil(n_slot, D)


def rows_read_end(r_begin, n_slot, D):
    """One past the last row a wave's ring loads."""
    return (r_begin if n_slot > 0 else 0) + SLOT_ROWS * issued_slots(n_slot, D)


def assert_padding(n, P, storage, K):
    """The read-ahead of both products stays inside the allocations."""
    D = depth(storage, K)
    ld = ld_of(P)
    # X^T W: A = X, (n + DENSE_PAD_ROWS) x ld; a load spans a whole column
    # block, which may pass the end of its row into the following rows
    g = tdot_geometry(n, P, storage, K)
    for q, s in enumerate(g.n_slot):
        assert issued_slots(s, D) - s <= 2 * D - 1
        end = rows_read_end(q * g.rows_per_wave, s, D)
        last_elem = (end - 1) * ld + g.n_colblk * g.block
        assert last_elem <= (n + DENSE_PAD_ROWS) * ld, (n, P, storage, K, q)
        # B = w, (n + DENSE_BATCH_ROW_PAD) x stride
        assert end <= n + DENSE_BATCH_ROW_PAD, (n, P, storage, K, q)
    # X V: A = the transposed copy, (ld rounded to 64 + DENSE_PAD_ROWS) x ldn;
    # the units of a sweep are whole units of ldn
    h = dot_geometry(n, P, storage, K)
    assert h.n_unit * unit(storage) == h.ldn
    xt_rows = _ceil(ld, XT_ROW_ROUND) * XT_ROW_ROUND + DENSE_PAD_ROWS
    for q, s in enumerate(h.n_slot):
        end = rows_read_end(q * h.rows_per_wave, s, D)
        assert end <= xt_rows, (n, P, storage, K, q)
        # B = v, (ld + DENSE_BATCH_ROW_PAD + 2) x stride
        assert end <= ld + DENSE_BATCH_ROW_PAD + 2, (n, P, storage, K, q)


# ---- the case tables --------------------------------------------------------
DEPTHS = (5, 6)            # asserted against depth() by the CPU tests
RING_S = tuple(sorted({s for D in DEPTHS
                       for s in (D - 1, D, D + 1, 2 * D, 2 * D + 1)}))
EDGE_P = 9                 # ld 16

# X^T W, rows: n = 1 one live part of one slot (one row); 4: that slot full;
# 5: a part of one row behind it, then empty parts; 127: every part one slot,
# the last with 3 rows; 128: every part exactly one full slot; 129: rows per
# wave 8, a part with one row followed by empty parts
TDOT_ROW_N = (1, 4, 5, 127, 128, 129)
# X^T W, ring: every part exactly s slots, s around one and two ring periods
# of both depths; 128 D -+ 1: the last live slot holds 3 rows / 1 row
TDOT_RING_N = tuple(128 * s for s in RING_S) + tuple(
    128 * D + e for D in DEPTHS for e in (-1, 1))
# X^T W, columns (n = 129): ld 8; one unit exactly (32 / 64) and + 8; one
# column block (128 / 256) - 8, exactly, + 8
TDOT_COL_N = 129
TDOT_COL_P = (1, 8, 9, 32, 33, 64, 65, 120, 128, 129, 248, 256, 257)
# X V, contraction (n = 65: the last live unit holds one live row and at f64
# a further unit none): quarters of 0 rows, 1 row, 1 slot, 2 slots; every
# quarter exactly s slots; one row past D slots per quarter
DOT_CONTR_N = 65
DOT_CONTR_P = (1, 4, 5, 16, 17) + tuple(16 * s for s in RING_S) + tuple(
    16 * D + 1 for D in DEPTHS)
# X V, units (P = 9): 257 / 769 / 1281 units of f32 and 258 / 770 / 1282 of
# f64 over 256 workgroups: 2 and 1, 4 and 3, 4 + 2 and 4 + 1 units each
DOT_UNIT_N = (8193, 16385, 24577, 40961, 49153, 81921)
BIG_N = DOT_UNIT_N[-3:]    # K = 2 and 32 only


def all_cases():
    """(n, P) of every case, in table order, without repeats."""
    cases = [(n, EDGE_P) for n in TDOT_ROW_N + TDOT_RING_N]
    cases += [(TDOT_COL_N, P) for P in TDOT_COL_P]
    cases += [(DOT_CONTR_N, P) for P in DOT_CONTR_P]
    cases += [(n, EDGE_P) for n in DOT_UNIT_N]
    return list(dict.fromkeys(cases))


def case_widths(n):
    return (2, 32) if n in BIG_N else TEST_K


GAUSS_MAX_ENTRIES = dlo.GAUSS_MAX_ENTRIES


def gauss_cases():
    """The Gaussian subset: every case within the cap but P = 1 (a centred
    design with intercept has no predictor there; ld 8 is reached by P = 8)."""
    return [(n, P) for n, P in all_cases()
            if n * ld_of(P) <= GAUSS_MAX_ENTRIES and P > 1]


# ---- K-chain inputs ---------------------------------------------------------
@functools.lru_cache(maxsize=4)
def int_batch(n, P, K):
    """dlo.int_case(n, P) with K different integer vectors per side: V[K, P],
    W[K, n] in [-8, 8], OM[K, n] in [1, 4] (different per chain), and the
    int64 results T = V Xi^T, G = W Xi, TS = OM .* T, TWT_c = sum OM_c T_c^2.
    The 2^53 condition -- on sum |terms| of every component, <t, Omega t>
    included -- is asserted here, on the inputs alone."""
    c = dlo.int_case(n, P)
    rng = np.random.default_rng([79, n, P, K])
    V = rng.integers(-8, 9, size=(K, P))
    W = rng.integers(-8, 9, size=(K, n))
    OM = rng.integers(1, 5, size=(K, n))
    k = np.arange(K)
    for i in range(min(n, 3)):              # the chain's number in base 4
        OM[:, i] = 1 + (k // 4 ** i) % 4
    for j in range(min(P, 2)):              # ... and in base 17
        V[:, j] = (k // 17 ** j) % 17 - 8
    Xi = c.Xi.astype(np.int64)
    A = np.abs(Xi)
    T, G = V @ Xi.T, W @ Xi
    Ta, Ga = np.abs(V) @ A.T, np.abs(W) @ A
    TWT = (OM * T * T).sum(axis=1)
    abs_max = int(max((OM * Ta).max(), Ga.max(), (OM * Ta * Ta).sum(axis=1).max()))
    assert abs_max < 2 ** 53, (n, P, K, abs_max)
    # (as many different rowscales / vectors as the shape has room for)
    assert len({row.tobytes() for row in OM}) >= min(K, 4 ** min(n, 3))
    assert len({row.tobytes() for row in V}) >= min(K, 17 ** min(P, 2))
    f = np.float64
    return SimpleNamespace(case=c, Xi=c.Xi, intercept=c.intercept, X=c.X,
                           V=V.astype(f), W=W.astype(f), OM=OM.astype(f),
                           T=T.astype(f), G=G.astype(f),
                           TS=(OM * T).astype(f), TWT=TWT.astype(f),
                           abs_max=abs_max)


@functools.lru_cache(maxsize=4)
def gauss_batch(n, P, K, storage):
    """dlo.gauss_case(n, P)'s predictors on a centred design with intercept,
    K Gaussian vectors per side and Gamma rowscales, with the long-double
    products of stored(...) and their bounds, per component."""
    c = dlo.gauss_case(n, P)
    rng = np.random.default_rng([80, n, P, K])
    V, W = rng.normal(size=(K, P)), rng.normal(size=(K, n))
    OM = rng.gamma(2., .5, size=(K, n))
    Xt = dlo.stored(c.X, 'float64', storage, True, True)
    XL, AL = _ld(Xt), np.abs(_ld(Xt))
    VL, WL, OL = _ld(V), _ld(W), _ld(OM)
    u = LD(dlo.U)
    ld = ld_of(P)
    T, Ta = VL @ XL.T, np.abs(VL) @ AL.T
    G, Ga = WL @ XL, np.abs(WL) @ AL
    B = LD(ld + 6) * u * Ta                       # X V
    TWT = (OL * T * T).sum(axis=1)
    twt_b = ((OL * (2 * np.abs(T) * B + B * B)).sum(axis=1) * (1 + 4 * u)
             + LD(n + 264) * u * (OL * (np.abs(T) + B) ** 2).sum(axis=1))
    return SimpleNamespace(
        X=c.X, Xt=Xt, V=V, W=W, OM=OM, T=T, T_bound=B, G=G,
        G_bound=LD(n + 13) * u * Ga, TS=OL * T,
        TS_bound=LD(ld + 7) * u * OL * Ta, TWT=TWT, TWT_bound=twt_b)


# ---- a float64 replay of the kernels' sums (the CPU negative control) -------
ORDERS = ('forward', 'reversed', 'pairwise')


def _sum64(T, order):
    """float64 sum of T along axis 0 (empty: zeros)."""
    if T.shape[0] == 0:
        return np.zeros(T.shape[1:])
    if order == 'pairwise':
        return T.sum(axis=0)
    if order == 'reversed':
        T = T[::-1]
    return np.cumsum(T, axis=0)[-1]


def _fold(parts):
    """(w0 + w1) + (w2 + w3) of consecutive groups of four."""
    p = parts.reshape((-1, 4) + parts.shape[1:])
    return (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])


def _swap_units(out, U, a, b):
    """Rows [aU, aU + U) and [bU, bU + U) of out exchanged (zeros past its
    end: what a unit past the live rows holds)."""
    rows = max(max(a, b) * U + U, out.shape[0])
    full = np.zeros((rows,) + out.shape[1:])
    full[:out.shape[0]] = out
    full[a * U:a * U + U], full[b * U:b * U + U] = (
        full[b * U:b * U + U].copy(), full[a * U:a * U + U].copy())
    return full[:out.shape[0]]


def replay_tdot(Xt, W, storage, order='forward', drop_row=None,
                drop_slot=None, swap_units=None):
    """G[K, P] = W Xt in float64 with the kernel's blocking: 32 row parts
    summed in `order`, the four-wave fold, the eight slabs in index order.
    drop_row: a row that is skipped; drop_slot = (part, slot): four rows of
    one part that are skipped; swap_units = (a, b): unit a's columns stored
    in unit b's place and the reverse."""
    K, n = W.shape
    P = Xt.shape[1]
    g = tdot_geometry(n, P, storage, K)
    terms = Xt[:, :, None] * W.T[:, None, :]          # [n, P, K]
    if drop_row is not None:
        terms[drop_row] = 0.
    sums = []
    for q, s in enumerate(g.n_slot):
        lo = q * g.rows_per_wave
        part = terms[lo:min(n, lo + g.rows_per_wave)]
        if drop_slot is not None and drop_slot[0] == q:
            part = part.copy()
            part[SLOT_ROWS * drop_slot[1]:SLOT_ROWS * drop_slot[1] + 4] = 0.
        sums.append(_sum64(part, order))
    slabs = _fold(np.stack(sums))                     # [8, P, K]
    out = np.cumsum(slabs, axis=0)[-1]                # b_finalize_kernel
    if swap_units is not None:
        out = _swap_units(out, unit(storage), *swap_units)
    return out.T


def replay_dot(Xt, V, OM, storage, order='forward', drop_row=None,
               drop_slot=None, swap_units=None, skip_rowscale=None):
    """(T, TS, TWT): T[K, n] = V Xt^T in float64 with the kernel's blocking
    (four quarters of the contracted rows, the fold), TS = OM .* T and
    TWT_c = sum_i fma-free TS T in row order.  drop_row: a contracted row;
    drop_slot = (quarter, slot); swap_units = (a, b): units of result rows;
    skip_rowscale: a chain whose rowscale is not applied."""
    K, P = V.shape
    n = Xt.shape[0]
    h = dot_geometry(n, P, storage, K)
    terms = Xt.T[:, :, None] * V.T[:, None, :]        # [P, n, K]
    if drop_row is not None:
        terms[drop_row] = 0.
    sums = []
    for q, s in enumerate(h.n_slot):
        lo = q * h.rows_per_wave
        part = terms[lo:min(P, lo + h.rows_per_wave)]
        if drop_slot is not None and drop_slot[0] == q:
            part = part.copy()
            part[SLOT_ROWS * drop_slot[1]:SLOT_ROWS * drop_slot[1] + 4] = 0.
        sums.append(_sum64(part, order))
    T = _fold(np.stack(sums))[0]                      # [n, K]
    if swap_units is not None:
        T = _swap_units(T, unit(storage), *swap_units)
    T = T.T
    scale = OM.copy()
    if skip_rowscale is not None:
        scale[skip_rowscale] = 1.
    TS = scale * T
    TWT = _sum64((TS * T).T, order)
    return T, TS, TWT
