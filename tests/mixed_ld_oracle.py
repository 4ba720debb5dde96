"""Host statement of the products of a MIXED design -- stored split by value,
X = B + D + S (csrc/spmv_tiled.hip HybridParts) -- the designs of the part-edge
cases built by shape, an integer flavour whose products are exact, a Gaussian
flavour with a derived componentwise bound, and planted faults.  Shared by the
CPU tests (test_mixed_ld_oracle.py, test_mixed_split_cpu.py) and the GPU tests
(test_hip_mixed_edges.py).  Plain NumPy / SciPy: no GPU, no libbbx.

A case is n rows by p = p_bin + kd columns:
    B   p_bin binary columns, FOUR ones a row in distinct columns (more where
        p_bin < 4 forces repeats: those are duplicates, legal CSR);
    D   kd full columns behind them.  Integer flavour: values from {-8 .. 8}
        without 0, so about one entry in sixteen is 1.0 and belongs to B;
        Gaussian flavour: N(0, 1) with every 11th entry set to 1.0.  The even
        rows never hold a 1.0 there, so a D column keeps >= max(n / 2, 1)
        values and stays a dense one at every n, n = 1, 2, 3 included;
    S   's' = None: absent;  'quad': one to three valued entries in each of the
        first min(n, 128) - 2 rows (at least one row), the rows behind empty --
        one step of one 128-row slice, and with n > 128 a second panel WITHOUT a
        single step: the shape from which the suite once met an illegal
        access;  'two': a quarter of the rows of each S column, every row
        range: with n > 128 at least two slices.  S sits in `s_cols` columns
        spread over the binary ones (fewer than n / 2 entries each, so none of
        them becomes a dense column) and needs n >= 8.

Integer flavour.  Every stored value, v, w in {-8 .. 8} and omega in {1 .. 4}
are integers, so every term and every partial sum of the three products is an
integer; `int_reference` asserts that the sum of the ABSOLUTE values of the
terms of every component stays below 2^51.  Then float64 holds every partial
sum in every order, fused or not, exactly: the reference is the int64 product
and the device must return it bit for bit.  Centring is left out: column means
are not integers.

Gaussian flavour.  The reference is np.longdouble.  A sum of m terms in any
order, with or without fused multiply-adds, errs by at most gamma_m sum|terms|,
gamma_m = m u / (1 - m u), u = 2^-53 (Higham, Accuracy and Stability, 3.1/3.4).
    X~ v, row i:      m = nnz_i + p + 4 (the row, the shared offset dot,
                      intercept, addend);  terms |v0|, |x_ij v_j|, |off_j v_j|
    X~^T w, column j: m = nnz_j + n + 4;  terms |x_ij w_i| and |off_j| |w_i|
                      (intercept component: the |w_i|)
    X~^T (Omega X~ v): t has the first bound, e_i; u_i = omega_i t_i adds one
                      rounding, f_i = omega_i e_i + u |u_i|; column j then
                      carries sum_i (|x_ij| + |off_j|) f_i on top of the second
                      bound applied to the u_i.
The tests allow TWICE these bounds (the offsets are themselves rounded means
and the reference is rounded to double on comparison)."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy import sparse

LD = np.longdouble
U = 2.0 ** -53
HYB_TDOT_CHUNKS = 256      # csrc/spmv_tiled.hip: row chunks of D^T w
ALLOW = 2.0                # the tests allow twice the derived bound
FAULT_SHARPNESS = 100.     # every planted fault lies this many bounds away


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1. - m * U)


# ---- designs -----------------------------------------------------------------
def _binary_part(rng, n, p_bin):
    per_row = 4
    cols = np.empty((n, per_row), dtype=np.int64)
    if p_bin >= per_row:
        # distinct columns per row: a start and a stride coprime handling is
        # not needed -- start + k * step with step < p_bin / 4
        start = rng.integers(0, p_bin, n)
        step = rng.integers(1, max(p_bin // per_row, 1) + 1, n)
        for k in range(per_row):
            cols[:, k] = (start + k * step) % p_bin
    else:
        cols[:] = rng.integers(0, p_bin, (n, per_row))
    rows = np.repeat(np.arange(n), per_row)
    return rows, cols.ravel(), np.ones(n * per_row)


def _s_columns(p_bin, s_cols):
    """s_cols columns spread over the binary ones, and the last one (with two
    column blocks S then sits in both)."""
    spread = (p_bin * (2 * np.arange(s_cols) + 1)) // (2 * s_cols)
    return np.unique(np.concatenate((spread, [p_bin - 1])))


def _values(rng, size, flavour):
    if flavour == 'int':
        v = rng.integers(1, 9, size).astype(np.float64)
        return v * rng.choice([-1., 1.], size)
    return rng.standard_normal(size)


def _valued_rest(rng, n, p_bin, s, s_cols, flavour):
    if s is None:
        return (np.zeros(0, np.int64),) * 2 + (np.zeros(0),)
    if n < 8:
        raise ValueError("a valued rest needs n >= 8: below that one entry "
                         "makes its column a dense one")
    sc = _s_columns(p_bin, s_cols)
    if s == 'quad':
        n_rows = max(min(n, 128) - 2, 1)
        cnt = rng.integers(1, 4, n_rows)
        rows = np.repeat(np.arange(n_rows), cnt)
        k = np.concatenate([np.arange(c) for c in cnt])
        cols = sc[(rows + k) % len(sc)]
        # fewer than n / 2 entries per column, so that none becomes dense
        keep = np.ones(len(rows), bool)
        for j in sc:
            at = np.flatnonzero(cols == j)
            keep[at[max(n // 2 - 1, 1):]] = False
        rows, cols = rows[keep], cols[keep]
    elif s == 'two':
        rows, cols = [], []
        for j in sc:
            m = max(min(n // 4, n // 2 - 1), 1)
            r = np.sort(rng.choice(n, m, replace=False))
            # (the last row always carries an entry: no empty trailing panel)
            r[-1] = n - 1
            rows.append(np.unique(r))
            cols.append(np.full(len(rows[-1]), j))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
    else:
        raise ValueError(s)
    vals = _values(rng, len(rows), flavour)
    vals[vals == 1.] = -3.          # a 1.0 would belong to B
    return rows, cols, vals


def _dense_part(rng, n, p_bin, kd, flavour):
    rows = np.tile(np.arange(n), kd)
    cols = np.repeat(p_bin + np.arange(kd), n)
    vals = _values(rng, n * kd, flavour)
    odd = (rows & 1) == 1
    if flavour == 'int':
        vals[(vals == 1.) & ~odd] = 2.
    else:
        vals[odd & (np.arange(n * kd) % 11 == 5)] = 1.
    return rows, cols, vals


@functools.lru_cache(maxsize=None)
def mixed_case(n, p_bin, kd, s=None, flavour='int', intercept=True,
               center=False, s_cols=7, seed=0):
    """One case by shape (cached: shared by the tests that need it, never
    changed).  Returns a namespace with the CSR arrays (int32 ids ascending per
    row, duplicates kept), the expected split, the inputs v (P), w (n),
    omega (n) and the column offsets."""
    if flavour == 'int' and center:
        raise ValueError("the integer flavour has no centring")
    rng = np.random.default_rng(
        [seed, n, p_bin, kd, {None: 0, 'quad': 1, 'two': 2}[s],
         int(flavour == 'int')])
    p = p_bin + kd
    parts = [_binary_part(rng, n, p_bin),
             _valued_rest(rng, n, p_bin, s, s_cols, flavour),
             _dense_part(rng, n, p_bin, kd, flavour)]
    rows = np.concatenate([q[0] for q in parts]).astype(np.int64)
    cols = np.concatenate([q[1] for q in parts]).astype(np.int64)
    vals = np.concatenate([q[2] for q in parts]).astype(np.float64)
    order = np.lexsort((cols, rows))        # stable: duplicates keep their order
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    indptr = np.cumsum(indptr)
    c = SimpleNamespace(n=n, p=p, p_bin=p_bin, kd=kd, s=s, flavour=flavour,
                        intercept=bool(intercept), center=bool(center))
    c.rows, c.cols, c.vals = rows, cols, vals
    c.indptr = indptr.astype(np.int32)
    c.indices = cols.astype(np.int32)
    c.P = p + int(c.intercept)
    # the split the library must find
    is_d = cols >= p_bin
    one = vals == 1.
    c.ones_nnz = int(one.sum())
    c.dense_nnz = int((is_d & ~one).sum())
    c.rest_nnz = int((~is_d & ~one).sum())
    c.dense_cols = list(range(p_bin, p))
    if center:
        X = sparse.csr_matrix((vals, c.indices, indptr), shape=(n, p))
        c.offset = np.asarray(X.mean(axis=0), dtype=np.float64).ravel()
    else:
        c.offset = None
    if flavour == 'int':
        c.v = rng.integers(-8, 9, c.P).astype(np.float64)
        c.w = rng.integers(-8, 9, n).astype(np.float64)
        c.omega = rng.integers(1, 5, n).astype(np.float64)
    else:
        c.v = rng.standard_normal(c.P)
        c.w = rng.standard_normal(n)
        c.omega = rng.uniform(.5, 2., n)
    for a in (c.rows, c.cols, c.vals, c.indptr, c.indices, c.v, c.w, c.omega):
        a.setflags(write=False)
    return c


def design(c, storage='tiled'):
    """The device design of a case (constant columns kept: from_csr_arrays)."""
    from bayesbridge_amd import HipSparseDesignMatrix
    return HipSparseDesignMatrix.from_csr_arrays(
        (c.n, c.p), c.indptr, c.indices, c.vals, column_offset=c.offset,
        add_intercept=c.intercept, storage=storage)


# ---- references ---------------------------------------------------------------
def _off(c, dtype):
    return (np.zeros(c.p, dtype) if c.offset is None
            else c.offset.astype(dtype))


def dot_ref(c, v, dtype=LD, drop=None):
    """X~ v from the triplets; `drop` = indices of triplets left out."""
    a = int(c.intercept)
    v = np.asarray(v).astype(dtype)
    keep = np.ones(len(c.vals), bool)
    if drop is not None:
        keep[np.atleast_1d(drop)] = False
    out = np.zeros(c.n, dtype)
    np.add.at(out, c.rows[keep],
              c.vals[keep].astype(dtype) * v[a:][c.cols[keep]])
    out -= np.sum(_off(c, dtype) * v[a:])
    if c.intercept:
        out += v[0]
    return out


def tdot_ref(c, w, dtype=LD, drop=None):
    w = np.asarray(w).astype(dtype)
    keep = np.ones(len(c.vals), bool)
    if drop is not None:
        keep[np.atleast_1d(drop)] = False
    out = np.zeros(c.p, dtype)
    np.add.at(out, c.cols[keep],
              c.vals[keep].astype(dtype) * w[c.rows[keep]])
    out -= np.sum(w) * _off(c, dtype)
    if c.intercept:
        out = np.concatenate(([np.sum(w)], out))
    return out


def gram_ref(c, omega, v, dtype=LD):
    return tdot_ref(c, np.asarray(omega).astype(dtype) * dot_ref(c, v, dtype),
                    dtype)


def int_reference(c, v=None, w=None, omega=None):
    """(X v, X^T w, X^T (omega X v)) as int64, with the 2^53 head-room of every
    partial sum asserted (sum of the absolute values of the terms)."""
    assert c.flavour == 'int' and c.offset is None
    v = c.v if v is None else v
    w = c.w if w is None else w
    omega = c.omega if omega is None else omega
    a = int(c.intercept)
    X = sparse.csr_matrix((c.vals.astype(np.int64), c.indices.copy(),
                           c.indptr.astype(np.int64)), shape=(c.n, c.p))
    # (|x| entry by entry: duplicates must not cancel before the absolute value)
    Xa = sparse.csr_matrix((np.abs(c.vals).astype(np.int64), c.indices.copy(),
                            c.indptr.astype(np.int64)), shape=(c.n, c.p))
    vi, wi, oi = (np.asarray(x).astype(np.int64) for x in (v, w, omega))
    assert np.array_equal(vi, v) and np.array_equal(wi, w)
    t = X @ vi[a:] + (vi[0] if a else 0)
    tw = X.T @ wi
    u = oi * t
    g = X.T @ u
    head = max((Xa @ np.abs(vi[a:])).max() + 8,
               (Xa.T @ np.abs(wi)).max(), np.abs(wi).sum(),
               (Xa.T @ np.abs(u)).max(), np.abs(u).sum())
    assert head < 2 ** 53 / 4, head
    if a:
        tw = np.concatenate(([wi.sum()], tw))
        g = np.concatenate(([u.sum()], g))
    return (t.astype(np.float64), tw.astype(np.float64), g.astype(np.float64))


# ---- the derived bounds ---------------------------------------------------------
def dot_bound(c, v):
    a = int(c.intercept)
    v = np.abs(np.asarray(v, dtype=np.float64))
    terms = np.zeros(c.n)
    np.add.at(terms, c.rows, np.abs(c.vals) * v[a:][c.cols])
    terms += np.sum(np.abs(_off(c, np.float64)) * v[a:])
    if a:
        terms += v[0]
    m = np.diff(c.indptr.astype(np.int64)) + c.p + 4
    return gamma(m) * terms


def tdot_bound(c, w):
    w = np.abs(np.asarray(w, dtype=np.float64))
    terms = np.zeros(c.p)
    np.add.at(terms, c.cols, np.abs(c.vals) * w[c.rows])
    terms += np.abs(_off(c, np.float64)) * w.sum()
    m = np.bincount(c.cols, minlength=c.p) + c.n + 4
    b = gamma(m) * terms
    if c.intercept:
        b = np.concatenate(([gamma(c.n + 4) * w.sum()], b))
    return b


def gram_bound(c, omega, v):
    omega = np.asarray(omega, dtype=np.float64)
    t = np.asarray(dot_ref(c, v), dtype=np.float64)
    u_vec = omega * t
    f = omega * dot_bound(c, v) + U * np.abs(u_vec)
    carried = np.zeros(c.p)
    np.add.at(carried, c.cols, np.abs(c.vals) * f[c.rows])
    carried += np.abs(_off(c, np.float64)) * f.sum()
    if c.intercept:
        carried = np.concatenate(([f.sum()], carried))
    return carried + tdot_bound(c, u_vec)


def ratio(got, ref, bound):
    """max_i |got_i - ref_i| / bound_i (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0., 0., err / bound)
    return float(np.max(r)) if r.size else 0.


# ---- planted faults -------------------------------------------------------------
def tdot_chunk_last_rows(n):
    """Last row of every non-empty row chunk of hyb_dense_tdot_kernel: chunks
    of ceil(n / 256) rows rounded up to an even count."""
    rows = -(-n // HYB_TDOT_CHUNKS)
    rows = (rows + 1) // 2 * 2
    starts = np.arange(0, n, rows)
    return np.minimum(starts + rows, n) - 1


def planted_faults(c):
    """{name: (product, triplet index)} for the faults this case can carry:
    'S entry' (an entry of the valued rest missing from X~ v), 'D row' (one row
    of one dense column missing from X~ v) and 'chunk tail' (the last row of a
    chunk of one dense column missing from X~^T w).  The entry is the one
    whose own term is largest relative to the bound of its component."""
    a = int(c.intercept)
    is_d = c.cols >= c.p_bin
    not_one = c.vals != 1.
    bd, bt = dot_bound(c, c.v), tdot_bound(c, c.w)
    term_v = np.abs(c.vals * c.v[a:][c.cols]) / bd[c.rows]
    term_w = np.abs(c.vals * c.w[c.rows]) / bt[a:][c.cols]
    out = {}
    cand = np.flatnonzero(~is_d & not_one)
    if len(cand):
        out['S entry'] = ('dot', int(cand[np.argmax(term_v[cand])]))
    cand = np.flatnonzero(is_d & not_one)
    if len(cand):
        out['D row'] = ('dot', int(cand[np.argmax(term_v[cand])]))
        tails = np.isin(c.rows, tdot_chunk_last_rows(c.n))
        cand = np.flatnonzero(is_d & not_one & tails)
        if len(cand):
            out['chunk tail'] = ('tdot', int(cand[np.argmax(term_w[cand])]))
    return out


# ---- the cases --------------------------------------------------------------------
SEP_KD = (0, 1, 3, 4, 5, 8, 9)
SEP_S = (None, 'quad', 'two')
SEP_N = (2, 129, 130, 131, 255, 256, 257, 511, 512, 513)
EPI_KD = (1, 7, 8)
EPI_N = (1, 2, 127, 128, 129, 1025)
WAVE_KD = (9, 127, 128, 129, 256, 257, 512, 513, 1023, 1024)
WAVE_N = (1, 3, 63, 64, 65)
WAVE_LAP_N = (16383, 16384, 16385)
WG_KD = (1025, 2048, 2049, 4096, 4097, 8191, 8192)
WG_N = (1, 2, 5, 65)
BATCH_KD = (0, 1, 3, 8, 9)
BATCH_N = (130, 257)
P_BIN = 65


def separate_cases(flavour, n):
    """kd x S at one n (n = 2: no valued rest; kd = 0 without S is a binary
    design, not a mixed one, and is left to the binary tests)."""
    out = []
    for kd in SEP_KD:
        for s in SEP_S:
            if (s is not None and n < 8) or (kd == 0 and s is None):
                continue
            out.append(mixed_case(n, P_BIN, kd, s, flavour, True,
                                  flavour != 'int' and kd % 2 == 1))
    return out


def case8_cases(flavour):
    """130 x 65, no dense column, S of one step in one slice whose second
    panel is empty, with the four flag combinations (integer flavour: the two
    without centring)."""
    return [mixed_case(130, P_BIN, 0, 'quad', flavour, i, ctr)
            for i in (False, True) for ctr in (False, True)
            if not (ctr and flavour == 'int')]


def gaussian_cases():
    """Every case of the Gaussian flavour that the device tests run (the
    largest shapes excepted where the integer flavour carries them)."""
    out = []
    for n in SEP_N:
        out += separate_cases('gauss', n)
    out += case8_cases('gauss')
    out.append(mixed_case(130, 16130, 0, 'two', 'gauss', True, True, 11))
    for kd in EPI_KD:
        for n in EPI_N:
            out.append(mixed_case(n, 40, kd, None, 'gauss', False, False))
    for kd in WAVE_KD:
        for n in WAVE_N:
            out.append(mixed_case(n, 40, kd, None, 'gauss', False, False))
    for kd in WG_KD:
        out.append(mixed_case(5, 40, kd, None, 'gauss', False, False))
    # (one of the case-[8] flag combinations is also a `separate` case)
    return list({id(c): c for c in out}.values())
