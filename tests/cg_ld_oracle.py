"""Host statement of one conjugate-gradient draw (csrc/cg_sampler.hip) in long
double, the designs and inputs of the P-vector edge cases, integer cases whose
products are exact, and planted faults -- shared by the CPU tests
(test_cg_ld_oracle.py) and the GPU tests (test_hip_cg_edges.py).  Plain NumPy:
no GPU, no libbbx.

The P-length work of a solve runs on NPART x VEC_BLOCK = 256 x 256 = 65 536
threads (csrc/vecops.hip, the finalize of csrc/spmv_csr.hip); a thread's first
coordinate is pre-loaded, every further one is loaded inside a grid-stride
loop whose first trip starts at coordinate 65 536.  The folded step of
csrc/spmv_tiled.hip gives each workgroup ceil(P / n_wg) coordinates, 1024 at a
time.  The widths below sit around a wave (64), a block (256), the first trip
(65 536) and the third (2 x 65 536).

`replay` restates the header of csrc/cg_sampler.hip (cg_sampler.py:61-94,
104-109,128-138 and SciPy's `cg` recurrence):
    s_j = 2 sd_j (j < n_unshrunk) | 1 / phi_j ;  d = (s phi)^2
    b = s (z + X~^T(sqrt(Omega) eta1) + phi eta2) ;  x = x0 / s
    r = b - A x   (r = b when x0 is all zero) ;  A x = d x + s X~^T Omega X~ (s x)
    for k < maxiter: if ||r|| < atol: stop;  rho = r.r;
        p = r + (rho / rho_prev) p;  q = A p;  alpha = rho / (p.q);
        x += alpha p;  r -= alpha q
    coef = s x
in np.longdouble (80-bit, eps 1.08e-19) or np.float64.  Products come from the
COO triplets through np.add.at, in the triplets' order or in the reversed one;
the inner products are np.sum of the terms in the same two orders.

Solves cut at maxiter = 1 and 2 are the sharp probe: there the float64 replay
stays within about 1e-14 of the long-double one (relative to max|coef|), while
one stale or mis-indexed coordinate is off by the size of its own update,
about 1e-2 of the scale with the inputs used here (local scales within a
factor e^.3 of each other, z ~ N(0, 3^2)).

The integer cases need no bound: v, w integers in [-8, 8], omega in 1..4 and
a binary design on 256 rows whose column means are multiples of 2^-8.  Every
term and every partial sum of X~ v and X~^T w is then a multiple of 2^-8, of
X~^T (Omega X~ v) a multiple of 2^-16, and the sum of the absolute values of
all terms of any component stays below 2^53 / 2^16 (asserted in `int_case`):
float64 holds every partial sum in every order, fused or not, exactly, and the
device must return the int64 result bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
N_ROWS = 256               # column means are multiples of 2^-8
TRIP = 65536               # NPART x VEC_BLOCK: coordinates of one loop trip
FOLD_THREADS = 1024        # TILE_THREADS: coordinates of one trip of the fold

# ---- tolerances of the truncated solves --------------------------------------
# max_j |coef_j - coef_ld_j| / max|coef_ld| after k iterations.  Measured by
# test_cg_ld_oracle.py::test_float64_replay_is_within_the_constants over every
# case of TRUNC_CASES and the extra designs, both summation orders (x86-64,
# NumPy 2.2, 80-bit long double):
#     k = 1:  7.87e-16 (binary P = 65 601, warm start, natural order)
#     k = 2:  6.41e-15 (dense 257 x 65 537, reversed order; natural 5.76e-15;
#             the sparse designs at most 4.40e-15, most of them below 1e-15)
# rounded up in MEASURED,
# times MARGIN = 32: the device differs from the host's float64 runs by a third
# summation order (256 block partials re-added per wave), by fused
# multiply-adds and by the one-pass form of the initial residual -- roundings
# of the kind the two host orders already differ by, so the margin is for the
# number of such choices, not for another kind of error.
MARGIN = 32.
MEASURED = {1: 8.0e-16, 2: 6.5e-15}
TRUNC_TOL = {k: MARGIN * v for k, v in MEASURED.items()}
# every planted fault misses TRUNC_TOL[2] by at least this factor
FAULT_SHARPNESS = 1000.


# ---- designs -----------------------------------------------------------------
def _pattern(rng, n, p, empty):
    """2..4 entries per column in distinct rows (base + k step mod n with
    3 step < n), none in the columns of `empty`; triplets in CSR order."""
    m = rng.integers(2, 5, p)
    m[list(empty)] = 0
    base = rng.integers(0, n, p)
    step = rng.integers(1, max(n // 4, 2), p)
    cols = np.repeat(np.arange(p), m)
    k = np.arange(cols.size) - np.repeat(np.cumsum(m) - m, m)
    rows = (base[cols] + k * step[cols]) % n
    order = np.lexsort((cols, rows))
    return rows[order], cols[order]


@functools.lru_cache(maxsize=None)
def design(P, intercept=True, kind='binary', n=N_ROWS, seed=0):
    """The design of width P (intercept included): n, p, COO triplets in CSR
    order (rows, cols, vals [None: all 1.0]), the float64 centring offsets
    (column means) and the CSR arrays.  Empty columns sit at coordinates
    65 535 and 65 537 where the design has them, else at predictor 1.
    kind: 'binary'; 'valued' (the same patterns with N(0, 1) values);
    'mixed' (binary, with three predictors replaced by full N(0, 1) columns:
    the first, the middle one and the last); 'dense' (n x p, N(0, 1) rounded
    to float32, not centred -- a matrix, no triplets)."""
    p = P - int(intercept)
    assert p >= 1
    rng = np.random.default_rng([91, n, P, int(intercept), seed])
    c = SimpleNamespace(n=n, p=p, P=P, intercept=bool(intercept), kind=kind)
    if kind == 'dense':
        X = rng.standard_normal((n, p)).astype(np.float32).astype(np.float64)
        c.X, c.offset = X, None
        c.Xt = np.hstack((np.ones((n, 1)), X)) if intercept else X
        c.Xt.setflags(write=False)
        return c
    empty = [j - int(intercept) for j in (TRIP - 1, TRIP + 1) if j < P - 1]
    if not empty and p >= 6:
        empty = [1]
    rows, cols = _pattern(rng, n, p, empty)
    vals = None
    if kind == 'valued':
        vals = rng.standard_normal(rows.size)
    elif kind == 'mixed':
        dense_cols = sorted({0, p // 2, p - 1})
        assert len(dense_cols) == 3
        keep = ~np.isin(cols, dense_cols)
        r2 = np.concatenate([rows[keep]] + [np.arange(n)] * 3)
        c2 = np.concatenate([cols[keep]] + [np.full(n, j) for j in dense_cols])
        v2 = np.concatenate((np.ones(int(keep.sum())),
                             rng.standard_normal(3 * n)))
        order = np.lexsort((c2, r2))
        rows, cols, vals = r2[order], c2[order], v2[order]
        c.dense_cols = dense_cols
    else:
        assert kind == 'binary'
    c.rows, c.cols, c.vals, c.empty = rows, cols, vals, empty
    weights = vals if vals is not None else None
    c.offset = np.bincount(cols, weights=weights, minlength=p) / n
    if vals is None and n & (n - 1) == 0:
        assert np.array_equal(c.offset * n, np.round(c.offset * n))
    c.indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n))))
    c.indptr = c.indptr.astype(np.int32)
    c.indices = cols.astype(np.int32)
    for a in (c.rows, c.cols, c.offset, c.indptr, c.indices):
        a.setflags(write=False)
    if vals is not None:
        vals.setflags(write=False)
    return c


def _dense_as(c, dtype, rev=False):
    """The dense design's matrix in `dtype`, or (rev) a contiguous copy with
    rows and columns in reversed order; converted once."""
    key = 'Xt_%s%s' % (np.dtype(dtype).name, '_rev' if rev else '')
    if getattr(c, key, None) is None:
        setattr(c, key, np.ascontiguousarray(
            c.Xt[::-1, ::-1] if rev else c.Xt, dtype=dtype))
    return getattr(c, key)


def _total(a, rev):
    return np.sum(a[::-1] if rev else a)


def dot(c, v, dtype=LD, rev=False):
    """X~ v = v0 + X v1 - <offset, v1> (intercept and centring as the device
    design has them), terms added in triplet order (rev: reversed)."""
    v = np.asarray(v, dtype=dtype)
    if c.kind == 'dense':
        # (float64: element-wise products and NumPy's own sums, not `@` -- a
        # BLAS picks its kernels, and with them the order of a sum, by
        # machine; long double has no BLAS and goes through the generic loop)
        if dtype != np.float64:
            return _dense_as(c, dtype) @ v
        if rev:
            return (_dense_as(c, dtype, True) * v[::-1]).sum(axis=1)[::-1]
        return (_dense_as(c, dtype) * v).sum(axis=1)
    v1 = v[int(c.intercept):]
    terms = v1[c.cols]
    if c.vals is not None:
        terms = np.asarray(c.vals, dtype=dtype) * terms
    rows = c.rows
    if rev:
        rows, terms = rows[::-1], terms[::-1]
    out = np.zeros(c.n, dtype=dtype)
    np.add.at(out, rows, terms)
    out -= _total(np.asarray(c.offset, dtype=dtype) * v1, rev)
    if c.intercept:
        out += v[0]
    return out


def tdot(c, w, dtype=LD, rev=False):
    """X~^T w = [sum w ; X^T w - sum(w) offset]."""
    w = np.asarray(w, dtype=dtype)
    if c.kind == 'dense':
        if dtype != np.float64:
            return w @ _dense_as(c, dtype)
        if rev:
            return (w[::-1, None] * _dense_as(c, dtype, True)).sum(axis=0)[::-1]
        return (w[:, None] * _dense_as(c, dtype)).sum(axis=0)
    terms = w[c.rows]
    if c.vals is not None:
        terms = np.asarray(c.vals, dtype=dtype) * terms
    cols = c.cols
    if rev:
        cols, terms = cols[::-1], terms[::-1]
    g = np.zeros(c.p, dtype=dtype)
    np.add.at(g, cols, terms)
    tot = _total(w, rev)
    g -= tot * np.asarray(c.offset, dtype=dtype)
    if c.intercept:
        g = np.concatenate((np.array([tot], dtype=dtype), g))
    return g


# ---- inputs --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(n, P, n_unshrunk, seed, warm, wide=True):
    from helpers import cg_inputs
    inp = cg_inputs(n, P, n_unshrunk=n_unshrunk, seed=seed, lam_log_sd=.3)
    # Two changes keep the truncated solves sharp.  (1) Prior scales ten times
    # wider (about .5): the data part s^2 X~^T Omega X~ of the operator is
    # then of the order of its diagonal part d instead of 1e-3 of it, so a
    # fault in what feeds the products moves the draw as much as one in the
    # vector updates.  (2) The intercept's scale 2 sd_0 is set to the
    # posterior's own, 1 / sqrt(sum Omega), instead of O(1): with sd_0 ~ 1 the
    # preconditioned system has one eigenvalue sum(Omega) = 1e2..1e4 times the
    # others and the float64 replay itself is only good to 1e-12 after two
    # iterations.
    # (the dense design keeps the narrow prior -- every one of its 65 536
    # columns is full, so its data part is 1e2 times a sparse column's as it
    # is -- and gets observation weights within .3 .. .45 instead of over
    # three decades: X X^T of a wide Gaussian matrix is close to a multiple of
    # the identity, so the 257 large eigenvalues of its operator then lie
    # together and a solve takes a dozen iterations instead of 98, each of
    # them two long-double passes over 257 x 65 537 entries)
    phi = inp['prior_prec_sqrt']
    if wide:
        phi[n_unshrunk:] *= .1
    else:
        inp['obs_prec'] = .3 + .05 * inp['obs_prec']
    if n_unshrunk > 0:
        inp['coef_scaled_sd'][0] = .5 / np.sqrt(inp['obs_prec'].sum())
    if not warm:
        inp['coef_cg_init'] = np.zeros(P)
    for a in inp.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp


def inputs(case, warm=None):
    """helpers.cg_inputs(..., lam_log_sd=.3) of the case (read-only arrays; a
    cold start has coef_cg_init all zero).  warm: None = the case's own."""
    return _inputs(case.n, case.P, case.nu, case.seed,
                   case.warm if warm is None else bool(warm),
                   case.kind != 'dense')


def oracle_design(c):
    """The project's float64 oracle operator (oracle.OracleSparseDesign) on
    the triplets of a sparse design `c`, with no column dropped."""
    import scipy.sparse as sparse
    from oracle.design_matrix import OracleSparseDesign, _Counting
    vals = np.ones(c.rows.size) if c.vals is None else c.vals
    X = sparse.csr_matrix((vals, c.indices, c.indptr), shape=(c.n, c.p))
    self = OracleSparseDesign.__new__(OracleSparseDesign)
    _Counting.__init__(self)
    self.X_main, self.X_main_T = X, X.T
    self.centered, self.intercept_added = True, c.intercept
    self.column_offset = np.array(c.offset)
    return self


# ---- planted faults ------------------------------------------------------------
# One per kernel role; each touches one coordinate only (fault_coordinate).
FAULTS = ('x_stale',         # x_j not updated in iteration 2 (update kernels)
          'beta_dropped',    # p_j = r_j: beta * p_j dropped (direction step)
          'pdp_missing',     # d_j p_j^2 left out of <p, d p> (the curvature)
          'r_prev_alpha',    # r_j updated with the previous alpha (0 at first)
          'sr_stale',        # s_j r_j not written for the next folded step
          'read_shifted')    # p_j read from j - 65 536 (small cases: j - 1)


def fault_coordinate(P):
    """(j, shift): the coordinate a planted fault touches -- 65 536, the first
    of the loops' second trip, where the design has it, else the last one --
    and how far below it 'read_shifted' reads."""
    return (TRIP, TRIP) if P > TRIP else (P - 1, 1)


def fault_applies(fault, P):
    return P >= 2 or fault != 'read_shifted'


# ---- the replay ----------------------------------------------------------------
def replay(c, inp, n_unshrunk, maxiter, atol, dtype=LD, order='natural',
           fault=None):
    """One CG draw on design `c` (see the module text): (coef, n_iter,
    converged).  order: 'natural' | 'reversed' summation.  fault: None or one
    of FAULTS (negative controls)."""
    assert order in ('natural', 'reversed')
    rev = order == 'reversed'
    T = dtype
    omega, phi, z, x0, sd, eta1, eta2 = (
        np.asarray(inp[k], dtype=T) for k in (
            'obs_prec', 'prior_prec_sqrt', 'z', 'coef_cg_init',
            'coef_scaled_sd', 'randn_n', 'randn_P'))
    P = c.P
    nu = int(n_unshrunk)
    s = np.empty(P, dtype=T)
    s[:nu] = 2 * sd[:nu]
    s[nu:] = 1 / phi[nu:]
    d = (s * phi) ** 2

    def op_of(sv, pv):
        return d * pv + s * tdot(c, omega * dot(c, sv, T, rev), T, rev)
    b = s * (z + tdot(c, np.sqrt(omega) * eta1, T, rev) + phi * eta2)
    x = x0 / s
    r = b - op_of(s * x, x) if x0.any() else b.copy()
    j, shift = fault_coordinate(P)
    sr = s * r
    p = sp = None
    rho_prev = alpha_prev = T(0)
    n_iter, converged = 0, False
    for k in range(maxiter):
        rho = _total(r * r, rev)
        if np.sqrt(rho) < atol:
            converged = True
            break
        if k == 0:
            p = r.copy()
            sp = s * p
        else:
            beta = rho / rho_prev
            p_old, sp_old = p, sp
            p = r + beta * p_old
            if fault == 'beta_dropped':
                p[j] = r[j]
            elif fault == 'read_shifted':
                p[j] = r[j] + beta * p_old[j - shift]
            sp = s * p
            if fault == 'sr_stale':
                sp[j] = sr[j] + beta * sp_old[j]
        q = op_of(sp, p)
        pq = _total(p * q, rev)
        if fault == 'pdp_missing':
            pq = pq - d[j] * p[j] * p[j]
        alpha = rho / pq
        x_new = x + alpha * p
        if fault == 'x_stale' and k == 1:
            x_new[j] = x[j]
        r_new = r - alpha * q
        if fault == 'r_prev_alpha':
            r_new[j] = r[j] - alpha_prev * q[j]
        sr_new = s * r_new
        if fault == 'sr_stale':
            sr_new[j] = sr[j]
        x, r, sr = x_new, r_new, sr_new
        rho_prev, alpha_prev = rho, alpha
        n_iter += 1
    return s * x, n_iter, converged


def rel_err(coef, coef_ld):
    """max_j |coef_j - coef_ld_j| / max|coef_ld|, in long double."""
    ref = np.asarray(coef_ld, dtype=LD)
    return float(np.abs(np.asarray(coef, dtype=LD) - ref).max()
                 / np.abs(ref).max())


# ---- the case table ------------------------------------------------------------
def case(P, intercept=True, nu=1, warm=True, kind='binary', n=N_ROWS, seed=0):
    name = "%s-P%d%s-nu%d-%s%s" % (kind, P, '' if intercept else '-noint', nu,
                                   'warm' if warm else 'cold',
                                   '' if n == N_ROWS else '-n%d' % n)
    return SimpleNamespace(name=name, P=P, intercept=intercept, nu=nu,
                           warm=warm, kind=kind, n=n, seed=seed + P % 7)


def design_of(cs):
    return design(cs.P, cs.intercept, cs.kind, cs.n)


P_SMALLEST = (1, 2, 3)             # 1: no intercept
P_WAVE = (63, 64, 65)
P_BLOCK = (255, 256, 257)
P_TRIP = (65535, 65536, 65537)
P_PAST = (65601,)
P_THIRD = (131073,)                # two full further trips and a ragged third
P_ALL = P_SMALLEST + P_WAVE + P_BLOCK + P_TRIP + P_PAST + P_THIRD


def _table():
    out = []
    for i, P in enumerate(P_ALL):
        # n_unshrunk 0, 1, 2 and warm / cold starts rotate over the widths
        nu = 0 if P == 1 else (1, 2, 0)[i % 3] if P > 2 else 1
        out.append(case(P, intercept=P > 1, nu=nu, warm=i % 2 == 0))
    out.append(case(3, nu=3, warm=True))            # n_unshrunk = P
    out.append(case(257, nu=1, warm=False))
    out.append(case(65537, nu=1, warm=True))
    out.append(case(65601, nu=1, warm=False))
    out.append(case(65601, nu=1, warm=True))
    return list({cs.name: cs for cs in out}.values())


TRUNC_CASES = _table()
# the extra designs of the GPU paths: valued entries, three dense columns next
# to binary ones, a dense design (n = 257: 5 rows per chunk of the Tdot, most
# of the 64 chunks ragged or empty), 20 000 rows (157 workgroups of 128 rows)
EXTRA_CASES = ([case(P, kind='valued', warm=w)
                for P, w in ((3, True), (257, False), (65601, True))]
               + [case(P, kind='mixed', warm=w)
                  for P, w in ((260, True), (65601, False))]
               + [case(65537, kind='dense', n=257, warm=True)]
               + [case(P, n=20000, warm=w)
                  for P, w in ((2, True), (3, False), (157, True),
                               (65601, True))])


def trunc_iters(cs):
    """The cut-off counts of a case: maxiter = 1 and 2; a width-1 system is
    solved exactly by one iteration (r = 0 up to rounding, the second
    iteration divides rounding noise by rounding noise), so it has k = 1
    only."""
    return (1,) if cs.P == 1 else (1, 2)


@functools.lru_cache(maxsize=None)
def _reference(name, maxiter, atol):
    cs = CASES_BY_NAME[name]
    return replay(design_of(cs), inputs(cs), cs.nu, maxiter, atol, LD)


def reference(cs, maxiter, atol=0.):
    """The long-double replay of a case, computed once and left unchanged."""
    coef, n_iter, conv = _reference(cs.name, maxiter, float(atol))
    coef.setflags(write=False)
    return coef, n_iter, conv


CASES_BY_NAME = {cs.name: cs for cs in TRUNC_CASES + EXTRA_CASES}
assert len(CASES_BY_NAME) == len(TRUNC_CASES) + len(EXTRA_CASES)


# ---- integer operator cases ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_case(P, intercept=True, n=N_ROWS):
    """The binary design of width P with integer v[P], w[n] in [-8, 8] and
    omega[n] in 1..4, and the exact products as float64: t = X~ v, g = X~^T w,
    op = X~^T (omega .* t), from int64 arithmetic scaled by n (t, g) and n^2
    (op).  n is a power of two.  Asserts the exactness condition itself."""
    assert n & (n - 1) == 0
    c = design(P, intercept, 'binary', n)
    rng = np.random.default_rng([92, n, P, int(intercept)])
    v = rng.integers(-8, 9, P)
    w = rng.integers(-8, 9, n)
    omega = rng.integers(1, 5, n)
    cnt = np.round(c.offset * n).astype(np.int64)      # column counts
    assert np.array_equal(cnt / n, c.offset)
    i0 = int(intercept)

    def right(x, xabs):
        """(n X~ x, sum of |terms| of the worst row) for integer x[P]."""
        x1 = x[i0:]
        out = np.zeros(n, dtype=np.int64)
        np.add.at(out, c.rows, n * x1[c.cols])
        out -= np.sum(cnt * x1)
        big = np.zeros(n, dtype=np.int64)
        np.add.at(big, c.rows, n * xabs[i0:][c.cols])
        big += np.sum(cnt * xabs[i0:])
        if intercept:
            out += n * x[0]
            big += n * xabs[0]
        return out, big

    def left(y, yabs):
        """(n X~^T y, sum of |terms| per column) for integer y[n]."""
        g = np.zeros(c.p, dtype=np.int64)
        np.add.at(g, c.cols, n * y[c.rows])
        tot = np.sum(y)
        g -= tot * cnt
        big = np.zeros(c.p, dtype=np.int64)
        np.add.at(big, c.cols, n * yabs[c.rows])
        big += np.sum(yabs) * cnt
        if intercept:
            g = np.concatenate(([n * tot], g))
            big = np.concatenate(([n * np.sum(yabs)], big))
        return g, big
    t, t_abs = right(v, np.abs(v))
    g, g_abs = left(w, np.abs(w))
    op, op_abs = left(omega * t, omega * t_abs)          # scaled by n^2
    abs_max = max(int(t_abs.max()) * n, int(g_abs.max()) * n,
                  int(op_abs.max()))
    assert abs_max < 2 ** 53, (P, abs_max)
    out = SimpleNamespace(design=c, P=P, intercept=intercept, abs_max=abs_max,
                          v=v.astype(np.float64), w=w.astype(np.float64),
                          omega=omega.astype(np.float64),
                          t=t / n, g=g / n, op=op / (n * n))
    # the scaled integers divide exactly (powers of two, results below 2^53)
    assert np.array_equal(out.t * n, t) and np.array_equal(out.g * n, g)
    assert np.array_equal(out.op * (n * n), op)
    for a in (out.v, out.w, out.omega, out.t, out.g, out.op):
        a.setflags(write=False)
    return out


def release():
    """Drops the cached designs, inputs, references and integer cases (the
    dense design alone holds 0.7 GB in its float64 and long-double forms)."""
    for f in (design, _inputs, _reference, int_case):
        f.cache_clear()
