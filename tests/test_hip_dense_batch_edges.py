"""GPU: the batched dense products (csrc/dense_batch.hip, the K-column X V and
X^T W on the f64 matrix cores) at the edges of their kernels -- row parts with
no row, one row, one slot; parts of exactly s slots for s around one and two
periods of the register ring of either depth; one unit, one column block and
8 columns to either side; wave quarters of the contraction with 0 rows, 1 row,
1 slot; and every sweep width of every instantiation (the three-unit f32 tail
included).  tests/dense_batch_oracle.py derives the cases from the kernels'
geometry and tests/test_dense_batch_oracle.py checks, without a GPU, that each
has the property it is listed for.

The X V product is taken in both forms: as `bbx_batch_dot` launches it and as
the CG loop does (`HipChainBatch.dot(v, rowscale, return_twt=True)`: per-chain
rowscale, interleaved output, the partials of <t, Omega t>).

  * integer cases: every partial sum in every order is an integer below 2^53,
    so the device must EQUAL the int64 results -- products, scaled products,
    <t, Omega t>;
  * Gaussian cases on a centred design with intercept: within the derived
    per-component bounds of the long-double products of stored(...);
  * isolation: a chain full of NaN and infinities leaves the other chains'
    bits alone; the products leave the batch as they found it.
LABNOTES, "Batched dense products at kernel edges", has the case table and the
observed error / bound ratios."""
from ctypes import c_void_p

import numpy as np
import pytest

import dense_batch_oracle as dbo
import dense_ld_oracle as dlo
from test_hip_dense_edges import _design, _int_design

pytestmark = pytest.mark.gpu

CASES = dbo.all_cases()
IDS = ["%dx%d" % c for c in CASES]


def _batch(design, K):
    """A batch of K linear chains on `design` (never run: the products only)."""
    from bayesbridge_amd import HipChainBatch, HipGibbsChain
    n, P = design.shape
    y = np.random.default_rng(n + P).standard_normal(n)
    sd = [np.inf] if P > 1 else []
    chains = [HipGibbsChain(design, 'linear', y, sd_unshrunk=sd, seed=s)
              for s in range(K)]
    return HipChainBatch(chains, allow_slow=True)


def _eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64),
                          np.asarray(b, dtype=np.float64))


# ---- a. integer cases: equality ---------------------------------------------
@pytest.mark.parametrize("storage", dbo.STORAGES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_products_are_exact_on_integer_cases(case, storage):
    n, P = case
    design = _int_design(dlo.int_case(n, P), storage)
    for K in dbo.case_widths(n):
        b = dbo.int_batch(n, P, K)          # asserts the 2^53 condition
        assert b.abs_max < 2 ** 53
        dbo.assert_padding(n, P, storage, K)
        batch = _batch(design, K)
        tag = (n, P, K, storage)
        T, G = batch.dot(b.V), batch.Tdot(b.W)
        assert _eq(T, b.T), tag
        assert _eq(G, b.G), tag
        TS, part, twt = batch.dot(b.V, b.OM, return_twt=True)
        assert _eq(TS, b.TS), tag
        assert _eq(twt, b.TWT), tag
        assert part.shape == (K, dbo.NPART)
        assert _eq(part.sum(axis=1), b.TWT), tag       # integers: any order
        # without a rowscale, sums on: the plain product and sum t^2
        T1, part1, twt1 = batch.dot(b.V, None, return_twt=True)
        assert _eq(T1, b.T) and _eq(twt1, (b.T * b.T).sum(axis=1)), tag
        # a unit vector per chain, each at its own index: stored columns / rows
        jj = (P - 1 - np.arange(K)) % P
        ii = (n - 1 - 5 * np.arange(K)) % n
        EV, EW = np.zeros((K, P)), np.zeros((K, n))
        EV[np.arange(K), jj] = 1.
        EW[np.arange(K), ii] = 1.
        assert _eq(batch.dot(EV), b.Xi[:, jj].T), tag
        assert _eq(batch.Tdot(EW), b.Xi[ii, :]), tag
        # permuted chains: permuted outputs, bit for bit
        perm = np.roll(np.arange(K), 1)
        assert _eq(batch.dot(b.V[perm]), T[perm]), tag
        assert _eq(batch.Tdot(b.W[perm]), G[perm]), tag
        TSp, partp, _ = batch.dot(b.V[perm], b.OM[perm], return_twt=True)
        assert _eq(TSp, TS[perm]) and _eq(partp, part[perm]), tag
        # a second call: the same bits
        TS2, part2, _ = batch.dot(b.V, b.OM, return_twt=True)
        assert _eq(TS2, TS) and _eq(part2, part), tag
        assert _eq(batch.Tdot(b.W), G), tag
        batch.close()


# ---- b. Gaussian cases: the derived bounds ----------------------------------
def _within(out, ref, bound, what):
    r = dlo.ratio(out, ref, bound)
    print("ratio %s: %.2e of the bound" % (what, r))
    return r <= 1.


@pytest.mark.parametrize("storage", dbo.STORAGES)
@pytest.mark.parametrize("case", dbo.gauss_cases(),
                         ids=["%dx%d" % c for c in dbo.gauss_cases()])
def test_products_keep_the_derived_bounds(case, storage):
    n, P = case
    assert n * dlo.ld_of(P) <= dlo.GAUSS_MAX_ENTRIES
    design = _design(dlo.gauss_case(n, P).X, 'float64', storage, True, True)
    for K in dbo.case_widths(n):
        g = dbo.gauss_batch(n, P, K, storage)
        batch = _batch(design, K)
        tag = "%dx%d K=%d %s" % (n, P, K, storage)
        T, G = batch.dot(g.V), batch.Tdot(g.W)
        TS, part, twt = batch.dot(g.V, g.OM, return_twt=True)
        ok = [_within(T, g.T, g.T_bound, "X V " + tag),
              _within(G, g.G, g.G_bound, "X^T W " + tag),
              _within(TS, g.TS, g.TS_bound, "omega X V " + tag),
              _within(twt, g.TWT, g.TWT_bound, "<t, Omega t> " + tag)]
        assert all(ok), (tag, ok)
        assert _eq(batch.dot(g.V), T) and _eq(batch.Tdot(g.W), G), tag
        batch.close()


# ---- c. isolation -----------------------------------------------------------
@pytest.mark.parametrize("storage", dbo.STORAGES)
@pytest.mark.parametrize("K,bad", [(2, 1), (16, 5), (32, 3), (32, 20)])
def test_a_poisoned_chain_leaves_the_others_alone(K, bad, storage):
    """One chain's v (and, separately, its w) full of NaN and +-inf: every
    other chain's outputs and <t, Omega t> partials are bit for bit those of
    the run with finite values (K = 32: the poisoned chain in the first and in
    the second group of 16)."""
    n, P = 129, 257                          # three column blocks, three units
    g = dbo.gauss_batch(n, P, K, storage)
    batch = _batch(_design(dlo.gauss_case(n, P).X, 'float64', storage, True,
                           True), K)
    poison = np.array([np.nan, np.inf, -np.inf])
    others = np.arange(K) != bad
    TS, part, _ = batch.dot(g.V, g.OM, return_twt=True)
    T, G = batch.dot(g.V), batch.Tdot(g.W)
    V, W = g.V.copy(), g.W.copy()
    V[bad] = poison[np.arange(P) % 3]
    W[bad] = poison[np.arange(n) % 3]
    TSb, partb, _ = batch.dot(V, g.OM, return_twt=True)
    assert _eq(TSb[others], TS[others]) and _eq(partb[others], part[others])
    assert not np.isfinite(TSb[bad]).any() and not np.isfinite(partb[bad]).all()
    assert _eq(batch.dot(V)[others], T[others])
    Gb = batch.Tdot(W)
    assert _eq(Gb[others], G[others]) and not np.isfinite(Gb[bad]).any()
    # and the finite run again on the same handle
    TS2, part2, _ = batch.dot(g.V, g.OM, return_twt=True)
    assert _eq(TS2, TS) and _eq(part2, part) and _eq(batch.Tdot(g.W), G)


# ---- d. the same handle afterwards ------------------------------------------
@pytest.mark.parametrize("K,storage", [(4, 'float32'), (32, 'float64')])
def test_a_run_after_the_products_equals_a_fresh_batch(K, storage):
    """The product entries leave the batch's vectors and their zero padding as
    they found them: one Gibbs iteration afterwards is, bit for bit, that of
    a batch that made no such call."""
    from bayesbridge_amd import HipChainBatch
    from test_hip_batch import _chains, _dense_problem
    n, p = 641, 40
    X, y, hip = _dense_problem(n, p, storage=storage)
    rng = np.random.default_rng(4)
    V, W = rng.standard_normal((K, p + 1)), rng.standard_normal((K, n))
    OM = rng.gamma(2., .5, (K, n))
    used = HipChainBatch(_chains(hip, y, 'linear', list(range(K))),
                         allow_slow=True)
    V[K - 1, ::2], W[0, ::3] = np.nan, np.inf
    used.dot(V), used.Tdot(W), used.dot(V, OM, return_twt=True)
    used.dot(V, None, return_twt=True)
    s_used, u_used = used.run(1)
    fresh = HipChainBatch(_chains(hip, y, 'linear', list(range(K))),
                          allow_slow=True)
    s_fresh, u_fresh = fresh.run(1)
    assert u_used == u_fresh == 0
    for key in ('coef', 'global_scale', 'logp', 'n_cg_iter'):
        assert np.array_equal(s_used[key], s_fresh[key]), key
    assert np.all(np.isfinite(s_used['coef']))


# ---- e. the entry on a tiled sparse batch, and its refusals -----------------
def test_the_scaled_entry_on_a_tiled_sparse_batch():
    from bayesbridge_amd import HipChainBatch, _lib
    from test_hip_batch import _chains, _problem
    K = 2
    X, y, hip = _problem(6000, 3000, 'linear')
    batch = HipChainBatch(_chains(hip, y, 'linear', [0, 1]), allow_slow=True)
    n, P = hip.shape
    rng = np.random.default_rng(6)
    v, om = rng.standard_normal((K, P)), rng.gamma(2., .5, (K, n))
    off = np.asarray(X.mean(axis=0)).ravel()
    out, part, twt = batch.dot(v, om, return_twt=True)
    plain, part1, twt1 = batch.dot(v, None, return_twt=True)
    assert part.shape == (K, dbo.NPART)
    for c in range(K):
        ref = v[c, 0] + X @ v[c, 1:] - off @ v[c, 1:]
        tol = 1e-11 * np.abs(ref).max()
        assert np.abs(plain[c] - ref).max() <= tol
        assert np.abs(out[c] - om[c] * ref).max() <= tol * om[c].max()
        for got, want in ((twt[c], om[c] @ (ref * ref)),
                          (twt1[c], ref @ ref)):
            assert abs(got - want) <= 1e-11 * want
    assert np.array_equal(batch.dot(v), plain)
    # refusals: status codes, never a crash
    lib = _lib.load()
    err_invalid = -1

    def p(a):
        return None if a is None else a.ctypes.data_as(c_void_p)
    o, t = np.empty((K, n)), np.empty((K, dbo.NPART))
    assert lib.bbx_batch_dot_scaled(None, p(v), p(om), p(o), p(t)) == err_invalid
    assert 'NULL' in _lib.last_error()
    assert lib.bbx_batch_dot_scaled(batch._b, None, p(om), p(o), p(t)) == err_invalid
    assert lib.bbx_batch_dot_scaled(batch._b, p(v), p(om), None, p(t)) == err_invalid
    assert lib.bbx_batch_dot_scaled(batch._b, p(v), p(om), p(o), None) == err_invalid
    assert lib.bbx_batch_dot_scaled(batch._b, p(v), None, p(o), p(t)) == 0
    assert np.array_equal(o, plain) and np.array_equal(t, part1)
    with pytest.raises(ValueError):
        batch.dot(v[:, :-1], om)
    with pytest.raises(ValueError):
        batch.dot(v, om[:, :-1])
    with pytest.raises(ValueError):
        batch.dot(v, om[:1], return_twt=True)
