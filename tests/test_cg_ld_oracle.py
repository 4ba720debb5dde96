"""CPU: the host side of the CG edge tests (cg_ld_oracle.py) checked on its
own -- the float64 replay against the project's oracle (oracle.cg_sample), the
tolerance constants against the measured float64-vs-long-double levels of
every case in both summation orders, every planted fault against the
tolerance it must miss by a factor of 1000, the integer cases against Python
integers and against the long-double products, and the kernel geometry the
widths are derived from against the text of the sources."""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sparse

import cg_ld_oracle as clo
import oracle
from conftest import ROOT

CSRC = os.path.join(ROOT, "bayes-bridge_amd", "csrc")
ALL_CASES = clo.TRUNC_CASES + clo.EXTRA_CASES


@pytest.fixture(scope='module', autouse=True)
def _release_after_the_module():
    yield
    clo.release()
    _level.cache_clear()


def test_widths_sit_at_the_edges_of_the_kernels():
    with open(os.path.join(CSRC, "common.hpp")) as f:
        common = f.read()
    npart = int(re.search(r"NPART\s*=\s*(\d+)", common).group(1))
    block = int(re.search(r"VEC_BLOCK\s*=\s*(\d+)", common).group(1))
    wave = int(re.search(r"\bWAVE\s*=\s*(\d+)", common).group(1))
    assert npart * block == clo.TRIP
    assert clo.P_WAVE == (wave - 1, wave, wave + 1)
    assert clo.P_BLOCK == (block - 1, block, block + 1)
    assert clo.P_TRIP == (clo.TRIP - 1, clo.TRIP, clo.TRIP + 1)
    assert clo.P_THIRD == (2 * clo.TRIP + 1,)
    with open(os.path.join(CSRC, "tiled_layout.hpp")) as f:
        tiled = f.read()
    assert int(re.search(r"define BBX_TILE_THREADS\s+(\d+)",
                         tiled).group(1)) == clo.FOLD_THREADS
    got = {cs.P for cs in clo.TRUNC_CASES}
    assert got == set(clo.P_ALL)
    assert {cs.nu for cs in clo.TRUNC_CASES} >= {0, 1, 2}
    assert any(cs.nu == cs.P for cs in clo.TRUNC_CASES)
    for group in (clo.P_SMALLEST, clo.P_WAVE, clo.P_BLOCK, clo.P_TRIP,
                  clo.P_PAST + clo.P_THIRD):
        assert {cs.warm for cs in clo.TRUNC_CASES if cs.P in group} \
            == {True, False}


@pytest.mark.parametrize("P", [65537, 65601, 131073])
def test_designs_have_an_empty_column_on_each_side_of_the_first_trip(P):
    c = clo.design(P)
    per_col = np.bincount(c.cols, minlength=c.p)
    coord = np.flatnonzero(per_col == 0) + 1
    # (P = 65 537 ends at coordinate 65 536: one empty column, below it)
    assert list(coord) == [j for j in (clo.TRIP - 1, clo.TRIP + 1) if j < P - 1]
    assert len(coord) == (2 if P > clo.TRIP + 2 else 1)
    assert per_col[clo.TRIP - 1] >= 2                # coordinate 65 536 itself
    assert per_col.max() <= 4 and c.n == 256
    # distinct rows inside a column, ascending columns inside a row
    A = sparse.csr_matrix((np.ones(c.rows.size), c.indices, c.indptr),
                          shape=(c.n, c.p))
    assert A.has_canonical_format and A.max() == 1.
    assert np.array_equal(c.offset, np.asarray(A.mean(axis=0)).ravel())


SMALL = [cs for cs in ALL_CASES if cs.P <= 260 and cs.kind != 'dense']


@pytest.mark.parametrize("cs", SMALL, ids=lambda cs: cs.name)
def test_float64_replay_agrees_with_the_project_oracle(cs):
    """Same n_iter; coefficients within the oracle's own rounding: the two are
    float64 statements of one recurrence that differ in summation order, so
    they may differ by what the two orders of the replay differ by -- after 1
    and 2 iterations TRUNC_TOL, at convergence the criterion of
    test_hip_cg_sampler.py."""
    c, inp = clo.design_of(cs), clo.inputs(cs)
    ora = clo.oracle_design(c)
    v = np.random.default_rng(1).normal(size=c.P)
    assert np.allclose(ora.dot(v), clo.dot(c, v, np.float64), 1e-13, 1e-13)
    atol = 1e-5 * np.sqrt(c.P)
    for maxiter in clo.trunc_iters(cs) + (500,):
        co, io = oracle.cg_sample(
            ora, inp['obs_prec'], inp['prior_prec_sqrt'], inp['z'],
            inp['coef_cg_init'], inp['coef_scaled_sd'], cs.nu, inp['randn_n'],
            inp['randn_P'], maxiter, atol if maxiter == 500 else 0.)
        cr, n_iter, conv = clo.replay(c, inp, cs.nu, maxiter,
                                      atol if maxiter == 500 else 0.,
                                      np.float64)
        assert n_iter == io['n_iter'] and conv == io['converged']
        assert conv == (maxiter == 500)
        tol = clo.TRUNC_TOL[maxiter] if maxiter <= 2 else 1e-6
        assert clo.rel_err(cr, co) <= tol, (maxiter, clo.rel_err(cr, co))


@functools.lru_cache(maxsize=None)
def _level(name, k, order):
    """float64 replay against the long-double one: the measured rounding."""
    cs = clo.CASES_BY_NAME[name]
    ref, n_iter, conv = clo.reference(cs, k)
    assert n_iter == k and not conv
    co, n64, c64 = clo.replay(clo.design_of(cs), clo.inputs(cs), cs.nu, k, 0.,
                              np.float64, order)
    assert n64 == k and not c64
    return clo.rel_err(co, ref)


@pytest.mark.parametrize("cs", ALL_CASES, ids=lambda cs: cs.name)
def test_float64_replay_is_within_the_constants(cs):
    """Every case and order within TRUNC_TOL[k] / MARGIN = MEASURED[k]."""
    for k in clo.trunc_iters(cs):
        for order in ('natural', 'reversed'):
            err = _level(cs.name, k, order)
            print("%s k = %d %s: float64 vs long double %.3g (constant %.3g)"
                  % (cs.name, k, order, err, clo.MEASURED[k]))
            assert err <= clo.TRUNC_TOL[k] / clo.MARGIN
    assert clo.TRUNC_TOL[1] == 32 * clo.MEASURED[1]
    assert clo.TRUNC_TOL[2] == 32 * clo.MEASURED[2]


def test_constants_are_the_measured_levels_not_more():
    """The largest measured level is within a factor 2 of each constant: the
    constants are measurements, not allowances."""
    for k in (1, 2):
        worst = max(_level(cs.name, k, order) for cs in ALL_CASES
                    for order in ('natural', 'reversed')
                    if k in clo.trunc_iters(cs))
        print("k = %d: largest float64-vs-long-double level %.3g, "
              "TRUNC_TOL %.3g" % (k, worst, clo.TRUNC_TOL[k]))
        assert clo.MEASURED[k] / 2 <= worst <= clo.MEASURED[k]


_sharp = []


@pytest.mark.parametrize("cs", [cs for cs in ALL_CASES if cs.P > 1],
                         ids=lambda cs: cs.name)
def test_planted_faults_miss_the_tolerance_by_a_factor_of_1000(cs):
    c, inp = clo.design_of(cs), clo.inputs(cs)
    ref, _, _ = clo.reference(cs, 2)
    j, shift = clo.fault_coordinate(cs.P)
    assert j >= clo.TRIP or j == cs.P - 1
    for fault in clo.FAULTS:
        if not clo.fault_applies(fault, cs.P):
            continue
        co, n_iter, _ = clo.replay(c, inp, cs.nu, 2, 0., np.float64,
                                   'natural', fault)
        ratio = clo.rel_err(co, ref) / clo.TRUNC_TOL[2]
        _sharp.append(ratio)
        print("%s %s: error / TRUNC_TOL[2] = %.3g" % (cs.name, fault, ratio))
        assert n_iter == 2
        assert ratio >= clo.FAULT_SHARPNESS, (fault, ratio)
    print("smallest planted-fault / tolerance ratio so far: %.3g"
          % min(_sharp))


def test_a_fault_touches_one_coordinate_of_the_first_iteration_only():
    """The faults are what they say: after ONE iteration 'r_prev_alpha',
    'sr_stale', 'pdp_missing' have changed nothing but through coordinate j,
    and the others nothing at all (they act from the second iteration on)."""
    cs = clo.CASES_BY_NAME['binary-P65601-nu1-warm']
    c, inp = clo.design_of(cs), clo.inputs(cs)
    base, _, _ = clo.replay(c, inp, cs.nu, 1, 0., np.float64)
    for fault in ('x_stale', 'beta_dropped', 'read_shifted', 'sr_stale',
                  'r_prev_alpha'):
        co, _, _ = clo.replay(c, inp, cs.nu, 1, 0., np.float64, 'natural',
                              fault)
        assert np.array_equal(co, base), fault
    co, _, _ = clo.replay(c, inp, cs.nu, 1, 0., np.float64, 'natural',
                          'pdp_missing')
    assert not np.array_equal(co, base)


@pytest.mark.parametrize("P,intercept", [(1, False), (2, True), (3, True),
                                         (3, False), (65, True), (257, True)])
def test_integer_cases_equal_python_integers(P, intercept):
    ic = clo.int_case(P, intercept)
    c = ic.design
    n, i0 = c.n, int(intercept)
    X = [[0] * c.p for _ in range(n)]
    for r, j in zip(c.rows, c.cols):
        X[int(r)][int(j)] += 1
    off = [Fraction(sum(X[i][j] for i in range(n)), n) for j in range(c.p)]
    Xt = [[Fraction(1)] * i0 + [X[i][j] - off[j] for j in range(c.p)]
          for i in range(n)]
    v, w, om = ([int(a) for a in x] for x in (ic.v, ic.w, ic.omega))
    t = [sum(Xt[i][j] * v[j] for j in range(P)) for i in range(n)]
    g = [sum(Xt[i][j] * w[i] for i in range(n)) for j in range(P)]
    op = [sum(Xt[i][j] * om[i] * t[i] for i in range(n)) for j in range(P)]
    for got, want in ((ic.t, t), (ic.g, g), (ic.op, op)):
        assert [Fraction(float(a)) for a in got] == want


@pytest.mark.parametrize("P", clo.P_ALL)
def test_integer_cases_hold_the_exactness_bound(P):
    """2^53 (asserted inside int_case too), and float64 products in both
    orders and the long-double ones return the int64 results bit for bit."""
    ic = clo.int_case(P, P > 1)
    assert ic.abs_max < 2 ** 53
    c = ic.design
    for dtype in (np.float64, clo.LD):
        for rev in (False, True):
            t = clo.dot(c, ic.v, dtype, rev)
            assert np.array_equal(t, ic.t)
            assert np.array_equal(clo.tdot(c, ic.w, dtype, rev), ic.g)
            assert np.array_equal(clo.tdot(c, ic.omega * t, dtype, rev), ic.op)
    assert np.any(ic.t != np.round(ic.t)) or P == 1     # centring is in there
