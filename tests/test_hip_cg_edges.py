"""GPU: the conjugate-gradient draw (csrc/cg_sampler.hip) at the edges of its
P-vector kernels, against the long-double replay of cg_ld_oracle.py.

Every P-length kernel of a solve -- cg_setup, prep_v, cg_direction, cg_update,
cg_finish (csrc/vecops.hip), the Tdot finalize with its three epilogues
(csrc/spmv_csr.hip), the folded direction step (csrc/spmv_tiled.hip) -- keeps a
thread's first coordinate in registers and loads every further one inside a
loop; with 65 536 threads those loops start at P = 65 537.  The widths here
(cg_ld_oracle.P_ALL) lie around a wave, a block, that first trip and the
third; the same cases run on every solve path, and each design asserts from
tiled_info(), hybrid_info, cg_launches or its shape that it IS on the path it
names:

  csr       reference layout: cg_update_kernel, chunk-pointer arm of the
            finalize (5 launches per iteration: direction, X~ v, X~^T w,
            finalize, update)
  tiled     one column group, fold off: update in the Tdot epilogue (4)
  fold      the same with the direction step in the X~ v kernel (3), ONE
            workgroup: its share is all P coordinates, 65 trips at 65 601
            (the builder's own choice at 256 rows is two 128-row panels, so
            the panel height is set to 256)
  foldmany  20 000 rows in 128-row panels: 157 workgroups, whose shares
            ceil(P / 157) are ragged at 65 601 and empty for most at 2, 3, 157
  groups    several column groups (the builder's choice past 16 128
            columns): dot finalize plus separate update (5)
  valued    Gaussian values (plain ids, no fold, 4)
  mixed     three full Gaussian columns in the dot epilogue (launch_tdot_hybrid)
  slabNN    X^T in NN column groups: the 16 + 8 + 1 slab loop of the finalize
  dense     257 x 65 537, f32 and f64 storage: two-kernel operator, 64 chunks

Tolerances: cg_ld_oracle.TRUNC_TOL for solves cut at 1 and 2 iterations (the
measured float64-vs-long-double level times 32, see there; planted faults of
one coordinate miss it by a factor of 1000 and more), test_hip_cg_sampler's
criteria for converged solves, equality for the integer operator cases and
for the solve that stops at its first test."""
import warnings

import numpy as np
import pytest

import cg_ld_oracle as clo
import oracle

pytestmark = pytest.mark.gpu

_KNOBS = ('BBX_TILED_PR', 'BBX_TILED_PR_T', 'BBX_TILED_G', 'BBX_TILED_G_T',
          'BBX_TILED_BLOCKS', 'BBX_TILED_BLOCKS_T', 'BBX_TILED_PACK')
SLAB_GROUPS = (15, 16, 17, 24, 25)     # around the 16 pre-loaded and 16 + 8
SLAB_P = (257, 65537)
TILE_W_MAX = 16128                     # columns of one slice of X

# path -> (storage, environment around the constructor, fold)
PATHS = {
    'csr': ('csr', {}, None),
    'tiled': ('tiled', {'BBX_TILED_G': '1'}, False),
    'fold': ('tiled', {'BBX_TILED_G': '1', 'BBX_TILED_PR': '256'}, True),
    'foldmany': ('tiled', {'BBX_TILED_G': '1', 'BBX_TILED_PR': '128'}, True),
    'groups': ('tiled', {}, None),
    'valued': ('tiled', {'BBX_TILED_G': '1'}, None),
    'mixed': ('tiled', {}, None),
}
for _g in SLAB_GROUPS:
    PATHS['slab%d' % _g] = ('tiled', {'BBX_TILED_G': '1',
                                      'BBX_TILED_G_T': str(_g),
                                      'BBX_TILED_BLOCKS_T': str(_g)}, False)

_built = {}


@pytest.fixture(scope='module', autouse=True)
def _release_after_the_module():
    """The device designs and the host cases are shared by the tests of this
    file and freed after the last of them."""
    yield
    _built.clear()
    clo.release()


def _design(path, c):
    """The device design of `c` on `path`, built once, path asserted."""
    key = (path, c.kind, c.n, c.P, c.intercept)
    if key in _built:
        return _built[key]
    from bayesbridge_amd import HipDenseDesignMatrix, HipSparseDesignMatrix
    if c.kind == 'dense':
        storage = {'dense-f32': 'float32', 'dense-f64': 'float64'}[path]
        hip = HipDenseDesignMatrix(c.X, center_predictor=False,
                                   add_intercept=c.intercept,
                                   storage_dtype=storage)
        assert hip.shape == (257, 65537) and hip.storage_dtype == storage
        assert hip.cg_launches == 5          # not the single-pass operator
        _built[key] = hip
        return hip
    storage, env, fold = PATHS[path]
    with pytest.MonkeyPatch.context() as mp:
        for k in _KNOBS:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        hip = HipSparseDesignMatrix.from_csr_arrays(
            (c.n, c.p), c.indptr, c.indices, data=c.vals,
            column_offset=c.offset, add_intercept=c.intercept, storage=storage)
    if fold is not None:
        hip.set_cg_fold(fold)
    assert hip.shape == (c.n, c.P) and hip.storage_format == storage
    info = hip.tiled_info() if storage == 'tiled' else None
    if path == 'csr':
        assert hip.cg_launches == 5 and hip.hybrid_info is None
    elif path == 'tiled':
        assert info['X']['G'] == 1 and hip.cg_launches == 4
    elif path == 'fold':
        assert info['X']['G'] == 1 and info['X']['grid'] == 1
        assert hip.cg_launches == 3
    elif path == 'foldmany':
        assert info['X']['G'] == 1 and 1 < info['X']['grid'] <= 256
        assert info['X']['grid'] == -(-c.n // 128)
        assert hip.cg_launches == 3
    elif path == 'groups':
        assert c.p > TILE_W_MAX and info['X']['G'] > 1
        assert hip.cg_launches == 5 and hip.hybrid_info is None
    elif path == 'valued':
        assert not info['X']['packed'] and not info['Xt']['packed']
        assert not hip.is_binary and hip.hybrid_info is None
        assert info['X']['G'] == 1 and hip.cg_launches == 4
    elif path == 'mixed':
        assert hip.hybrid_info is not None
        assert hip.hybrid_info['dense_cols'] == 3
        assert hip.hybrid_info['dense_nnz'] == 3 * c.n
    else:
        g = int(path[4:])
        assert info['Xt']['G'] == g and info['X']['G'] == 1
        assert hip.cg_launches == 4
    _built[key] = hip
    return hip


def paths_for(cs):
    """Every path that admits the case."""
    if cs.kind == 'dense':
        return ['dense-f32', 'dense-f64']
    if cs.kind in ('valued', 'mixed'):
        return ['csr', cs.kind]
    if cs.n != clo.N_ROWS:
        return ['csr', 'foldmany']
    out = ['csr', 'tiled', 'fold']
    if cs.P - int(cs.intercept) > TILE_W_MAX:
        out.append('groups')
    if cs.P in SLAB_P and cs.intercept:
        out += ['slab%d' % g for g in SLAB_GROUPS]
    return out


class _Replay:
    def __init__(self, vecs):
        self.vecs = list(vecs)

    def __call__(self, size):
        return self.vecs.pop(0)


def _draw(hip, inp, nu, maxiter, atol):
    """One draw through HipCGSampler with the case's normals planted in the
    global NumPy stream; (coef, info, (dots, Tdots) of this draw)."""
    from bayesbridge_amd import HipCGSampler
    hip.reset_matvec_count()
    orig = np.random.randn
    np.random.randn = _Replay([inp['randn_n'], inp['randn_P']])
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')    # cut solves stop at maxiter
            coef, info = HipCGSampler(nu).sample(
                hip, inp['obs_prec'], inp['prior_prec_sqrt'], inp['z'],
                coef_cg_init=inp['coef_cg_init'], precond_by='prior',
                coef_scaled_sd=inp['coef_scaled_sd'], maxiter=maxiter,
                atol=atol)
    finally:
        np.random.randn = orig
    return coef, info, hip.get_dot_count()


ALL_CASES = clo.TRUNC_CASES + clo.EXTRA_CASES
_ids = dict(ids=lambda cs: cs.name)


# ---- a. the operator, exact ------------------------------------------------------
@pytest.mark.parametrize("P,intercept", [(P, True) for P in clo.P_ALL if P > 1]
                         + [(P, False) for P in clo.P_ALL])
def test_operator_equals_the_int64_products(P, intercept):
    ic = clo.int_case(P, intercept)
    c = ic.design
    paths = ['csr', 'tiled']
    if c.p > TILE_W_MAX:
        paths.append('groups')
    if P in SLAB_P and intercept:
        paths += ['slab%d' % g for g in SLAB_GROUPS]
    for path in paths:
        hip = _design(path, c)
        assert np.array_equal(hip.dot(ic.v), ic.t), path
        assert np.array_equal(hip.Tdot(ic.w), ic.g), path
        hip.reset_matvec_count()
        op = hip.gram_matvec(ic.omega, ic.v)
        assert hip.get_dot_count() == (1, 1), path
        assert np.array_equal(op, ic.op), path
        assert np.array_equal(hip.gram_matvec(ic.omega, ic.v), op), path


# ---- b. stop at the first test ---------------------------------------------------
@pytest.mark.parametrize("cs", ALL_CASES, **_ids)
def test_solve_that_stops_at_its_first_test_returns_the_start(cs):
    """atol = 1e30: n_iter = 0, converged, coef = s .* (x0 ./ s) bit for bit;
    products that ran: X~ (s x0) of a warm start and the one X~^T pass of the
    initial residual.  The folded path takes this stop inside the X~ v
    kernel."""
    c = clo.design_of(cs)
    for path in paths_for(cs):
        hip = _design(path, c)
        for warm in (True, False):
            inp = clo.inputs(cs, warm)
            coef, info, counts = _draw(hip, inp, cs.nu, 5, 1e30)
            assert info == {'n_iter': 0, 'valid_input': True,
                            'converged': True}, (path, warm)
            s = np.empty(cs.P)
            s[:cs.nu] = 2. * inp['coef_scaled_sd'][:cs.nu]
            s[cs.nu:] = 1. / inp['prior_prec_sqrt'][cs.nu:]
            want = s * (inp['coef_cg_init'] / s)
            assert np.array_equal(coef, want), (path, warm)
            assert counts == ((1, 1) if warm else (0, 1)), (path, warm)
            if not warm:
                assert not coef.any()


# ---- c. truncated solves ---------------------------------------------------------
@pytest.mark.parametrize("cs", ALL_CASES, **_ids)
def test_truncated_solves_equal_the_long_double_replay(cs):
    c, inp = clo.design_of(cs), clo.inputs(cs)
    warm = int(cs.warm)
    for k in clo.trunc_iters(cs):
        ref, n_ref, conv_ref = clo.reference(cs, k)
        assert n_ref == k and not conv_ref
        scale = float(np.abs(ref).max())
        got = {}
        for path in paths_for(cs):
            hip = _design(path, c)
            coef, info, counts = _draw(hip, inp, cs.nu, k, 0.)
            err = clo.rel_err(coef, ref)
            print("%s %s k = %d: device vs long double %.3g = %.3g of "
                  "TRUNC_TOL" % (cs.name, path, k, err, err / clo.TRUNC_TOL[k]))
            assert info == {'n_iter': k, 'valid_input': True,
                            'converged': False}, (path, k)
            assert counts == (k + warm, k + 1), (path, k)
            # every coordinate, none left out
            assert coef.shape == (cs.P,) and np.all(np.isfinite(coef))
            assert err <= clo.TRUNC_TOL[k], (path, k, err,
                                             int(np.abs(coef - ref).argmax()))
            again, info2, _ = _draw(hip, inp, cs.nu, k, 0.)
            assert np.array_equal(again, coef) and info2 == info, (path, k)
            got[path] = coef
        names = sorted(got)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                d = float(np.abs(got[a] - got[b]).max()) / scale
                assert d <= 2 * clo.TRUNC_TOL[k], (a, b, k, d)


# ---- d. converged solves ---------------------------------------------------------
@pytest.mark.parametrize("cs", ALL_CASES, **_ids)
def test_converged_solves_equal_the_long_double_replay(cs):
    """To atol = 1e-5 sqrt(P) under the criteria of test_hip_cg_sampler, and
    the residual of the returned draw, rebuilt with separate dot / Tdot calls
    (test_long_solves_meet_atol_on_the_recomputed_residual), within 3 atol."""
    from test_hip_cg_sampler import _assert_close
    c, inp = clo.design_of(cs), clo.inputs(cs)
    atol = 1e-5 * np.sqrt(cs.P)
    ref, n_ref, conv_ref = clo.reference(cs, 500, atol)
    assert conv_ref
    ref = np.asarray(ref, dtype=np.float64)
    omega, phi, z = inp['obs_prec'], inp['prior_prec_sqrt'], inp['z']
    s = np.empty(cs.P)
    s[:cs.nu] = 2. * inp['coef_scaled_sd'][:cs.nu]
    s[cs.nu:] = 1. / phi[cs.nu:]
    for path in paths_for(cs):
        hip = _design(path, c)
        coef, info, counts = _draw(hip, inp, cs.nu, 500, atol)
        print("%s %s: n_iter %d (replay %d), max error %.3g"
              % (cs.name, path, info['n_iter'], n_ref,
                 np.abs(coef - ref).max()))
        _assert_close(coef, info, ref, {'converged': True, 'n_iter': n_ref})
        assert counts == (info['n_iter'] + int(cs.warm), info['n_iter'] + 1)
        b = z + hip.Tdot(np.sqrt(omega) * inp['randn_n']) \
            + phi * inp['randn_P']
        resid = s * (b - (hip.Tdot(omega * hip.dot(coef)) + phi ** 2 * coef))
        worst = float(np.linalg.norm(resid)) / atol
        assert worst <= 3., (path, worst)


# ---- e. non-finite input ---------------------------------------------------------
@pytest.mark.parametrize("path", ['tiled', 'fold'])
def test_nan_in_z_past_the_first_trip_is_reported(path):
    """The flag comes from the direction kernel on the 4-launch path and from
    the X~ v kernel on the folded one; the design stays usable."""
    from bayesbridge_amd import BbxError
    cs = clo.CASES_BY_NAME['binary-P65601-nu1-warm']
    c, inp = clo.design_of(cs), clo.inputs(cs)
    hip = _design(path, c)
    bad = dict(inp)
    bad['z'] = np.array(inp['z'])
    bad['z'][clo.TRIP] = np.nan
    with pytest.raises(BbxError, match='non-finite residual inside CG'):
        _draw(hip, bad, cs.nu, 5, 1e-5 * np.sqrt(cs.P))
    ref, _, _ = clo.reference(cs, 1)
    coef, info, _ = _draw(hip, inp, cs.nu, 1, 0.)
    assert info['n_iter'] == 1 and info['valid_input']
    assert clo.rel_err(coef, ref) <= clo.TRUNC_TOL[1]


# ---- f. one Gibbs iteration at P = 65 601 ------------------------------------------
ALPHA, SLAB = .5, 2.
# Prior sd of the intercept.  test_hip_chain_pin.py uses 2 on 3 000 rows; on
# these 256 rows that leaves the intercept's direction of the preconditioned
# system so weakly determined that a CONVERGED solve is only good to 1e-5
# there whoever computes it: on the chain's own inputs of its second
# iteration the float64 oracle is 1.1e-5 from the long-double replay, and two
# device paths (csr, folded) 2.5e-6 from each other, while their solves cut at
# 1 and 2 iterations agree with long double to 0.01 of TRUNC_TOL.  With .2
# all of these agree to 6e-8, and the 1e-6 of the pin tests means something.
SD0 = .2


def _chain_problem():
    cs = clo.CASES_BY_NAME['binary-P65601-nu1-warm']
    c = clo.design_of(cs)
    hip = _design('fold', c)
    ora_design = clo.oracle_design(c)
    rng = np.random.default_rng(8)
    beta = np.zeros(c.P)
    beta[1:40] = rng.normal(0., 1.5, 39)
    n_trial = np.ones(c.n)
    n_success = (rng.random(c.n) < 1. / (1. + np.exp(-ora_design.dot(beta)))
                 ).astype(np.float64)
    return c, hip, ora_design, (n_success, n_trial)


def _oracle_draw(ch, it, ora, n, P, outcome):
    """The oracle's CG draw from the chain's state before iteration `it`."""
    from oracle.summarizer import CoefSummarizer, regularized_prior_scale
    coef_b, obs_b, ls_b, g_b = ch.get_state()
    mean_b, square_b, n_avg = ch.get_summary()
    assert n_avg == it and ch.iteration == it
    summ = CoefSummarizer(P, 1, SLAB)
    summ.set_state({'mean': mean_b, 'square': square_b, 'n_averaged': n_avg})
    y_gauss = (outcome[0] - outcome[1] / 2) / obs_b
    z = ora.design.Tdot(obs_b * y_gauss)
    prior_sd = np.concatenate((ora.sd_unshrunk,
                               regularized_prior_scale(g_b, ls_b, SLAB)))
    phi = 1 / prior_sd
    x0 = summ.extrapolate_coef_condmean(g_b, ls_b)
    sd = summ.estimate_post_sd()
    eta1, eta2 = ch.eta(it)
    coef_o, info_o = oracle.cg_sample(ora.design, obs_b, phi, z, x0, sd, 1,
                                      eta1, eta2, 500, 10e-6 * np.sqrt(P))
    return coef_o, info_o, summ, g_b, ls_b


def _check_draw(coef_d, n_cg, coef_o, info_o):
    import math
    slack = max(2, math.ceil(.10 * info_o['n_iter']))
    assert abs(n_cg - info_o['n_iter']) <= slack, (n_cg, info_o['n_iter'])
    tol = 1e-6 if n_cg == info_o['n_iter'] else 1e-5
    err = np.abs(coef_d - coef_o).max()
    assert err <= tol * max(1., np.abs(coef_o).max()), (err, n_cg, info_o)


def test_one_chain_iteration_at_65601_equals_the_oracle_and_the_replay():
    """The chain's own P-length kernels (prior, summary, coefficient sums,
    local scales) on their second trip: two iterations (cold, then warm
    start) pinned as in test_hip_chain_pin.py."""
    from bayesbridge_amd.device_chain import HipGibbsChain
    from oracle.gibbs import OracleGibbs
    from test_hip_chain_pin import _check_draws_against_replay
    c, hip, ora_design, outcome = _chain_problem()
    n, P = c.n, c.P
    ora = OracleGibbs(outcome, ora_design, 'logit', bridge_exponent=ALPHA,
                      sd_for_intercept=SD0, regularizing_slab_size=SLAB,
                      gscale_shape=1.5, gscale_rate=.3)
    assert (ora.n, ora.P) == (n, P)
    chain = HipGibbsChain(hip, 'logit', outcome[0], n_trial=outcome[1],
                          sd_unshrunk=[SD0], bridge_exponent=ALPHA,
                          slab_size=SLAB, gscale_shape=1.5, gscale_rate=.3,
                          seed=17)
    rng = np.random.default_rng(5)
    chain.set_state(np.zeros(P), None, np.exp(rng.normal(0., 1., P - 1)), .07)
    chain.init_obs_prec()
    for it in range(2):
        coef_o, info_o, summ, g_b, ls_b = _oracle_draw(chain, it, ora, n, P,
                                                       outcome)
        kept, n_unconv = chain.run(1, save=('coef', 'local_scale',
                                            'obs_prec'))
        assert n_unconv == 0
        coef_d = kept['coef'][0]
        _check_draw(coef_d, int(kept['n_cg_iter'][0]), coef_o, info_o)
        summ.update(coef_d, g_b, ls_b)
        mean_a, square_a, n_avg_a = chain.get_summary()
        assert n_avg_a == it + 1
        assert np.abs(mean_a - summ.mean).max() <= 1e-12 * max(
            1., np.abs(summ.mean).max())
        assert np.abs(square_a - summ.square).max() <= 1e-12 * max(
            1., np.abs(summ.square).max())
        coef_a, obs_a, ls_a, g_a = chain.get_state()
        assert np.array_equal(coef_a, coef_d)
        assert np.array_equal(ls_a, kept['local_scale'][0])
        lp_o = ora.logp(coef_a, g_a, obs_a)
        lp_d = float(kept['logp'][0])
        assert abs(lp_d - lp_o) <= 1e-10 * abs(lp_o), (lp_d, lp_o)
        assert np.all(ls_a > 0) and np.all(np.isfinite(ls_a))
        _check_draws_against_replay('P = 65601 fold', 17, it, 'logit',
                                    ora.design, outcome, 1, ora.shape0,
                                    ora.rate0, coef_a, obs_a, ls_a, g_a)
    chain.close()


def test_one_step_of_a_two_chain_batch_at_65601_equals_the_oracle():
    """b_finalize_kernel (csrc/batch.hip) past its first trip: every column
    of one batch step against the oracle's draw, as test_hip_batch_pin.py."""
    from bayesbridge_amd import HipChainBatch
    from bayesbridge_amd.device_chain import HipGibbsChain
    from oracle.gibbs import OracleGibbs
    c, hip, ora_design, outcome = _chain_problem()
    n, P = c.n, c.P
    ora = OracleGibbs(outcome, ora_design, 'logit', bridge_exponent=ALPHA,
                      sd_for_intercept=SD0, regularizing_slab_size=SLAB)
    chains = []
    for k, gscale in enumerate((.02, .3)):
        ch = HipGibbsChain(hip, 'logit', outcome[0], n_trial=outcome[1],
                           sd_unshrunk=[SD0], bridge_exponent=ALPHA,
                           slab_size=SLAB, seed=300 + 7 * k)
        rng = np.random.default_rng(40 + k)
        ch.set_state(np.zeros(P), None, np.exp(rng.normal(0., 1., P - 1)),
                     gscale)
        ch.set_gscale_update(None)
        ch.init_obs_prec()
        chains.append(ch)
    batch = HipChainBatch(chains, allow_slow=True)
    draws = [_oracle_draw(ch, 0, ora, n, P, outcome) for ch in chains]
    kept, n_unconv = batch.run(1)
    assert n_unconv == 0 and batch.n_unconverged == [0, 0]
    n_cg = kept['n_cg_iter'][:, 0].astype(int)
    for k, (coef_o, info_o, summ, g_b, ls_b) in enumerate(draws):
        coef_d = kept['coef'][k, 0]
        _check_draw(coef_d, int(n_cg[k]), coef_o, info_o)
        summ.update(coef_d, g_b, ls_b)
        mean_a, square_a, n_avg_a = chains[k].get_summary()
        assert n_avg_a == 1
        assert np.abs(mean_a - summ.mean).max() <= 1e-12 * max(
            1., np.abs(summ.mean).max())
        assert np.abs(square_a - summ.square).max() <= 1e-12 * max(
            1., np.abs(summ.square).max())
        coef_a, obs_a, ls_a, g_a = chains[k].get_state()
        assert np.array_equal(coef_a, coef_d) and g_a == g_b
        lp_o = ora.logp(coef_a, g_a, obs_a)
        assert abs(kept['logp'][k, 0] - lp_o) <= 1e-10 * abs(lp_o)
    batch.close()
    for ch in chains:
        ch.close()
