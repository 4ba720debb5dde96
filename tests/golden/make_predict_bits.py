"""Writes tests/golden/predict_parent_bits.npz: what model.predict of the
linear, logit, Poisson, negative-binomial and ordinal models returned on an
MI355X in the build of the commit BEFORE the two summary kernels
(predict_summary_kernel, ordinal_summary_kernel) and their two host drivers
were folded onto the accumulators and the pass driver of
csrc/predict_summary.hpp.  tests/test_hip_predict_bits.py imports `cases` and
`compute` and compares bit for bit.

    python tests/golden/make_predict_bits.py OUT.npz     (needs a GPU)

To write the fixture again, run this file from this tree with the package of
the parent commit's build first on PYTHONPATH: the row counts come from this
tree's header (the parent had the same PRED_BLOCK and PRED_DRAWS).

Every model is trained on N_TRAIN seeded rows of a dense float64 design with 5
columns and predicts n new rows, so that every optional argument is the
case's own.  A case is (variant, n, S, outcome, draws, draws_per_pass).  The
results do not depend on draws_per_pass -- that is the kernels' contract, and
`main` refuses to write a fixture of a build that breaks it -- so the fixture
holds one array per (variant, n, S, outcome, draws), the results one after
the other (`pack`), and every draws_per_pass of {0, 1, 2, S} is compared with
it.

The cross of variants, rows, draws and pass sizes in full would be ten times
the size a fixture may have.  What is crossed with what:
  * the five PRIMARY variants (every family once, with its optional row
    vector) take every row count and every number of draws: n = 1 with every S;
    PRED_BLOCK - 1 with S = 2 and, without an outcome, with S = 5;
    PRED_BLOCK + 1 with S = 5; 2 PRED_BLOCK + 3 with
    S = PRED_DRAWS + 1 (two passes at the default, seventeen at one draw per
    pass); and the training rows themselves (X_new=None);
  * the other variants (no n_trial, no exposure, no offset, K = 2, K = 16)
    change nothing in how a thread finds its row or its draw: PRED_BLOCK - 1
    rows (K = 16: PRED_BLOCK + 1) with S = 5 and an outcome, and one row with
    S = 1 and none;
  * return_draws (the four scalar families): PRED_BLOCK + 1 rows, S = 5;
  * the non-finite paths, which are a row's own arithmetic, on 4 rows, S = 5."""
import functools
import os
import re
import sys
import warnings

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..',
                    'bayes-bridge_amd', 'csrc')
N_TRAIN = 24
PRIMARY = ('linear', 'logit_m', 'poisson_e', 'negbin_e', 'ordinal3_o')
OTHERS = ('logit', 'poisson', 'negbin', 'ordinal3', 'ordinal2_o', 'ordinal2',
          'ordinal16_o', 'ordinal16')
VARIANTS = PRIMARY + OTHERS
# (variant, the non-finite path): see _nonfinite
NONFINITE = (('poisson_e', 'overflow'), ('negbin_e', 'overflow'),
             ('ordinal3_o', 'overflow')) + tuple((v, 'nan') for v in PRIMARY)
ARRAYS = ('mean', 'sd', 'lpd', 'loglik_mean', 'loglik_var', 'lppd', 'p_waic',
          'waic', 'draws')


def _constant(name):
    text = open(os.path.join(CSRC, 'predict_summary.hpp')).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))


def rows():
    """The row counts, from the header: one row per thread, PRED_BLOCK
    threads per workgroup."""
    block = _constant('PRED_BLOCK')
    return (1, block - 1, block + 1, 2 * block + 3)


def n_draws():
    return (1, 2, 5, _constant('PRED_DRAWS') + 1)


def _family(variant):
    return re.match('[a-z]+', variant).group(0)


def _n_category(variant):
    """K of an ordinal variant; 0 for the others."""
    digits = re.search(r'\d+', variant)
    return int(digits.group(0)) if digits else 0


def _with_vector(variant):
    """Whether the variant has its optional row vector: n_trial, exposure or
    offset."""
    return '_' in variant


def cases():
    """Every (variant, n, S, outcome, draws, draws_per_pass); n = 0 stands
    for the training rows, n < 0 for the -n rows of a non-finite path."""
    n1, below, above, two = rows()
    s1, s2, s5, s17 = n_draws()
    cells = []
    for v in PRIMARY:
        cells += [(v, n1, S, S > 1, False) for S in n_draws()]
        cells += [(v, below, s2, True, False), (v, below, s5, False, False),
                  (v, above, s5, True, False), (v, two, s17, True, False),
                  (v, 0, s5, True, False)]
    for v in OTHERS:
        n = above if _n_category(v) == 16 else below
        # (K = 16 without an offset goes without an outcome too)
        cells += [(v, n, s5, v != 'ordinal16', False),
                  (v, n1, s1, False, False)]
    cells += [(v, above, s5, True, True) for v in PRIMARY
              if _family(v) != 'ordinal']
    cells += [(v + ':' + path, -4, s5, True, False) for v, path in NONFINITE]
    return [cell + (per,) for cell in cells
            for per in sorted({0, 1, 2, cell[2]})]


def name(case):
    """The case's key in the fixture (draws_per_pass is not part of it)."""
    variant, n, S, outcome, draws, _ = case
    return '%s_n%d_S%d_%s%s' % (variant.replace(':', '_'), abs(n), S,
                                'y' if outcome else 'x', 'd' if draws else '')


@functools.lru_cache(maxsize=None)
def _model(variant):
    """The variant's model on N_TRAIN seeded rows."""
    from bayesbridge_amd import HipDenseDesignMatrix, RegressionModel
    family = _family(variant)
    rng = np.random.default_rng([VARIANTS.index(variant), 0])
    ordinal = family == 'ordinal'
    X = rng.normal(size=(N_TRAIN, 5 if ordinal else 4))
    dsn = HipDenseDesignMatrix(X, add_intercept=not ordinal,
                               center_predictor=True, storage_dtype='float64')
    assert dsn.shape == (N_TRAIN, 5)
    outcome = _outcome(variant, N_TRAIN, rng)
    outcome = outcome if outcome[1] is not None else outcome[0]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if family == 'negbin':
            return RegressionModel(outcome, dsn, family, dispersion=2.)
        return RegressionModel(outcome, dsn, family)


def _outcome(variant, n, rng):
    """(y, the optional row vector or None) of n rows."""
    family = _family(variant)
    vector = None
    if family == 'linear':
        y = rng.normal(size=n)
    elif family == 'logit':
        m = rng.integers(1, 6, n) if _with_vector(variant) else np.ones(n, int)
        y = rng.binomial(m, .4).astype(np.float64)
        vector = m.astype(np.float64) if _with_vector(variant) else None
    elif family in ('poisson', 'negbin'):
        y = rng.poisson(2., n).astype(np.float64)
        vector = rng.uniform(.5, 2., n) if _with_vector(variant) else None
    else:
        K = _n_category(variant)
        # (a training outcome needs every category)
        y = rng.permutation(np.arange(n) % K).astype(np.float64)
        vector = rng.normal(size=n) * .3 if _with_vector(variant) else None
    return y, vector


def _nonfinite(variant, path, X, coef, y):
    """The non-finite paths, in place.  'overflow': row 0 overflows in draw 2
    of 5 and row 1 in every draw -- a Poisson mean of +inf that sticks and a
    log-likelihood of -inf in one draw and in all of them; the ordinal model's
    eta = +inf with an outcome below the top category, the same.  (The
    negative binomial's log-likelihood stays finite there: only its mean
    overflows.)  'nan': one coefficient of draw 1 is a NaN."""
    if path == 'nan':
        coef[3, 1] = np.nan
        return
    big = 1e200 if _family(variant) == 'ordinal' else 800.
    X[0, 0], X[1, 1] = big, big
    one = 1e200 if _family(variant) == 'ordinal' else 1.
    j = 0 if _family(variant) == 'ordinal' else 1    # (past the intercept)
    coef[j] = 0.
    coef[j, 2] = one
    coef[j + 1] = one
    y[:2] = 0.


def compute(case):
    """{name: float64 array} of model.predict in one case."""
    variant, n, S, outcome, draws, per = case
    variant, _, path = variant.partition(':')
    family = _family(variant)
    model = _model(variant)
    rng = np.random.default_rng([VARIANTS.index(variant), abs(n), S])
    coef = rng.normal(size=(5, S)) * .3
    kw = {}
    if family == 'linear':
        kw['obs_prec'] = rng.uniform(.5, 2., S)
    if family == 'ordinal':
        K = _n_category(variant)
        args = (np.sort(rng.normal(size=(K - 1, S)) * 2., axis=0),)
    else:
        args = (rng.uniform(.5, 5., S),) if family == 'negbin' else ()
        kw['return_draws'] = draws
    if n != 0:
        kw['X_new'] = rng.normal(size=(abs(n), 5 - int(family != 'ordinal')))
        y, vector = _outcome(variant, abs(n), rng)
        if path:
            _nonfinite(variant, path, kw['X_new'], coef, y)
        if outcome:
            kw['y_new'] = y
        if vector is not None and (outcome or family != 'logit'):
            kw[{'logit': 'n_trial_new', 'ordinal': 'offset_new'}.get(
                family, 'exposure_new')] = vector
    res = model.predict(coef, *args, _draws_per_pass=per, **kw)
    assert set(res) <= set(ARRAYS), sorted(res)
    assert ('lpd' in res) == outcome and ('draws' in res) == draws
    return {key: np.ascontiguousarray(val, dtype=np.float64).reshape(-1)
            for key, val in res.items()}


def pack(res):
    """The results of a case as one array, in the order of ARRAYS."""
    return np.concatenate([res[key] for key in ARRAYS if key in res])


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64),
                                                 b.view(np.uint64))


def main(path):
    out, packed = {}, {}
    for case in cases():
        res = compute(case)
        for key, val in res.items():
            full = name(case) + '_' + key
            assert same_bits(out.setdefault(full, val), val), (case, key)
        packed[name(case)] = pack(res)
    np.savez_compressed(path, **packed)
    print('wrote', path, len(cases()), 'cases', len(packed), 'arrays',
          sum(v.size for v in packed.values()), 'doubles',
          os.path.getsize(path), 'bytes')
    # the non-finite paths are the ones meant
    cell = 'poisson_e_overflow_n4_S5_y_'
    assert np.all(out[cell + 'mean'][:2] == np.inf), out[cell + 'mean']
    assert np.isfinite(out[cell + 'lpd'][0]) \
        and out[cell + 'lpd'][1] == -np.inf, out[cell + 'lpd']
    assert np.all(out[cell + 'loglik_mean'][:2] == -np.inf)
    assert np.all(np.isfinite(out[cell + 'lpd'][2:]))
    assert np.all(out['negbin_e_overflow_n4_S5_y_mean'][:2] == np.inf)
    cell = 'ordinal3_o_overflow_n4_S5_y_'
    assert np.isfinite(out[cell + 'lpd'][0]) \
        and out[cell + 'lpd'][1] == -np.inf, out[cell + 'lpd']
    for v in PRIMARY:
        for key in ARRAYS[:5]:
            assert np.all(np.isnan(out['%s_nan_n4_S5_y_%s' % (v, key)])), v
    print('the non-finite cases hold what they are meant to')


if __name__ == "__main__":
    main(sys.argv[1])
