"""Writes tests/golden/cand_sums_parent_bits.npz: what the candidate sums of
the three families with an auxiliary parameter -- the negative binomial's
dispersion sums, the Weibull model's shape sums and the ordinal model's
cutpoint sums -- computed on an MI355X in the build of the commit BEFORE their
three kernels, host drivers and C fronts were folded onto csrc/glm_rows.hpp's
candidate skeleton: one candidate with the coefficients given, then 3 and 8
candidates on the cached linear predictor, the last of the 8 being the one
candidate again, on a seeded dense float64 design with 5 columns, at the row
counts where the kernel changes path; and the Weibull overflow rule.
tests/test_hip_cand_sums_bits.py imports `compute` and compares bit for bit.

    python tests/golden/make_cand_sums_bits.py OUT.npz     (needs a GPU)

To write the fixture again, run this file from this tree with the package of
the parent commit's build first on PYTHONPATH: the row counts come from this
tree's headers (the parent had the same GLM_ROW_U, 4)."""
import os
import sys
import warnings
from ctypes import c_void_p

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_glm_rows_bits import rows  # noqa: E402,F401

FAMILIES = ('negbin', 'weibull', 'ordinal')
P = 5                    # columns of the design
N_CATEGORY = 4
CUTS = np.array([-1., .2, 1.3])
SEED = 1009              # (apart from make_glm_rows_bits.py's streams)


def _design(n, rng, intercept):
    """n seeded rows of 5 columns, the intercept among them or not."""
    from bayesbridge_amd import HipDenseDesignMatrix, design_matrix
    X = rng.normal(size=(n, P - 1 if intercept else P))
    # The design classes drop columns that are constant over the rows, as
    # hand-made intercepts, and every column of a single row is constant: the
    # filter is switched off while a one-row design is built, as in
    # make_glm_rows_bits.py.  (A single centred row is a row of zeros: the
    # intercept-free one-row design stays uncentred, as in
    # tests/test_hip_ordinal.py.)
    keep = design_matrix.remove_intercept_indicator
    if n == 1:
        design_matrix.remove_intercept_indicator = lambda X: X
    try:
        dsn = HipDenseDesignMatrix(X, add_intercept=intercept,
                                   center_predictor=intercept or n > 1,
                                   storage_dtype='float64')
    finally:
        design_matrix.remove_intercept_indicator = keep
    assert dsn.shape == (n, P)
    return X, dsn


def _ordinal_any_rows(y, dsn, o):
    """The device model on rows that do not hold every category (a single
    row): the C ABI takes them, the model's constructor does not
    (tests/test_hip_ordinal.py's _AnyRows)."""
    from bayesbridge_amd import OrdinalModel, cutpoints
    m = object.__new__(OrdinalModel)
    m.y, m.offset = y, o
    m.n_category, m.design, m.name = N_CATEGORY, dsn, 'ordinal'
    m.cutpoints_fixed = False
    m._cutpoints = CUTS.copy()
    m.cutpoint_prior = cutpoints.check_prior(None)
    m._ham_prefix, m._ordinal = 'bbx_ordinal_', c_void_p()
    m._location_serial = 0
    return m


def _model(family, n, rng, log_time_of_row=None):
    """(the family's device model on n seeded rows, its sums' method, the
    candidates of the three calls); log_time_of_row = (row, value) replaces
    one row's log time before the handle is made."""
    from bayesbridge_amd import RegressionModel
    X, dsn = _design(n, rng, intercept=family != 'ordinal')
    rate = np.exp(.2 + X[:, :P - 1].dot(rng.normal(size=P - 1) * .3))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if family == 'negbin':
            e = rng.uniform(.5, 2., n)
            y = rng.poisson(rate * e * rng.gamma(2., .5, n))
            model = RegressionModel((y.astype(np.float64), e), dsn, 'negbin',
                                    dispersion=2.)
            cand = (.7, np.array([.05, 3., 1e4]),
                    np.array([.01, .3, 1., 2.5, 40., 1e3, 1e6, .7]))
            return model, model.dispersion_loglik, cand
        if family == 'weibull':
            t = rng.exponential(size=n) / rate
            event = rng.uniform(size=n) < .7
            model = RegressionModel(
                (np.where(event, t, np.inf), np.where(event, np.inf, t)), dsn,
                'weibull', weibull_shape=1.5)
            if log_time_of_row:
                model.log_time[log_time_of_row[0]] = log_time_of_row[1]
            cand = (1.3, np.array([.4, 1., 2.5]),
                    np.array([.05, .5, .9, 1., 1.7, 3., 6., 1.3]))
            return model, model.shape_loglik, cand
        y = rng.permutation(np.arange(n) % N_CATEGORY).astype(np.float64)
        o = rng.normal(size=n) * .5
        if n >= N_CATEGORY:
            model = RegressionModel((y, o), dsn, 'ordinal', cutpoints=CUTS)
        else:
            model = _ordinal_any_rows(y, dsn, o)
        more = np.sort(CUTS + rng.normal(size=(10, N_CATEGORY - 1)) * .2,
                       axis=1)
        assert np.all(np.diff(more, axis=1) > 0)
        cand = (CUTS, more[:3], np.vstack([more[3:], CUTS[None, :]]))
        return model, model.cutpoint_loglik, cand


def compute(family, n):
    """{name: float64 array} of family's candidate sums on n rows: 'k1' one
    candidate at a seeded beta, 'k3' and 'k8' on the cached linear predictor;
    the last of the 8 is the one of 'k1'."""
    rng = np.random.default_rng([SEED, FAMILIES.index(family), n])
    model, sums, cand = _model(family, n, rng)
    beta = rng.normal(size=P) * .3
    assert len(cand[1]) == 3 and len(cand[2]) == 8
    assert np.array_equal(cand[2][-1], cand[0])
    return {'k1': np.array([sums(beta, cand[0])]), 'k3': sums(None, cand[1]),
            'k8': sums(None, cand[2])}


def compute_weibull_overflow(n):
    """The shape sums of a Weibull handle on n rows of which one has log t =
    300: with k = 3 its eta + k lt is past exp's range (709.78), with .8 and
    1.5 it is not."""
    rng = np.random.default_rng([SEED, len(FAMILIES), n])
    model, sums, _ = _model('weibull', n, rng, log_time_of_row=(n // 3, 300.))
    return sums(rng.normal(size=P) * .3, np.array([.8, 3., 1.5]))


if __name__ == "__main__":
    out = {}
    for family in FAMILIES:
        for n in rows():
            for key, val in compute(family, n).items():
                assert np.all(np.isfinite(val)), (family, n, key, val)
                out['%s_%d_%s' % (family, n, key)] = val
    over = compute_weibull_overflow(rows()[2])
    assert over[1] == -np.inf and np.isfinite(over[[0, 2]]).all(), over
    out['weibull_overflow'] = over
    np.savez(sys.argv[1], **out)
    print('wrote', sys.argv[1], len(out), 'arrays',
          sum(v.size for v in out.values()), 'doubles')
