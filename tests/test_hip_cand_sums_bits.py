"""GPU: the candidate sums of the three families with an auxiliary parameter
(glm_cand_kernel of csrc/glm_rows.hpp with the policies of csrc/negbin.hip,
weibull.hip and ordinal.hip) against the bits that the build of the commit
before the fold onto one kernel skeleton, one host driver and one C front
produced on an MI355X (tests/golden/cand_sums_parent_bits.npz, written by
tests/golden/make_cand_sums_bits.py): one candidate with the coefficients
given, then 3 and 8 candidates on the cached linear predictor, at the row
counts where the kernel changes path, and the Weibull overflow rule."""
import os

import numpy as np
import pytest

from test_hip_poisson import LAP, VEC_BLOCK, _constant

pytestmark = pytest.mark.gpu

U = _constant('GLM_ROW_U', 'glm_rows.hpp')
ROWS = (1, VEC_BLOCK - 1, VEC_BLOCK + 1, LAP + 1, U * LAP + 3)


@pytest.fixture(scope='module')
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, 'cand_sums_parent_bits.npz'))


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64),
                                                 b.view(np.uint64))


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('family', ['negbin', 'weibull', 'ordinal'])
def test_candidate_sums_give_the_parent_builds_bits(parent, family, n):
    from make_cand_sums_bits import compute, rows
    assert rows() == ROWS
    out = compute(family, n)
    assert set(out) == {'k1', 'k3', 'k8'}
    assert out['k1'].shape == (1,) and out['k3'].shape == (3,) \
        and out['k8'].shape == (8,)
    for key, val in out.items():
        assert _same_bits(val, parent['%s_%d_%s' % (family, n, key)]), key
    # the sum of a candidate depends neither on the number of candidates nor
    # on its place among them, nor on whether the linear predictor is cached
    assert _same_bits(out['k8'][-1:], out['k1'])


def test_weibull_overflow_row(parent):
    from make_cand_sums_bits import compute_weibull_overflow
    got = compute_weibull_overflow(VEC_BLOCK + 1)
    # one row's eta + k lt is past exp's range for the second candidate alone:
    # its sum is exactly -inf, and the other two keep their finite bits
    assert got[1] == -np.inf and np.isfinite(got[[0, 2]]).all()
    assert _same_bits(got, parent['weibull_overflow'])
