"""GPU: model.predict of the linear, logit, Poisson, negative-binomial and
ordinal models (csrc/predict.hip, negbin_predict.hip and ordinal_predict.hip
on the accumulators and the pass driver of csrc/predict_summary.hpp) against
the bits that the build of the commit before that fold produced on an MI355X
(tests/golden/predict_parent_bits.npz, written by
tests/golden/make_predict_bits.py, which says what is crossed with what):
every result at the row counts around a workgroup's edge, with one draw, two,
five and one more than a default pass, in passes of the default size, of one
draw, of two and of all of them, with an outcome and without, with the draws
returned, and on the non-finite paths -- a mean that overflows in one draw
and sticks, a log-likelihood of -inf in one draw and in all, a NaN draw."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from make_predict_bits import (ARRAYS, cases, compute, n_draws, name, pack,
                               rows, same_bits)

pytestmark = pytest.mark.gpu

HEADER = open(os.path.join(ROOT, 'bayes-bridge_amd', 'csrc',
                           'predict_summary.hpp')).read()
BLOCK, DRAWS = (int(re.search(r'constexpr int %s = (\d+);' % name_,
                              HEADER).group(1))
                for name_ in ('PRED_BLOCK', 'PRED_DRAWS'))
CASES = cases()


@pytest.fixture(scope='module')
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, 'predict_parent_bits.npz'))


def test_the_cases_are_the_fixtures(parent):
    assert rows() == (1, BLOCK - 1, BLOCK + 1, 2 * BLOCK + 3)
    assert n_draws() == (1, 2, 5, DRAWS + 1)
    assert {name(case) for case in CASES} == set(parent.files)
    # every cell in passes of the default size, of 1, of 2 and of all its draws
    for case in CASES:
        assert {c[5] for c in CASES if c[:5] == case[:5]} \
            == {0, 1, 2, case[2]}


@pytest.mark.parametrize(
    'case', CASES, ids=['%s-per%d' % (name(case), case[5]) for case in CASES])
def test_predict_gives_the_parent_builds_bits(parent, case):
    res = compute(case)
    want = parent[name(case)]
    assert pack(res).shape == want.shape
    at = 0
    for key in ARRAYS:
        if key in res:
            size = res[key].size
            assert same_bits(res[key], want[at:at + size]), key
            at += size
