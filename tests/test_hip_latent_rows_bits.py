"""GPU: the chains of the latent families (csrc/probit.hip, student_t.hip,
censored.hip on csrc/latent_rows.hpp, driven by chain.hip's one family
description) against the bits that the build of the commit before the fold
onto one kernel skeleton produced on an MI355X
(tests/golden/latent_rows_parent_bits.npz, written by
tests/golden/make_latent_rows_bits.py): latent, zbase, coef, the scalar
obs_prec, loglik and logp after create, set_state, init_obs_prec and each of
three 'cholesky' iterations (three 'cg' iterations at the two smallest and the
largest row count; Student-t: after set_df too), at the row counts where the
row kernel changes path."""
import os

import numpy as np
import pytest

from make_latent_rows_bits import _constant

pytestmark = pytest.mark.gpu

WAVE = _constant('WAVE', 'common.hpp')
ROW_GRID = _constant('ROW_GRID', 'chain.hpp')
ROWS = (1, WAVE - 1, WAVE + 1, 255, 257, ROW_GRID * 256 + 3)
CG_ROWS = (1, WAVE - 1, ROW_GRID * 256 + 3)
VALUES = ('latent', 'zbase', 'coef', 'obs_prec', 'loglik', 'logp')


def _keys(family, n):
    states = ['create', 'set_state', 'init'] + ['cholesky%d' % k
                                                for k in range(3)]
    if n in CG_ROWS:
        states += ['cg%d' % k for k in range(3)]
    if family == 'student_t':
        states.append('df7')
    values = [v for v in VALUES if v != 'obs_prec' or family != 'probit']
    return {'%s_%s' % (s, v) for s in states for v in values}


@pytest.fixture(scope='module')
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, 'latent_rows_parent_bits.npz'))


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('family', ['probit', 'student_t', 'censored'])
def test_chains_give_the_parent_builds_bits(parent, family, n):
    from make_latent_rows_bits import cg_rows, compute, rows
    assert rows() == ROWS and cg_rows() == CG_ROWS
    out = compute(family, n)
    assert set(out) == _keys(family, n)
    for key, val in out.items():
        want = parent['%s_%d_%s' % (family, n, key)]
        assert val.dtype == want.dtype == np.uint64, key
        assert val.shape == want.shape and np.array_equal(val, want), key
