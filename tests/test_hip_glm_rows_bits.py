"""GPU: the row-wise GLM handles (csrc/logit.hip, poisson.hip, negbin.hip on
csrc/glm_rows.hpp) against the bits that the build of the commit before the
fold onto one kernel skeleton produced on an MI355X
(tests/golden/glm_rows_parent_bits.npz, written by
tests/golden/make_glm_rows_bits.py): log-likelihood, gradient, one
Hessian-vector product and the end state of a 3-step trajectory at the row
counts where the row kernel changes path, the negative binomial's dispersion
sums and its gradient after set_dispersion, and the Poisson overflow rule."""
import os

import numpy as np
import pytest

from test_hip_poisson import LAP, VEC_BLOCK, _constant

pytestmark = pytest.mark.gpu

U = _constant('GLM_ROW_U', 'glm_rows.hpp')
ROWS = (1, VEC_BLOCK - 1, VEC_BLOCK + 1, LAP + 1, U * LAP + 3)
KEYS = ('loglik', 'grad', 'hessian_matvec', 'traj_q', 'traj_p', 'traj_logp',
        'traj_grad')
NEGBIN_KEYS = ('disp_k1', 'disp_k3', 'loglik_r7', 'grad_r7')


@pytest.fixture(scope='module')
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, 'glm_rows_parent_bits.npz'))


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64),
                                                 b.view(np.uint64))


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('family', ['logit', 'poisson', 'negbin'])
def test_rows_give_the_parent_builds_bits(parent, family, n):
    from make_glm_rows_bits import compute, rows
    assert rows() == ROWS
    out = compute(family, n)
    assert set(out) == set(KEYS + (NEGBIN_KEYS if family == 'negbin' else ()))
    for key, val in out.items():
        assert _same_bits(val, parent['%s_%d_%s' % (family, n, key)]), key


def test_poisson_overflow_rows(parent):
    from make_glm_rows_bits import compute_poisson_overflow
    over = compute_poisson_overflow(VEC_BLOCK + 1)
    # an offset that puts eta + o past exp's range: -inf and no gradient
    assert over['overflow'] == (-np.inf, None)
    # eta = +inf in every row: each ll_i is NaN, and mu == inf still raises
    assert over['inf_eta'] == (-np.inf, None)
    # an offset of +inf is refused at create, with the parent's status
    assert over['inf_offset_status'] < 0
    assert over['inf_offset_status'] == parent['poisson_inf_offset_status'][0]
    assert not over['inf_offset_handle']
    assert 'log_exposure[%d] is not finite' % ((VEC_BLOCK + 1) // 2) \
        in over['inf_offset_error']
