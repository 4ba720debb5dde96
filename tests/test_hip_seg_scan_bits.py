"""GPU: the handles whose likelihoods run the block scan of csrc/seg_scan.hpp
-- the conditional Poisson model (csrc/cpoisson.hip), the stratified Cox model
(csrc/cox_strat.hpp) and the five handles that launch cox_scan_out_kernel
(csrc/cox_scan.hpp) -- against the bits that the build of the commit before
the three copies of the scan were folded onto one skeleton produced on an
MI355X (tests/golden/seg_scan_parent_bits.npz, written by
tests/golden/make_seg_scan_bits.py): the log-likelihood, the gradient, one
Hessian matvec after set_location and the end state of a 3-step trajectory,
on every stratum layout and row count of make_seg_scan_bits.cases()."""
import os

import numpy as np
import pytest

from make_seg_scan_bits import cases, compute, key

pytestmark = pytest.mark.gpu

VALUES = ('loglik', 'grad', 'hessian_matvec', 'traj_q', 'traj_p', 'traj_logp',
          'traj_grad')


@pytest.fixture(scope='module')
def parent(golden_dir):
    return np.load(os.path.join(golden_dir, 'seg_scan_parent_bits.npz'))


def test_the_fixture_holds_the_cases_and_nothing_else(parent):
    """26 cases; the conditional Poisson layouts at two scales of beta."""
    want = set()
    for case in cases():
        scales = ('s0.3',)
        if case[0] == 'cpoisson':
            scales = ('shift',) if case[1] == 'shift800' else ('s0.3', 's2')
        want |= {key(case, '%s_%s' % (s, v)) for s in scales for v in VALUES}
    assert len(cases()) == 26 and set(parent.files) == want


@pytest.mark.parametrize('case', cases(), ids=lambda c: '%s-%s' % c)
def test_handles_give_the_parent_builds_bits(parent, case):
    out = compute(case)
    mine = {name for name in parent.files if name.startswith(key(case, ''))}
    assert {key(case, name) for name in out} == mine
    for name, val in out.items():
        want = parent[key(case, name)]
        assert val.dtype == want.dtype == np.uint64, name
        assert val.shape == want.shape and np.array_equal(val, want), name
