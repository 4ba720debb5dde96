"""Inputs and tolerances of the draw-by-draw pin of the quantile model's mixing
weights (csrc/quantile.hip, pass B) to the host replay of the inverse-Gaussian
draw (bayesbridge_amd.replay.inverse_gaussian).

Shared by tests/test_quantile_replay_cpu.py, which measures on these very
inputs how far a replayed weight moves when psi moves by the float64 product's
own rounding, and tests/test_hip_quantile.py (device against replay).

A weight is w_i = InverseGaussian(mean 1 / m_i, shape lambda), m_i = q (1 - q)
|y_i - psi_i|, lambda = tau / (2 q (1 - q)), from one normal and one uniform of
Philox(seed, STREAM_QMIX | it << 8, i).  The draw has ONE data-dependent
branch, u (1 + m x) <= 1: device and replay take the same one as long as no
draw's u (1 + m x) lies within BRANCH_MARGIN of 1 -- the CPU test asserts that
on these inputs under either perturbation of psi -- so no draw may be excluded
(cap 0), and the tolerance is

  replay_cases.GAMMA_TOL           the two libms over the normal's log and
                                   cospi (the rest is +, *, /, sqrt)
  + CHAIN_WEIGHT_CHANGE[q]         psi = X~ beta summed in another order
"""
import numpy as np

import replay_cases as C
from student_t_cases import SIZES, PLANTED, COEF, weight_inputs  # noqa: F401

QUANTILES = (.05, .5, .9)
SEED = 23
ITERATION = 2                          # the stream the weights are drawn on
TAU = 1.7
BRANCH_MARGIN = 1e-9

# ---- measured on the CPU over the inputs above
# (test_quantile_replay_cpu.py): the largest relative change of a weight when
# psi moves by +-replay_cases.CHAIN_PSI_DELTA max(1, |psi|), per q.  It is the
# same for every q, and far above the Student-t weights' 1e-14: where the normal
# is near 0 the draw is w ~ 1 / m, which moves by dpsi / |r| relative to itself,
# and among 524 289 rows one has |r| = 1.2e-4 (2e-15 / 1.2e-4 = 1.6e-11).  The
# closest u (1 + m x) comes to 1 on these inputs is 4.3e-7.
CHAIN_WEIGHT_CHANGE = {.05: 1.3e-11, .5: 1.3e-11, .9: 1.3e-11}
WEIGHT_TOL = {q: C.GAMMA_TOL + change
              for q, change in CHAIN_WEIGHT_CHANGE.items()}
# weights of one chain on an f32-stored design: replay_cases.CHAIN_F32_TOL
WEIGHT_CAP = 0


def level(q):
    """(q (1 - q), the shape lambda at TAU)."""
    qq = q * (1. - q)
    return qq, TAU / (2. * qq)


def replayed(stream, psi, y, q, tau=TAU, seed=SEED):
    """(weights, branch, u (1 + m x)) of the replay at (psi, y)."""
    from bayesbridge_amd import replay as R
    qq = q * (1. - q)
    return R.inverse_gaussian(seed, stream, qq * np.abs(y - psi),
                              tau / (2. * qq), trace=True, margin=True)


# ---- the posterior test (test 8 of tests/test_hip_quantile.py)
POSTERIOR_DATA_SEED = 12
POSTERIOR_Q = .8
