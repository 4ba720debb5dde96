"""Inputs and tolerances of the draw-by-draw pin of the Student-t model's mixing
weights (csrc/student_t.hip, pass B) to the host replay of gamma_draw
(bayesbridge_amd.replay.gamma).

Shared by tests/test_student_t_replay_cpu.py, which measures on these very
inputs how far a replayed weight moves when psi moves by the float64 product's
own rounding, and tests/test_hip_student_t.py (device against replay).

A weight is omega_i = g_i / ((nu + tau r_i^2) / 2), r = y - psi, with g_i the
Gamma((nu+1)/2) variate of Philox(seed, STREAM_MIX | it << 8, i).  g_i depends
on (seed, iteration, row, nu) alone: device and replay take the same branches
whatever the data, so no draw may be excluded (cap 0), and the tolerance is

  replay_cases.GAMMA_TOL           the two libms over the variate's arithmetic
  + CHAIN_WEIGHT_CHANGE[nu]        psi = X~ beta summed in another order

d log omega / d psi = 2 tau r / (nu + tau r^2), at most sqrt(tau / nu) in
magnitude (at tau r^2 = nu), so a weight moves by at most sqrt(tau / nu) |dpsi|
relative to itself: the measured values have to respect that bound.
"""
import numpy as np

import replay_cases as C

SIZES = (1, 255, 256, 257, 524289)     # the last: ROW_GRID * 256 + 1
DFS = (.5, 4., 30.)                    # (nu + 1) / 2 = .75: gamma_draw's boost
PLANTED = [0., 1e-8, -1e-8, 1e3, -1e3, 1e8, -1e8, 1e150, -1e150]
SEED = 23
ITERATION = 2                          # the stream the weights are drawn on
COEF = np.array([.5, 1., -1., .25])    # intercept first
TAU = 1.7

# ---- measured on the CPU over the inputs below
# (test_student_t_replay_cpu.py): the largest relative change of a weight when
# psi moves by +-replay_cases.CHAIN_PSI_DELTA max(1, |psi|), per nu
CHAIN_WEIGHT_CHANGE = {.5: 2.5e-14, 4.: 9.2e-15, 30.: 3.2e-15}
WEIGHT_TOL = {nu: C.GAMMA_TOL + change
              for nu, change in CHAIN_WEIGHT_CHANGE.items()}
# weights of one chain on an f32-stored design: replay_cases.CHAIN_F32_TOL
WEIGHT_CAP = 0


def weight_inputs(n):
    """(X raw [n, 3], the coefficients, psi as the oracle forms it, y, the
    planted positions): residuals N(0, 1.5^2) with every 13th one ten times
    wider, and from 255 rows on every planted residual at 3, 12, 21, ... from
    both ends.  psi = X~ COEF, X~ = [1, X - column means]; but one row centred
    is a row of zeros, which a design refuses, so n = 1 is the raw row without
    an intercept: psi = X COEF[1:]."""
    rng = np.random.default_rng(9000 + n)
    X = rng.standard_normal((n, 3))
    if n == 1:
        coef, psi = COEF[1:], X @ COEF[1:]
    else:
        Xt = np.hstack([np.ones((n, 1)), X - X.mean(axis=0)])
        coef, psi = COEF, Xt @ COEF
    resid = rng.normal(0., 1.5, n)
    resid[::13] *= 10.
    where = np.zeros(0, dtype=np.int64)
    if n >= 255:
        pos = 3 + 9 * np.arange(len(PLANTED))
        assert pos.max() < n - 1 - pos.max()
        where = np.concatenate((pos, n - 1 - pos))
        resid[where] = PLANTED + PLANTED
    y = psi + resid
    return X, coef, psi, y, where


def weight_change(psi, y, tau, nu, delta=C.CHAIN_PSI_DELTA):
    """Largest |omega(psi +- d) / omega(psi) - 1|, d = delta max(1, |psi|): the
    Gamma variate cancels."""
    d = delta * np.maximum(1., np.abs(psi))
    base = nu + tau * (y - psi) ** 2
    worst = 0.
    for s in (-1., 1.):
        moved = nu + tau * (y - (psi + s * d)) ** 2
        worst = max(worst, float(np.abs(base / moved - 1.).max()))
    return worst


def weight_change_bound(psi, tau, nu, delta=C.CHAIN_PSI_DELTA):
    return np.sqrt(tau / nu) * delta * max(1., float(np.abs(psi).max()))


# ---- the posterior test (test 3 of tests/test_hip_student_t.py)
POSTERIOR_DATA_SEED = 12
