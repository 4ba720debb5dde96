"""Inputs, seeds and the comparison rule of the draw-by-draw pin of the probit
model's truncated-normal sampler (csrc/probit.hip, TruncatedNormal of
csrc/samplers.hpp) to its host replay (bayesbridge_amd.replay).

Shared by tests/test_probit_replay_cpu.py, which measures on these very inputs
how far the replay moves when only its arithmetic changes (variant 0 against
variant 1: the kernel's forms of the proposal rate and of the exponential
variate), and tests/test_hip_probit.py (device against replay).  The rule is
replay_cases.py's: tolerance = 1000 x the largest difference of the two
variants, not below 1e-12.

The difference of two draws is measured in the units in which the sampler's
arithmetic errs.  With s = +-1 and a = -s psi:
  a <= 0   z = psi + normal: absolute errors of a few ulp of max(1, |psi|),
           whatever |z| is (z lies anywhere down to 0):  |dz| / max(1, |psi|);
  a >  0   z = s e, e = -log(u) / lambda(a): relative errors:  |dz| / |z|.
"""
import numpy as np

import replay_cases as C
from bayesbridge_amd import replay as R

# ---- measured on the CPU over the inputs below (test_probit_replay_cpu.py):
# the largest difference of variant 0 and variant 1; no draw of 525 059 took a
# different number of trials
TN_VARIANT_SPREAD = 6.2e-16
TN_TOL = C.tolerance(TN_VARIANT_SPREAD)

# (n, flavour): n = 1 holds ONE element, so it comes once per regime
# (flavour 0: a <= 0, 1: a > 0); 524 289 is one row past ROW_GRID x 256, where
# the kernel's grid-stride loop takes its second lap.
TN_CASES = ((1, 0), (1, 1), (255, 0), (256, 0), (257, 0), (524289, 0))
TN_PLANTED = [0., 1e-8, -1e-8, 37., -37., 40., -40., 1e3, -1e3, 1e8, -1e8]
TN_NONFINITE = [np.nan, np.inf, -np.inf]
# Seeds found by `search_seed` on the CPU replay: the smallest seed >= 1 with
# which (a) the two variants alone exclude no draw, (b) the case holds an
# element of at least 3 trials in each regime (n = 1: in its flavour's) and
# (c) no planted psi of magnitude <= 1e-8 puts psi + normal within 1e-12 of 0
# in any of its trials.  test_probit_replay_cpu.py asserts the three.
TN_SEEDS = {(1, 0): 1, (1, 1): 2, (255, 0): 1, (256, 0): 1, (257, 0): 1,
            (524289, 0): 1}

# The chain-level check recomputes psi = X~ beta with the oracle's design:
# |psi_device - psi_oracle| <= replay_cases.CHAIN_PSI_DELTA max(1, |psi|).  A
# latent moves with psi one to one (a <= 0) or through lambda(a) (a > 0);
# measured by test_probit_replay_cpu.py on 50 000 draws, in the units above
# (2 of them change their number of trials or, at psi = 0, their regime).
CHAIN_LATENT_CHANGE = 2.8e-15
CHAIN_LATENT_TOL = TN_TOL + 100 * CHAIN_LATENT_CHANGE


def tn_inputs(case):
    """(psi[n], positive uint8[n], positions of the non-finite psi)."""
    n, flavour = case
    rng = np.random.default_rng(7000 + n + flavour)
    psi = rng.normal(0., 2., n)
    psi[::13] = rng.normal(0., 12., len(psi[::13]))
    positive = (rng.random(n) < .5).astype(np.uint8)
    bad = np.zeros(0, dtype=np.int64)
    if n == 1:
        # one element in the flavour's regime, a = -s psi = -+0.1: where a
        # trial is accepted with probability 0.54, resp. 0.78
        psi[0] = .1 * (1. if positive[0] else -1.) * (-1. if flavour else 1.)
    if n >= 255:
        # every planted value with both outcomes, then the non-finite ones, in
        # the first block and, from 600 elements on, again in the last one
        vals = np.array([v for v in TN_PLANTED for _ in (0, 1)]
                        + TN_NONFINITE)
        ys = np.array([y for _ in TN_PLANTED for y in (1, 0)]
                      + [1, 0, 1], dtype=np.uint8)
        pos = 3 + 9 * np.arange(len(vals))
        assert pos.max() < 255
        where = [pos] + ([n - 1 - pos] if n >= 600 else [])
        for w in where:
            psi[w] = vals
            positive[w] = ys
        bad = np.concatenate([w[-3:] for w in where])
    return psi, positive, np.sort(bad)


def regime(psi, positive):
    """True where a = -s psi > 0 (the exponential proposal)."""
    s = np.where(np.asarray(positive) != 0, 1., -1.)
    return -s * psi > 0.


def difference(x, y, psi, positive):
    """|x - y| in the units of the head comment; 0 where both are NaN."""
    x, y = np.asarray(x), np.asarray(y)
    with np.errstate(invalid='ignore', divide='ignore'):
        den = np.where(regime(psi, positive), np.abs(y),
                       np.maximum(1., np.abs(psi)))
        d = np.abs(x - y) / den
    d[x == y] = 0.
    d[np.isnan(x) & np.isnan(y)] = 0.
    return d


def compare(name, dev, rep, psi, positive, tol, detail=None):
    """replay_cases.compare on the differences above: all within `tol` except
    at most cap(n) draws, each of which is printed."""
    d = difference(dev, rep, psi, positive)
    # (1 + d against 1: the relative difference replay_cases.compare forms is
    # d itself, to the 2e-16 of the addition)
    return C.compare(name, 1. + d, np.ones(d.shape), tol, detail)


def small_planted_margin(case, seed, stream=R.STREAM_LATENT):
    """min |psi + normal| over the trials of the planted |psi| <= 1e-8 that
    sit in the a <= 0 regime (inf: the case plants none)."""
    psi, positive, _ = tn_inputs(case)
    _, trials = R.truncated_normal(seed, stream, psi, positive, 0, trace=True)
    worst = np.inf
    low = np.flatnonzero((np.abs(psi) <= 1e-8) & ~regime(psi, positive))
    for i in low:
        for t in range(int(trials[i])):
            u1, u2 = R.uniform(seed, stream, int(i), t, 2)
            normal = np.sqrt(-2. * np.log(u1)) * np.cos(2. * np.pi * u2)
            worst = min(worst, abs(psi[i] + normal))
    return worst


def conditions(case, seed):
    """(draws on which the variants disagree about the trials, largest
    difference among the rest, most trials in the a <= 0 regime, most in the
    a > 0 regime, the margin of the small planted psi)."""
    psi, positive, bad = tn_inputs(case)
    z0, t0 = R.truncated_normal(seed, R.STREAM_LATENT, psi, positive, 0, True)
    z1, t1 = R.truncated_normal(seed, R.STREAM_LATENT, psi, positive, 1, True)
    same = t0 == t1
    d = difference(z0, z1, psi, positive)
    up = regime(psi, positive)
    finite = np.isfinite(psi)
    most = [int(t0[finite & (up == r)].max()) if (finite & (up == r)).any()
            else 0 for r in (False, True)]
    return (int((~same).sum()), float(d[same].max()), most[0], most[1],
            small_planted_margin(case, seed))


def holds(case, seed):
    differ, spread, low, high, margin = conditions(case, seed)
    n, flavour = case
    enough = (high if flavour else low) >= 3 if n == 1 \
        else min(low, high) >= 3
    return differ == 0 and spread <= TN_TOL and enough and margin > 1e-12


def search_seed(case, limit=200):
    """How TN_SEEDS was found."""
    return next(seed for seed in range(1, limit) if holds(case, seed))
