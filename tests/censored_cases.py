"""Inputs, seeds and the comparison rule of the draw-by-draw pin of the
censored-outcome model's latent kernel (csrc/censored.hip: TruncatedNormal of
csrc/samplers.hpp at psi' = (psi - b) sqrt(tau), then z = b + u / sqrt(tau)) to
its host replay (bayesbridge_amd.replay.censored_normal).

Shared by tests/test_censored_replay_cpu.py, which measures on these very
inputs how far the replay moves when only its arithmetic changes (variant 0
against variant 1), and tests/test_hip_censored.py (device against replay).
The rule is replay_cases.py's: tolerance = 1000 x the largest difference of the
two variants, not below 1e-12.

Differences are probit_cases.difference's, applied to u = (z - b) sqrt(tau) at
psi' = (psi - b) sqrt(tau): absolute over max(1, |psi'|) where the draw is psi'
+ normal, relative where it is the exponential variate.  u is recovered from
the stored z, so a last-bit change of u can move z by a whole ulp of b: in u's
units 2^-52 |b| sqrt(tau) / |u|, far above the sampler's own rounding when |u|
sqrt(tau) is small against |b|.  The inputs keep that term small where it
would drown the comparison: a = (b - psi) sqrt(tau) has the same law at every
tau (psi is placed around b at the scale 1 / sqrt(tau)), and the planted rows
have b = 0, where z = u / sqrt(tau) holds every bit of the far-tail draws (|u|
down to 1e-8).  b + u / sqrt(tau) with b != 0 is what all other rows do.
"""
import numpy as np

import probit_cases as P
import replay_cases as C
from bayesbridge_amd import replay as R

# ---- measured on the CPU over the inputs below (test_censored_replay_cpu.py):
# the largest difference of variant 0 and variant 1 (it sits at tau = 1e6,
# where an ulp of b is 2^-52 |b| 1e3 in u's units); no draw of 1 575 186 took a
# different number of trials
CN_VARIANT_SPREAD = 3.4e-12
CN_TOL = C.tolerance(CN_VARIANT_SPREAD)

# The chain-level check recomputes psi = X~ beta with the oracle's design:
# |psi_device - psi_oracle| <= replay_cases.CHAIN_PSI_DELTA max(1, |psi|).
# Measured by test_censored_replay_cpu.py on 50 000 draws at tau = 1, in the
# units above.
CHAIN_LATENT_CHANGE = 1.7e-13
CHAIN_LATENT_TOL = CN_TOL + 100 * CHAIN_LATENT_CHANGE

# the data seed of the posterior test (censored_oracle.posterior_problem):
# 43 % of the rows right-censored
POSTERIOR_DATA_SEED = 21

# X~^T y of linear_problem() summed in two orders (row after row, and NumPy's
# pairwise sum of each column), relative to its largest entry: measured by
# test_censored_replay_cpu.py.  A censored chain without a censored row forms
# zbase = X~^T z, z = y, through another fold than a linear chain's X~^T y.
RHS_ORDER_SPREAD = 1.3e-15
RHS_ORDER_TOL = C.tolerance(RHS_ORDER_SPREAD)

CN_TAUS = (1e-6, 1., 1e6)
# (n, status, flavour): n = 1 holds ONE row, so it comes once per status and,
# for the censored ones, per regime (flavour 0: the plain rejection, 1:
# Robert's exponential); larger n mix the statuses, a third each.  524 289 is
# one row past ROW_GRID x 256, where the grid-stride loop takes its second lap.
CN_SHAPES = ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1),
             (255, -1, 0), (256, -1, 0), (257, -1, 0), (524289, -1, 0))
CN_CASES = tuple(shape + (tau,) for shape in CN_SHAPES for tau in CN_TAUS)
CN_PLANTED = [0., 1e-8, -1e-8, 37., -37., 40., -40., 1e3, -1e3, 1e8, -1e8]
CN_NONFINITE = [np.nan, np.inf, -np.inf]
# Seeds found by `search_seed` on the CPU replay: the smallest seed >= 1 with
# which (a) the two variants alone exclude no draw, (b) the case holds a
# censored row of at least 3 trials in each regime (n = 1: in its flavour's; an
# observed row takes none) and (c) no planted |a| <= 1e-8 puts psi' + normal
# within 1e-12 of 0 in any of its trials.  test_censored_replay_cpu.py asserts
# the three.  (The same seed serves a shape at every tau: a's law does not
# depend on tau.)
_SHAPE_SEEDS = {(1, 0, 0): 1, (1, 1, 0): 7, (1, 1, 1): 2, (1, 2, 0): 1,
                (1, 2, 1): 2, (255, -1, 0): 1, (256, -1, 0): 1,
                (257, -1, 0): 1, (524289, -1, 0): 1}
CN_SEEDS = {case: _SHAPE_SEEDS[case[:3]] for case in CN_CASES}


def case_id(case):
    return "n%d-s%d-f%d-tau%g" % case


def cn_inputs(case):
    """(psi[n], bound[n], status uint8[n], positions of the non-finite psi)."""
    n, status1, flavour, tau = case
    rt = np.sqrt(tau)
    rng = np.random.default_rng(9000 + n + 10 * (status1 + 1) + flavour)
    a = rng.normal(0., 2., n)
    a[::13] = rng.normal(0., 12., len(a[::13]))
    bound = rng.normal(0., 2., n)
    status = rng.integers(0, 3, n).astype(np.uint8)
    bad = np.zeros(0, dtype=np.int64)
    if n == 1:
        # one row of the case's status; censored: in the flavour's regime at
        # TruncatedNormal's a = -+0.1, where a trial is accepted with
        # probability 0.54, resp. 0.78.  Right-censored rows have that a equal
        # to (b - psi) sqrt(tau), left-censored ones its negative.
        status[0] = status1
        a[0] = .1 * (1. if flavour else -1.) * (-1. if status1 == 2 else 1.)
    if n >= 255:
        # every planted value with both censored statuses, then the
        # non-finite ones, in the first block and, from 600 rows on, again in
        # the last one; b = 0 there (head comment)
        vals = np.array([v for v in CN_PLANTED for _ in (0, 1)])
        sts = np.array([s for _ in CN_PLANTED for s in (1, 2)]
                       + [1, 2, 0], dtype=np.uint8)
        pos = 3 + 9 * np.arange(len(vals) + 3)
        assert pos.max() < 255
        where = [pos] + ([n - 1 - pos] if n >= 600 else [])
        for w in where:
            a[w[:-3]] = vals
            bound[w] = 0.
            status[w] = sts
        bad = np.concatenate([w[-3:] for w in where])
    psi = bound - a / rt
    for k in range(0, len(bad), 3):
        psi[bad[k:k + 3]] = CN_NONFINITE
    return psi, bound, status, np.sort(bad)


def scaled(psi, bound, tau):
    """psi' as the kernel and the replay form it."""
    with np.errstate(invalid='ignore', over='ignore'):
        return (psi - bound) * np.sqrt(np.float64(tau))


def to_u(z, bound, tau):
    with np.errstate(invalid='ignore'):
        return (np.asarray(z) - bound) * np.sqrt(np.float64(tau))


def difference(x, y, psi, bound, status, tau):
    """probit_cases.difference on u = (z - b) sqrt(tau); 0 on observed rows
    that agree bit for bit (inf where they do not)."""
    x, y = np.asarray(x), np.asarray(y)
    d = P.difference(to_u(x, bound, tau), to_u(y, bound, tau),
                     scaled(psi, bound, tau), status == 1)
    obs = status == 0
    d[obs] = np.where(x[obs] == y[obs], 0., np.inf)
    return d


def compare(name, dev, rep, psi, bound, status, tau, tol, detail=None):
    """replay_cases.compare on the differences above: all within `tol` except
    at most cap(n) draws, each of which is printed."""
    d = difference(dev, rep, psi, bound, status, tau)
    return C.compare(name, 1. + d, np.ones(d.shape), tol, detail)


def small_planted_margin(case, seed, stream=R.STREAM_LATENT):
    """min |psi' + normal| over the trials of the planted |a| <= 1e-8 that sit
    in the plain-rejection regime (inf: the case plants none)."""
    psi, bound, status, _ = cn_inputs(case)
    tau = case[3]
    p = scaled(psi, bound, tau)
    _, trials = R.censored_normal(seed, stream, psi, bound, status, tau, 0,
                                  trace=True)
    worst = np.inf
    cens = status != 0
    low = np.flatnonzero(cens & (np.abs(p) <= 1e-8)
                         & ~P.regime(p, status == 1))
    for i in low:
        for t in range(int(trials[i])):
            u1, u2 = R.uniform(seed, stream, int(i), t, 2)
            normal = np.sqrt(-2. * np.log(u1)) * np.cos(2. * np.pi * u2)
            worst = min(worst, abs(p[i] + normal))
    return worst


def conditions(case, seed):
    """(draws on which the variants disagree about the trials, largest
    difference among the rest, most trials in the plain regime, most in the
    exponential regime, the margin of the small planted a)."""
    psi, bound, status, bad = cn_inputs(case)
    tau = case[3]
    z0, t0 = R.censored_normal(seed, R.STREAM_LATENT, psi, bound, status, tau,
                               0, True)
    z1, t1 = R.censored_normal(seed, R.STREAM_LATENT, psi, bound, status, tau,
                               1, True)
    same = t0 == t1
    d = difference(z0, z1, psi, bound, status, tau)
    p = scaled(psi, bound, tau)
    up = P.regime(p, status == 1)
    live = np.isfinite(p) & (status != 0)
    most = [int(t0[live & (up == r)].max()) if (live & (up == r)).any()
            else 0 for r in (False, True)]
    return (int((~same).sum()), float(d[same].max()), most[0], most[1],
            small_planted_margin(case, seed))


def holds(case, seed):
    differ, spread, low, high, margin = conditions(case, seed)
    n, status1, flavour, _ = case
    if n == 1:
        enough = status1 == 0 or (high if flavour else low) >= 3
    else:
        enough = min(low, high) >= 3
    return differ == 0 and spread <= CN_TOL and enough and margin > 1e-12


def search_seed(case, limit=400):
    """How CN_SEEDS was found."""
    return next(seed for seed in range(1, limit) if holds(case, seed))


def linear_problem():
    """(X [2000, 10], y): the data of the test that a censored chain without
    a censored row is the linear model."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((2000, 10))
    beta = np.array([4., -3., 2., -1., .5] + [0.] * 5)
    return X, .3 + X @ beta + .2 * rng.standard_normal(2000)
