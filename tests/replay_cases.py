"""Inputs and the comparison rule of the draw-by-draw pin of the device
samplers to the host replay (bayesbridge_amd.replay, csrc/replay_impl.hpp).

Shared by tests/test_replay_cpu.py (which measures, on these very inputs, how
far the replay moves when only its arithmetic changes: variant 0 against
variant 1) and tests/test_hip_sampler_replay.py (device against replay).

Tolerances.  A draw is a chain of libm calls on shared uniforms; device (OCML)
and host (glibc) differ by a few ulp per call, amplified by the last power
(exponent up to 7 at a = 1/8, `exp(y log x)` on the device).  The stand-in for
that on the CPU is variant 0 against variant 1 -- the same draws with the
kernels' forms of the arithmetic.  Rule: tolerance = 1000 x the largest
relative difference of the two variants over these inputs, not below 1e-12;
measured values below (test_replay_cpu.py asserts that the measurement still
holds and prints it).
"""
import numpy as np

# ---- measured on the CPU over the inputs below: largest relative difference
# between variant 0 and variant 1 among draws that took the same branches
PG_VARIANT_SPREAD = 0.            # no draw of 152 000 differs in any bit
TS_VARIANT_SPREAD = {.125: 1.6e-14, .25: 3.5e-15, .5: 4.5e-16}
# (no draw of 2 305 / 1 051 181 / 2 305 took another candidate)
GAMMA_TOL = 1e-12                 # no second form exists: the floor
NORMAL_ATOL = 1e-14               # absolute (|normal| <= 8.6, a few ulp)


def tolerance(spread):
    return max(1000. * spread, 1e-12)


def cap(n):
    """Draws that may be excluded because a uniform sits within rounding of a
    threshold and the two sides take different branches."""
    return max(2, int(1e-5 * n))


# ------------------------------------------------------------- Polya-Gamma

PG_SIZES = (1, 255, 256, 257, 49999, 50000, 51500)
PG_PLANTED = [0., 1e-8, -1e-8, 39.9999, -39.9999, 40., -40., 40.0001,
              -40.0001, 700., -700.]
PG_NONFINITE = [np.nan, np.inf, -np.inf]
# Seeds chosen by a search on the CPU replay so that every size has an
# element with more than one inverse-Gaussian attempt and one whose series
# test rejects (a restart, 7.5e-4 per draw: the sizes <= 257 would otherwise
# rarely hold one; n = 1 holds one element, which restarts after two attempts).
PG_SEEDS = {1: 2026, 255: 1, 256: 1, 257: 1, 49999: 1, 50000: 1, 51500: 1}


def pg_inputs(n):
    """(shape int32[n], tilt[n], positions of the non-finite tilts)."""
    rng = np.random.default_rng(1000 + n)
    tilt = rng.normal(0., 3., n)
    tilt[::11] = rng.normal(0., 30., len(tilt[::11]))
    shape = np.ones(n, dtype=np.int32)
    shape[::7] = rng.integers(2, 6, size=len(shape[::7]))
    if n == 1:
        shape[0] = 1          # the one element goes through the three passes
    bad = np.zeros(0, dtype=np.int64)
    if n >= 255:
        # planted values in the first block and, from 600 elements on, again in
        # the last 250 (the ragged block / the upper element slots of a lane)
        vals = np.array(PG_PLANTED + PG_NONFINITE)
        pos = 3 + 17 * np.arange(len(vals))
        where = [pos] + ([n - 1 - pos] if n >= 600 else [])
        for w in where:
            tilt[w] = vals
            shape[w] = 1
        bad = np.concatenate([w[-3:] for w in where])
    return shape, tilt, np.sort(bad)


# ----------------------------------------------------------- tilted stable

TS_EXPONENTS = (.125, .25, .5)
TS_BIG = 1048576 + 300         # grid cap 4096 blocks x 256: a second `base`


def _check_regime_margin(tp):
    """tilt^a exactly 2 or at least 1e-9 away: pow and the root forms agree
    on the regime."""
    d = np.abs(tp - 2.)
    assert np.all((d == 0.) | (d >= 1e-9))


def ts_mixed(a, n, seed=0):
    """Tilts spread over both regimes (test_hip_chain.py
    test_device_tilted_stable_mixed_tilts_match_the_host_sampler)."""
    rng = np.random.default_rng(2000 + seed + n)
    tp = np.where(rng.random(n) < .5, rng.uniform(.05, 9., n),
                  rng.uniform(9., 150., n))
    _check_regime_margin(tp)
    return tp ** (1 / a)


def ts_blocks(a):
    """Five kinds of 256-item block in one launch (1536 items):
    0 all plain rejection; 1 all double rejection; 2 one double-rejection item
    among 255 plain ones; 3 one plain item among 255 double-rejection ones;
    4 mixed with planted tilts 0, 1e-300, 2^(1/a) (tilt^a == 2 exactly) and
    tilt^a = 2 -+ 1e-6; 5 very large tilts, up to 1e40 (1e20 at a = 1/2)."""
    rng = np.random.default_rng(3000 + int(1000 * a))
    plain = lambda k: rng.uniform(.05, 1.95, k)          # noqa: E731
    double = lambda k: np.where(rng.random(k) < .6, rng.uniform(2.05, 9., k),  # noqa: E731
                                rng.uniform(9., 150., k))
    b0, b1 = plain(256), double(256)
    b2 = plain(256)
    b2[100] = 3.3
    b3 = double(256)
    b3[37] = .7
    b4 = np.where(rng.random(256) < .5, plain(256), double(256))
    tp = np.concatenate([b0, b1, b2, b3, b4])
    _check_regime_margin(tp)
    tilt = tp ** (1 / a)
    planted = np.array([0., 1e-300, 2. ** (1 / a), (2. - 1e-6) ** (1 / a),
                        (2. + 1e-6) ** (1 / a)])
    assert (2. ** (1 / a)) ** a == 2.
    _check_regime_margin(planted[3:] ** a)
    tilt[4 * 256 + 5 + 40 * np.arange(5)] = planted
    # (tilt^a <= 1e10: beyond, at a = 1/2 and tilts past 1e20, the double
    # rejection's own arithmetic cancels -- x - left at left ~ tilt^a -- and the
    # two variants of the replay ALONE differ by 4e-8 and disagree on the
    # winner of 2 draws in 256: no input for a test of bookkeeping)
    top = min(40., 10. / a)
    big = 10. ** rng.uniform(10., top, 256)
    big[0], big[255] = 10. ** top, 1e10
    return np.concatenate([tilt, big])


def ts_rounds(winner, items=256):
    """From the replay's winner indices, the round structure
    tilted_stable_block goes through for each block of `items` consecutive
    elements: a list of (copies, pending) per block."""
    out = []
    for lo in range(0, len(winner), items):
        w = np.asarray(winner[lo:lo + items], dtype=np.int64)
        tried = np.zeros(len(w), dtype=np.int64)
        pending = np.ones(len(w), dtype=bool)
        rounds = []
        while pending.any():
            m = int(pending.sum())
            copies = min(16, 256 // m)
            rounds.append((copies, m))
            done = pending & (w < tried + copies)
            tried[pending & ~done] += copies
            pending &= ~done
        out.append(rounds)
    return out


# ------------------------------------------------------------------- Gamma

GAMMA_SHAPES = (.4, 1., 3., 2.5e5)
GAMMA_N = 10000


# -------------------------------------------------------- the comparison

def compare(name, dev, rep, tol, detail=None):
    """Device draws against replayed ones: all within `tol` (relative) except
    at most cap(n), each of which is printed.  Returns (largest relative
    difference among the rest, number excluded)."""
    dev, rep = np.asarray(dev), np.asarray(rep)
    assert dev.shape == rep.shape
    both_nan = np.isnan(dev) & np.isnan(rep)
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(dev - rep) / np.abs(rep)
    rel[both_nan] = 0.
    rel[(dev == rep)] = 0.
    out = ~(rel <= tol)
    for i in np.flatnonzero(out)[:50]:
        print("%s: excluded draw %d: device %.17g replay %.17g%s"
              % (name, i, dev[i], rep[i],
                 "" if detail is None else " (%s)" % detail(i)))
    worst = float(rel[~out].max()) if (~out).any() else 0.
    print("%s: n = %d, largest relative difference %.3g (tolerance %.3g), "
          "excluded %d (cap %d)" % (name, dev.size, worst, tol, int(out.sum()),
                                    cap(dev.size)))
    assert int(out.sum()) <= cap(dev.size), (name, int(out.sum()))
    return worst, int(out.sum())


# ------------------------------------------------- the chain-level checks
# (tests/test_hip_chain_pin.py) recompute psi = X~ beta, sum |beta|^alpha and
# the residual sum of squares with the oracle instead of reading the device's.
#
# psi: device kernels against the oracle's design on the pin's eight cases,
# |psi_device - psi_oracle| <= 1.7e-15 max(1, |psi|) with f64 storage (MI355X;
# relative to |psi| alone up to 1.8e-11, at rows whose psi cancels to ~1e-4 --
# where a Polya-Gamma draw depends on psi^2 only).  CHAIN_PSI_DELTA rounds that
# up; test_replay_cpu.py perturbs the replay's tilts by it and measures the
# largest relative change of a draw: 7.2e-15 (no draw of 50 000 changes its
# branch).  Tolerance of the Omega check: 100 x that on top of the tolerance
# of the stand-alone Polya-Gamma comparison.
CHAIN_PSI_DELTA = 2e-15
CHAIN_OMEGA_CHANGE = 7.3e-15
CHAIN_OMEGA_TOL = tolerance(PG_VARIANT_SPREAD) + 100 * CHAIN_OMEGA_CHANGE
# tau and the observation precision are smooth in the recomputed sum (the Gamma
# variate does not depend on it): tau moves by delta / alpha, the precision by
# delta.  Sums of positive terms (sum |beta|^alpha over <= 1e4 coefficients,
# the residual sum of squares over <= 5e4 rows) in two summation orders differ
# by a few units of 2^-53 log2(n): delta <= 2e-15 (measured for the residual
# sums: <= 2.3e-16), times 1 / alpha = 2 for tau, times 100: below the floor
# of 1e-12.  With f32 storage the device's operator holds the centred entries
# rounded to 24 bits: psi differs by up to 1.9e-7 (measured), and with errors
# of random sign the residual sum of squares by 2 x 1.9e-7 / sqrt(n) = 7e-9 at
# n = 3 000 (measured on random coefficients: 1.3e-9) -- delta = 1e-8, times 100.
CHAIN_SCALAR_TOL = 1e-12
CHAIN_F32_TOL = 1e-6
