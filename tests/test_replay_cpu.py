"""CPU: the sequential host replay of the device samplers
(bayesbridge_amd.replay, csrc/replay_impl.hpp) -- the reference that
tests/test_hip_sampler_replay.py pins the kernels to, draw by draw.

A replay that restated a kernel's mistake would pin the mistake, so it is
checked here on its own: its Philox against the published known answers, the
counter layout against what csrc/philox.hpp documents, and the LAW of its
draws against closed forms at a power the GPU tests cannot afford (2e6
Polya-Gamma and 1e6 tilted-stable draws per setting, every check at 6 sigma).
The last test measures, on the inputs of the GPU tests, how far the draws move
when nothing but the arithmetic changes (variant 0 against variant 1): the
figure the GPU tests' tolerance is derived from.
"""
import numpy as np
from scipy import stats

import replay_cases as C
from bayesbridge_amd import replay as R

SIX_SIGMA_P = 1.97e-9          # two-sided tail of a normal beyond 6 sigma


# ------------------------------------------------------------------ Philox

def test_philox_known_answers():
    """Philox4x32-10 known-answer vectors of Random123 (Salmon et al.,
    SC'11; kat_vectors)."""
    def words(text):
        return [int(w, 16) for w in text.split()]
    kat = [([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ([0xffffffff] * 4, [0xffffffff] * 2,
            "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           (words("243f6a88 85a308d3 13198a2e 03707344"),
            words("a4093822 299f31d0"),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert list(R.philox_block(counter, key)) == words(want)


def test_philox_counter_layout_is_the_documented_one():
    """csrc/philox.hpp: key = seed; ctr[0] = sub-stream << 20 | draw counter,
    ctr[1] = low stream word, ctr[2] = low index word, ctr[3] = high index
    word ^ (high stream word << 16).  The chain's stream word is
    id | iteration << 8: from iteration 2^24 on its bits reach ctr[3]."""
    seed = 0x1122334455667788
    it = (1 << 24) + 5
    stream = R.iter_stream(R.STREAM_PG, it)
    assert stream == 3 | (it << 8) and stream >> 32 == 1
    index = (7 << 32) | 9
    ctr, key = R.philox_counter(seed, stream, index, 130)
    assert list(key) == [0x55667788, 0x11223344]
    assert list(ctr) == [130 << 20, (3 | (5 << 8)), 9, 7 ^ (1 << 16)]
    # a stream that differs in its high word only is another stream
    lo = R.iter_stream(R.STREAM_PG, 5)
    assert R.philox_counter(seed, lo, index, 130)[0][3] == 7
    assert not np.array_equal(R.normal(seed, stream, 8), R.normal(seed, lo, 8))
    # uniforms: words are handed out from the END of a block, two per
    # uniform, 53 bits, never 0 or 1; the counter's low word counts blocks
    u = R.uniform(seed, stream, index, 130, 6)
    for b in range(3):
        c = ctr.copy()
        c[0] += b
        w = [int(x) for x in R.philox_block(c, key)]
        for k, (hi, lo_) in enumerate([(w[3], w[2]), (w[1], w[0])]):
            bits = ((hi << 32) | lo_) >> 11
            assert u[2 * b + k] == (bits + .5) / 2. ** 53
    assert np.all((u > 0) & (u < 1))
    # sub-streams and elements are distinct streams
    assert not np.array_equal(R.uniform(seed, stream, index, 131, 6), u)
    assert not np.array_equal(R.uniform(seed, stream, index + 1, 130, 6), u)


def test_replayed_normals_are_standard_normal_to_the_last_digits():
    """Box-Muller with cos(2 pi u) reduced exactly: against a 40-digit
    evaluation from the same uniforms the relative error stays at a few ulp,
    also next to the zeros of the cosine, where cos(2 * M_PI * u) loses it."""
    seed, stream, n = 77, R.iter_stream(R.STREAM_ETA1, 3), 200000
    x = R.normal(seed, stream, n)
    u = np.array([R.uniform(seed, stream, i, 0, 2) for i in range(2000)])
    import mpmath
    mpmath.mp.dps = 40
    want = np.array([float(mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(u1))) *
                           mpmath.cospi(2 * mpmath.mpf(u2))) for u1, u2 in u])
    rel = np.abs(x[:2000] / want - 1)
    print("replayed normals against 40-digit arithmetic: largest relative "
          "error %.3g" % rel.max())
    assert rel.max() < 8 * 2. ** -53
    # next to the zeros of the cosine as well
    close = np.abs(np.abs(u[:, 1] % .5) - .25) < 2e-3
    assert close.sum() >= 5
    # at a zero: u2 = 1/4 + 2^-40 exactly -> cos(2 pi u2) = -sin(2 pi 2^-40)
    near = .25 + 2. ** -40
    from math import cos, pi, sin
    exact = -sin(2 * pi * 2. ** -40)
    assert abs(cos(2 * pi * near) / exact - 1) > 1e-6      # the naive form
    se = 1 / np.sqrt(n)
    assert abs(x.mean()) < 6 * se and abs(x.var() - 1) < 6 * np.sqrt(2.) * se
    assert stats.kstest(x, 'norm').pvalue > SIX_SIGMA_P


# --------------------------------------------------------------- the laws

def _logcosh(x):
    x = np.abs(x)
    return x + np.log1p(np.exp(-2 * x)) - np.log(2.)


def _six_sigma(sample, want, what):
    n = sample.size
    se = sample.std() / np.sqrt(n)
    assert abs(sample.mean() - want) < 6 * se, (what, sample.mean(), want, se)


def test_replayed_polya_gamma_has_the_right_law():
    """PG(1, c): mean tanh(c/2) / 2c, variance (sinh c - c) / (4 c^3
    cosh^2(c/2)), Laplace transform E exp(-t w) = cosh(c/2) /
    cosh(sqrt((c^2/2 + t) / 2)) (Polson, Scott & Windle 2013, eq. 4-5); tilts
    on both sides of the right_mass_direct switch at |c| = 40 (variant 1 is the
    kernel's arithmetic) and of the inverse-Gaussian regimes."""
    n = 2000000
    ones = np.ones(n, dtype=np.int32)
    for k, c in enumerate((0., .05, 1.2, 8., 39.9, 40.1, 120.)):
        w = R.polya_gamma(40 + k, R.STREAM_PG, ones, np.full(n, c),
                          variant=k % 2)
        assert np.all(w > 0) and np.all(np.isfinite(w))
        if c == 0.:
            mean, var = .25, 1 / 24.
        else:
            mean = np.tanh(c / 2) / (2 * c)
            # (sinh c - c) / cosh^2(c/2) = 2 (sinh c - c) / (1 + cosh c)
            var = (np.tanh(c / 2) - c / (1 + np.cosh(c))) / (2 * c ** 3)
        _six_sigma(w, mean, ('mean', c))
        _six_sigma((w - mean) ** 2, var, ('variance', c))
        for t in (.5, 4., 30.):
            want = np.exp(_logcosh(c / 2) -
                          _logcosh(np.sqrt((c * c / 2 + t) / 2)))
            _six_sigma(np.exp(-t * w), want, ('laplace', c, t))


def test_replayed_binomial_polya_gamma_and_traces():
    """Shapes 2..5 go through the sequential sampler on sub-stream 0 (double
    and int32 shapes alike); the traces count what they say."""
    n = 400000
    rng = np.random.default_rng(0)
    shape = rng.integers(2, 6, n).astype(np.int32)
    c = 1.7
    w = R.polya_gamma(3, R.STREAM_PG, shape, np.full(n, c))
    assert np.array_equal(
        w, R.polya_gamma(3, R.STREAM_PG, shape.astype(np.float64),
                         np.full(n, c)))
    mean = np.tanh(c / 2) / (2 * c)
    _six_sigma(w / shape, mean, 'binomial mean')
    ones = np.ones(n, dtype=np.int32)
    w, att, rst = R.polya_gamma(3, R.STREAM_PG, ones, np.full(n, c),
                                trace=True)
    assert att.min() == 0 and att.max() > 3 and 0 < rst.mean() < 2e-3
    tilt = np.full(8, c)
    tilt[[2, 5, 6]] = [np.nan, np.inf, -np.inf]
    out = R.polya_gamma(3, R.STREAM_PG, ones[:8], tilt)
    assert np.array_equal(np.isnan(out), ~np.isfinite(tilt))
    assert np.array_equal(out[[0, 1, 3, 4, 7]], w[[0, 1, 3, 4, 7]])


def test_replayed_tilted_stable_has_the_right_law():
    """X ~ e^{-lam x} f_a(x) / E with f_a positive stable: E exp(-s X) =
    exp(-((s + lam)^a - lam^a)), on both sides of the regime switch at
    tilt^a = 2, exactly at it, and deep in the double rejection."""
    n = 1000000
    cases = [(a, tp) for a in C.TS_EXPONENTS
             for tp in (.5, 1.9, 2., 2.1, 4., 20., 150.)]

    def one(k):
        a, tp = cases[k]
        lam = tp ** (1 / a)
        if tp == 2.:
            assert lam ** a == 2.
        x, win = R.tilted_stable(60 + k, R.STREAM_LSCALE, a, np.full(n, lam),
                                 variant=k % 2, trace=True)
        assert np.all(x > 0) and np.all(np.isfinite(x))
        assert win.max() < 4095
        for s in (.3, 2.):
            # (s + lam)^a - lam^a without the cancellation at large lam
            want = np.exp(-tp * np.expm1(a * np.log1p(s / lam)))
            _six_sigma(np.exp(-s * x), want, (a, tp, s))

    # (the replay runs outside the interpreter lock: four cases at a time)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as pool:
        list(pool.map(one, range(len(cases))))


def test_replayed_gamma_has_the_right_law():
    for k, shape in enumerate(C.GAMMA_SHAPES):
        x = R.gamma(80 + k, R.STREAM_GSCALE, shape, n=200000)
        assert np.all(x > 0)
        assert stats.kstest(x, 'gamma', args=(shape,)).pvalue > SIX_SIGMA_P
        _six_sigma(x, shape, ('gamma mean', shape))
    # element k of a run is the generator of index k
    assert R.gamma(80, R.STREAM_GSCALE, .4, n=1, index=7)[0] == \
        R.gamma(80, R.STREAM_GSCALE, .4, n=8)[7]


# ----------------------------------- arithmetic alone, on the GPU tests' inputs

def _spread(x0, x1, same):
    ok = same & ~(np.isnan(x0) & np.isnan(x1))
    return float(np.max(np.abs(x1[ok] / x0[ok] - 1), initial=0.))


def test_variants_differ_by_rounding_only_on_the_gpu_tests_inputs():
    """Variant 0 (the reference's arithmetic) against variant 1 (the kernels'
    forms) on every input of tests/test_hip_sampler_replay.py: the share of
    draws that take another branch stays within the cap on excluded draws, and
    the largest relative difference among the rest is what
    replay_cases.tolerance() multiplies by 1000."""
    worst = 0.
    for n in C.PG_SIZES:
        shape, tilt, _ = C.pg_inputs(n)
        x0, a0, r0 = R.polya_gamma(C.PG_SEEDS[n], R.STREAM_PG, shape, tilt, 0,
                                   trace=True)
        x1, a1, r1 = R.polya_gamma(C.PG_SEEDS[n], R.STREAM_PG, shape, tilt, 1,
                                   trace=True)
        same = (a0 == a1) & (r0 == r1)
        assert (~same).sum() <= C.cap(n)
        worst = max(worst, _spread(x0, x1, same))
        print("polya-gamma n = %d: %d of %d draws took another branch, "
              "largest relative difference %.3g"
              % (n, (~same).sum(), n, _spread(x0, x1, same)))
    assert worst <= C.PG_VARIANT_SPREAD
    for a in C.TS_EXPONENTS:
        worst = 0.
        sets = [('mixed %d' % n, C.ts_mixed(a, n)) for n in (1, 255, 256, 257)]
        sets.append(('blocks', C.ts_blocks(a)))
        if a == .25:
            sets.append(('mixed %d' % C.TS_BIG, C.ts_mixed(a, C.TS_BIG)))
        for name, tilt in sets:
            x0, w0 = R.tilted_stable(9, R.STREAM_LSCALE, a, tilt, 0, trace=True)
            x1, w1 = R.tilted_stable(9, R.STREAM_LSCALE, a, tilt, 1, trace=True)
            same = w0 == w1
            assert (~same).sum() <= C.cap(len(tilt)), (a, name)
            worst = max(worst, _spread(x0, x1, same))
            print("tilted stable a = %g %s: %d of %d draws took another "
                  "candidate, largest relative difference %.3g"
                  % (a, name, (~same).sum(), len(tilt), _spread(x0, x1, same)))
        assert worst <= C.TS_VARIANT_SPREAD[a], (a, worst)
        assert worst >= .5 * C.TS_VARIANT_SPREAD[a], (a, worst)  # not padded
    assert C.tolerance(0.) == 1e-12


def test_a_perturbed_linear_predictor_moves_the_draws_by_as_much():
    """The chain-level pin recomputes psi = X~ beta with the oracle's design:
    a summation order of its own, |psi_device - psi_oracle| <=
    replay_cases.CHAIN_PSI_DELTA max(1, |psi|).  How far that moves a
    Polya-Gamma draw, and how many draws it sends down another branch: the
    tolerance of the chain-level Omega check adds 100 x the former."""
    n = 50000
    shape, tilt, bad = C.pg_inputs(n)
    tilt[bad] = 1.
    rng = np.random.default_rng(2)
    moved = tilt + C.CHAIN_PSI_DELTA * np.maximum(1., np.abs(tilt)) * \
        rng.choice([-1., 1.], n)
    x0, a0, r0 = R.polya_gamma(1, R.STREAM_PG, shape, tilt, 0, trace=True)
    x1, a1, r1 = R.polya_gamma(1, R.STREAM_PG, shape, moved, 0, trace=True)
    same = (a0 == a1) & (r0 == r1)
    change = _spread(x0, x1, same)
    print("psi +- %.1e max(1, |psi|): %d of %d draws took another branch, "
          "largest relative change %.3g"
          % (C.CHAIN_PSI_DELTA, (~same).sum(), n, change))
    assert (~same).sum() <= C.cap(n)
    assert .5 * C.CHAIN_OMEGA_CHANGE <= change <= C.CHAIN_OMEGA_CHANGE
