"""CPU: what the GPU test of the quantile model's mixing weights relies on --
the replayed inverse-Gaussian draw follows its law (Kolmogorov-Smirnov against
scipy, both branches taken), the measured CHAIN_WEIGHT_CHANGE of
tests/quantile_cases.py, that no draw on the test's inputs can change its
branch between device and replay (so the GPU test uses cap 0), the
augmentation itself against a Metropolis chain on the marginal posterior with
a negative control, and the stream constants.  The density test and the
augmentation test exercise the NumPy oracle alone: they check the model that
the library implements, not the library, and pass without it.  No GPU."""
import numpy as np
import pytest

import replay_cases as C
import quantile_cases as K
import quantile_oracle as O
from bayesbridge_amd import replay as R


def test_stream_constants():
    assert R.STREAM_QMIX == 9 and R.STREAM_MIX == 8 and R.STREAM_OBSVAR == 6
    assert R.iter_stream(R.STREAM_QMIX, 2) == 9 | 2 << 8
    # the stream of a chain that has not run: iteration -1
    assert R.iter_stream(R.STREAM_QMIX, -1) == 0xFFFFFFFFFFFFFF09


@pytest.mark.parametrize("lam", (.7, 9.))
@pytest.mark.parametrize("m", (0., 1e-3, .5, 30.))
def test_the_replayed_draw_follows_its_law(m, lam):
    """InverseGaussian(mean 1 / m, shape lam), Levy's law at m = 0, by
    Kolmogorov-Smirnov on 400 000 draws of a fixed seed."""
    from scipy import stats
    n = 400000
    w, branch = R.inverse_gaussian(101, R.STREAM_QMIX, np.full(n, m), lam,
                                   trace=True)
    assert np.all(np.isfinite(w)) and np.all(w > 0.)
    if m == 0.:
        law = stats.levy(scale=lam)
        assert not branch.any()          # u <= 1: always the one root
    else:
        mean = 1. / m
        law = stats.invgauss(mean / lam, scale=lam)
        # both roots are taken: the other with probability E[m x / (1 + m x)]
        assert 0 < branch.sum() < n
    p = stats.kstest(w, law.cdf).pvalue
    print("m %g lambda %g: KS p %.3g, other root %d of %d"
          % (m, lam, p, branch.sum(), n))
    assert p > 1e-3
    # variant 1 is variant 0, and a draw is a function of its counters
    assert np.array_equal(
        w[:9], R.inverse_gaussian(101, R.STREAM_QMIX, np.full(9, m), lam, 1))


def test_extreme_arguments_give_finite_positive_weights():
    m = np.array([0., 1e-300, 1e-8, 1e150, .25e150])
    for seed in range(20):
        w = R.inverse_gaussian(seed, R.STREAM_QMIX, m, 1.3)
        assert np.all(np.isfinite(w)) and np.all(w > 0.), (seed, w)
    with pytest.raises(ValueError):
        R.inverse_gaussian(1, R.STREAM_QMIX, m, 0.)


def _rel(a, b):
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(a - b) / np.abs(b)
    rel[a == b] = 0.
    return rel


@pytest.mark.parametrize("q", K.QUANTILES)
def test_weight_change_is_the_measured_one_and_no_draw_can_change_branch(q):
    stream = R.iter_stream(R.STREAM_QMIX, K.ITERATION)
    worst, closest = 0., np.inf
    for n in K.SIZES:
        X, _, psi, y, where = K.weight_inputs(n)
        w, branch, margin = K.replayed(stream, psi, y, q)
        assert np.all(np.isfinite(w)) and np.all(w > 0.)
        closest = min(closest, float(np.abs(margin - 1.).min()))
        for s in (-1., 1.):
            moved = psi + s * C.CHAIN_PSI_DELTA * np.maximum(1., np.abs(psi))
            w2, branch2, margin2 = K.replayed(stream, moved, y, q)
            closest = min(closest, float(np.abs(margin2 - 1.).min()))
            # no draw changes its branch, so every weight stays within the
            # tolerance: cap 0 is the condition
            assert np.array_equal(branch, branch2)
            rel = _rel(w2, w)
            worst = max(worst, float(rel.max()))
            assert int((~(rel <= K.WEIGHT_TOL[q])).sum()) == K.WEIGHT_CAP == 0
        if n >= 255:
            r = np.array(K.PLANTED + K.PLANTED)
            big = w[where][np.abs(r) == 1e150]
            assert np.all(big > 0.) and np.all(np.isfinite(big))
            # at r = 0: Levy's law, always the one root
            assert not branch[where][r == 0.].any()
    print("q %g: largest relative change of a weight %.3g, closest "
          "u (1 + m x) to 1: %.3g" % (q, worst, closest))
    assert closest > K.BRANCH_MARGIN
    assert .5 * K.CHAIN_WEIGHT_CHANGE[q] <= worst <= K.CHAIN_WEIGHT_CHANGE[q]
    assert K.WEIGHT_TOL[q] == C.GAMMA_TOL + K.CHAIN_WEIGHT_CHANGE[q]


def test_loglik_is_the_asymmetric_laplace_density():
    """Against the mixture integrated numerically: int_0^inf Exp(v; rate tau)
    N(y; psi + theta v, kappa2 v / tau) dv."""
    from scipy import integrate, stats
    for q in K.QUANTILES:
        qq, theta, kappa2 = O.level(q)
        tau = 1.3
        for r in (-2., -.1, .4, 3.):
            dens = integrate.quad(
                lambda v: tau * np.exp(-tau * v) * stats.norm.pdf(
                    r, theta * v, np.sqrt(kappa2 * v / tau)), 0., np.inf,
                epsabs=0., epsrel=1e-11, limit=400)[0]
            want = O.loglik(np.zeros(1), np.array([r]), tau, q)
            assert abs(np.log(dens) - want) < 1e-8, (q, r)


_aug = {}


def _augmentation_reference():
    if not _aug:
        X, y, q, sd = O.augmentation_problem()
        _aug['problem'] = (X, y, q, sd)
        _aug['mh'] = [O.metropolis(y, X, q, sd, 220000, 20000, 50 + k)[0]
                      for k in range(2)]
    return _aug['problem'], _aug['mh']


def test_the_augmented_chain_draws_the_marginal_posterior():
    """The Gibbs oracle (beta by Cholesky, tau, w) against random-walk
    Metropolis on the marginal asymmetric-Laplace posterior of (beta, log tau):
    every coefficient's mean and variance, and tau's, at batch-means |z| < 4.5;
    the same oracle with theta = 0 fails it."""
    (X, y, q, sd), mh = _augmentation_reference()
    gibbs = [O.QuantileOracle(y, X, q, fixed_sd=sd).run(21000, 1000, 7 + k)
             for k in range(2)]
    z = O.z_scores(gibbs, mh)
    print("augmentation: largest z %.2f (moment %d)" % (z.max(), z.argmax()))
    assert z.shape == (10,) and np.all(np.isfinite(z))
    assert z.max() < 4.5
    wrong = [O.QuantileOracle(y, X, q, fixed_sd=sd, theta_zero=True)
             .run(21000, 1000, 7 + k) for k in range(2)]
    z0 = O.z_scores(wrong, mh)
    print("theta = 0 control: largest z %.2f" % z0.max())
    assert z0.max() > 4.5
