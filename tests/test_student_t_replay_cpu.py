"""CPU: what the GPU test of the Student-t model's mixing weights relies on --
the measured CHAIN_WEIGHT_CHANGE of tests/student_t_cases.py against its
analytic bound, that the replay alone excludes no draw on the test's inputs
(so the GPU test uses cap 0), the oracle chain recovering planted slopes on
contaminated data where a Gaussian fit does not, and the stream constants.
No GPU."""
import numpy as np
import pytest

import replay_cases as C
import student_t_cases as K
import student_t_oracle as O
from bayesbridge_amd import replay as R


def test_stream_constants():
    assert R.STREAM_MIX == 8 and R.STREAM_OBSVAR == 6
    assert R.iter_stream(R.STREAM_MIX, 2) == 8 | 2 << 8
    # the stream of a chain that has not run: iteration -1
    assert R.iter_stream(R.STREAM_MIX, -1) == 0xFFFFFFFFFFFFFF08


@pytest.mark.parametrize("nu", K.DFS)
def test_weight_change_is_the_measured_one_and_within_its_bound(nu):
    worst = 0.
    for n in K.SIZES:
        X, _, psi, y, where = K.weight_inputs(n)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(psi))
        if n >= 255:
            # the planted residuals as the device's subtraction sees them
            r = (y - psi)[where]
            want = np.array(K.PLANTED + K.PLANTED)
            assert np.all(np.abs(r - want) <= 2e-15 * np.maximum(
                np.abs(want), np.abs(psi[where])))
            assert np.all(r[want == 0.] == 0.)
        change = K.weight_change(psi, y, K.TAU, nu)
        # (2^-52: the rounding of the measurement's own division)
        assert change <= K.weight_change_bound(psi, K.TAU, nu) + 2. ** -52, n
        worst = max(worst, change)
    print("nu %g: largest relative change of a weight %.3g" % (nu, worst))
    assert .5 * K.CHAIN_WEIGHT_CHANGE[nu] <= worst <= K.CHAIN_WEIGHT_CHANGE[nu]
    assert K.WEIGHT_TOL[nu] == C.GAMMA_TOL + K.CHAIN_WEIGHT_CHANGE[nu]


@pytest.mark.parametrize("nu", K.DFS)
def test_the_replay_alone_excludes_no_draw(nu):
    """The Gamma variate branches on (seed, stream, row, nu) alone: weights
    replayed from psi and from psi moved by the product's rounding share it, so
    every one of them stays within the tolerance and cap 0 is the condition."""
    stream = R.iter_stream(R.STREAM_MIX, K.ITERATION)
    for n in K.SIZES:
        X, _, psi, y, where = K.weight_inputs(n)
        g = R.gamma(K.SEED, stream, (nu + 1.) / 2., n)
        assert np.all(np.isfinite(g)) and np.all(g > 0.)
        w = O.weights(g, psi, y, K.TAU, nu)
        assert np.all(np.isfinite(w)) and np.all(w >= 0.)
        for s in (-1., 1.):
            moved = psi + s * C.CHAIN_PSI_DELTA * np.maximum(1., np.abs(psi))
            w2 = O.weights(g, moved, y, K.TAU, nu)
            with np.errstate(invalid='ignore', divide='ignore'):
                rel = np.abs(w2 - w) / np.abs(w)
            rel[w2 == w] = 0.
            assert int((~(rel <= K.WEIGHT_TOL[nu])).sum()) == K.WEIGHT_CAP == 0
        # the same rows again: the draw is a function of its counters
        assert np.array_equal(
            g[:7], R.gamma(K.SEED, stream, (nu + 1.) / 2., min(n, 7)))
        if n > 300:
            assert np.array_equal(
                g[300:305], R.gamma(K.SEED, stream, (nu + 1.) / 2., 5, 300))
    # shape 0.75 < 1 takes gamma_draw's boost: one more uniform, another draw
    if nu == .5:
        assert not np.array_equal(R.gamma(K.SEED, stream, .75, 4),
                                  R.gamma(K.SEED, stream, 1.75, 4))


def test_weights_follow_their_conditional():
    """omega_i (nu + tau r_i^2) / 2 ~ Gamma((nu+1)/2): mean and variance of
    the replayed variates over 524 289 rows."""
    for nu in K.DFS:
        a = (nu + 1.) / 2.
        g = R.gamma(K.SEED, R.iter_stream(R.STREAM_MIX, 0), a, 524289)
        se = np.sqrt(a / g.size)
        assert abs(g.mean() - a) < 4.5 * se
        # Var = a; Var of (g - a)^2 = 2 a^2 + 6 a
        assert abs(g.var() - a) < 4.5 * np.sqrt((2 * a * a + 6 * a) / g.size)


def test_loglik_tends_to_the_linear_models():
    rng = np.random.default_rng(0)
    psi, y = rng.standard_normal(50), rng.standard_normal(50)
    tau = 1.3
    lin = 50 * np.log(tau) / 2 - tau * np.sum((y - psi) ** 2) / 2
    assert abs(O.loglik(psi, y, tau, 1e9) - lin) < 1e-6 * abs(lin)
    # and is the t-density: against scipy, with the dropped constant put back
    from scipy.stats import t
    full = np.sum(t.logpdf((y - psi) * np.sqrt(tau), 4.)) + 25 * np.log(tau)
    assert abs(O.loglik(psi, y, tau, 4.) - 25 * np.log(2 * np.pi) - full) \
        < 1e-12 * abs(full)


def test_oracle_recovers_planted_slopes_where_a_gaussian_fit_does_not():
    """The posterior test's data (10 % of the rows contaminated with a shift
    along the first column): the Student-t oracle's posterior mean of the first
    slope stays near the planted 1.2, the linear oracle's is dragged by ~0.6;
    and the scale of the clean noise is recovered."""
    X, y, beta = O.contaminated_problem(K.POSTERIOR_DATA_SEED)
    t_draws = O.StudentTOracle(y, X, 4.).run(1500, 300, 1)
    lin_draws = O.StudentTOracle(y, X, None).run(1500, 300, 1)
    t_mean, lin_mean = t_draws.mean(axis=0), lin_draws.mean(axis=0)
    print("student_t", np.round(t_mean, 3), "\nlinear   ", np.round(lin_mean, 3))
    t_sd = t_draws.std(axis=0)
    assert np.all(np.abs(t_mean[1:13] - beta) < 4. * t_sd[1:13] + .05)
    assert abs(t_mean[1] - 1.2) < .25 < .5 < abs(lin_mean[1] - 1.2)
    assert .5 < t_mean[13] < 1.6 and lin_mean[13] < .15
