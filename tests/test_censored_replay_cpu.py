"""CPU: the host replay of the censored-outcome model's latent draw
(bayesbridge_amd.replay.censored_normal on replay.truncated_normal) -- its
conventions, its distribution, the measurements that give
tests/test_hip_censored.py its tolerances (tests/censored_cases.py) -- and the
NumPy oracle against itself."""
import math

import numpy as np
import pytest
from scipy import stats

import censored_cases as K
import censored_oracle as O
import probit_cases as P
import replay_cases as C
from bayesbridge_amd import replay as R


def test_observed_rows_copy_and_censored_rows_keep_their_side():
    for case in K.CN_CASES:
        psi, bound, status, bad = K.cn_inputs(case)
        tau = case[3]
        for variant in (0, 1):
            z, trials = R.censored_normal(K.CN_SEEDS[case], R.STREAM_LATENT,
                                          psi, bound, status, tau, variant,
                                          trace=True)
            obs = status == 0
            assert np.array_equal(z[obs], bound[obs])
            assert np.all(trials[obs] == 0)
            ok = np.isfinite(psi)
            assert np.all(z[ok & (status == 1)] > bound[ok & (status == 1)])
            assert np.all(z[ok & (status == 2)] <= bound[ok & (status == 2)])
            cens_bad = bad[status[bad] != 0]
            assert np.all(np.isnan(z[cens_bad]))
            assert np.all(trials[cens_bad] == 0)
            assert np.all(trials[ok & ~obs] >= 1)
        if case[0] >= 255:
            # a third of the rows per status, the planted values with both
            # censored statuses, the non-finite psi with every status
            share = np.bincount(status, minlength=3) / len(status)
            assert np.all(np.abs(share - 1. / 3.) < .1)
            a = (bound - psi) * math.sqrt(tau)
            for s in (1, 2):
                for v in K.CN_PLANTED:
                    hit = (status == s) & (np.abs(a - v)
                                           <= 1e-9 * max(1., abs(v)))
                    assert hit.sum() >= (2 if case[0] >= 600 else 1), (s, v)
            assert sorted(status[bad][:3]) == [0, 1, 2]


@pytest.mark.parametrize("status", (1, 2))
@pytest.mark.parametrize("tau", (.25, 9.))
@pytest.mark.parametrize("a", (-2., 0., .5, 3.))
def test_the_replay_draws_the_truncated_normal_at_precision_tau(a, tau,
                                                                status):
    """Mean and variance of 2e5 draws against the exact ones of N(psi, 1 /
    tau) beyond b (status 1) or up to b (status 2), with a the distance of the
    bound into the allowed side's tail in standard deviations: |z| < 4.5."""
    n = 200000
    s = 1. if status == 1 else -1.
    b = 1.7
    psi = np.full(n, b - s * a / math.sqrt(tau))
    z = R.censored_normal(5 + status, R.STREAM_LATENT, psi, np.full(n, b),
                          np.full(n, status), tau)
    excess = s * (z - b) * math.sqrt(tau)       # x - a >= 0, x standardised
    assert np.all(excess >= 0.)
    m = math.exp(stats.norm.logpdf(a) - stats.norm.logsf(a))
    var = 1. + a * m - m * m
    mean_hat, var_hat = excess.mean(), excess.var()
    mu4 = np.mean((excess - mean_hat) ** 4)
    z_mean = (mean_hat - (m - a)) / math.sqrt(var / n)
    z_var = (var_hat - var) / math.sqrt((mu4 - var_hat ** 2) / n)
    print("a %g tau %g status %d: z of the mean %.2f, of the variance %.2f"
          % (a, tau, status, z_mean, z_var))
    assert abs(z_mean) < 4.5 and abs(z_var) < 4.5


def test_variant_spread_is_the_recorded_one():
    """Variant 0 against variant 1 over the inputs of censored_cases.py, with
    the recorded seeds: the three conditions of CN_SEEDS hold and the largest
    difference is CN_VARIANT_SPREAD."""
    worst, n_draw, searched = 0., 0, {}
    for case in K.CN_CASES:
        seed = K.CN_SEEDS[case]
        differ, spread, low, high, margin = K.conditions(case, seed)
        print("%s, seed %d: %d draws differ in trials, spread %.3g, most "
              "trials %d (plain) %d (exponential), margin of the small "
              "planted a %.3g" % (K.case_id(case), seed, differ, spread, low,
                                  high, margin))
        assert differ <= C.cap(case[0]) and differ == 0
        assert K.holds(case, seed)
        if case[0] < 1000:
            assert seed == K.search_seed(case)
        worst = max(worst, spread)
        n_draw += case[0]
    assert n_draw == 1575186
    assert .5 * K.CN_VARIANT_SPREAD <= worst <= K.CN_VARIANT_SPREAD
    assert K.CN_TOL == max(1000. * K.CN_VARIANT_SPREAD, 1e-12)


def test_the_largest_case_has_the_smallest_seed_that_holds():
    for case in K.CN_CASES:
        if case[0] >= 1000:
            assert K.CN_SEEDS[case] == 1 and K.holds(case, 1)


def test_a_perturbed_linear_predictor_moves_the_latents_by_as_much():
    """The chain-level check recomputes psi with the oracle's design: how far
    a CHAIN_PSI_DELTA perturbation moves a draw, and how many it sends down
    another branch (the tolerance of the latent check adds 100 x the former)."""
    n = 50000
    psi, bound, status, bad = K.cn_inputs((n, -1, 0, 1.))
    psi[bad] = 1.
    rng = np.random.default_rng(2)
    moved = psi + C.CHAIN_PSI_DELTA * np.maximum(1., np.abs(psi)) * \
        rng.choice([-1., 1.], n)
    z0, t0 = R.censored_normal(1, R.STREAM_LATENT, psi, bound, status, 1., 0,
                               True)
    z1, t1 = R.censored_normal(1, R.STREAM_LATENT, moved, bound, status, 1.,
                               0, True)
    pos = status == 1
    same = (t0 == t1) & (P.regime(K.scaled(psi, bound, 1.), pos)
                         == P.regime(K.scaled(moved, bound, 1.), pos))
    change = float(K.difference(z1, z0, psi, bound, status, 1.)[same].max())
    print("psi +- %.1e max(1, |psi|): %d of %d draws took another branch, "
          "largest change %.3g" % (C.CHAIN_PSI_DELTA, (~same).sum(), n, change))
    assert (~same).sum() <= C.cap(n)
    assert .5 * K.CHAIN_LATENT_CHANGE <= change <= K.CHAIN_LATENT_CHANGE


def test_sum_orders_of_the_right_hand_side_agree_to_the_recorded_spread():
    """X~^T y summed row after row against NumPy's pairwise sum of each
    column, on the data of the no-censored-row test: what its tolerance is
    1000 x of."""
    X, y = K.linear_problem()
    Xt = np.hstack([np.ones((len(y), 1)), X - X.mean(axis=0)])
    terms = Xt * y[:, None]
    one = np.add.reduce(terms, axis=0)                      # row after row
    other = np.ascontiguousarray(terms.T).sum(axis=1)       # pairwise
    spread = float(np.abs(one - other).max() / np.abs(one).max())
    print("X~^T y in two orders: %.3g of the largest entry" % spread)
    assert .2 * K.RHS_ORDER_SPREAD <= spread <= K.RHS_ORDER_SPREAD
    assert K.RHS_ORDER_TOL == max(1000. * K.RHS_ORDER_SPREAD, 1e-12)


def test_nonfinite_inputs_give_nan_and_no_trial():
    psi = np.array([np.nan, np.inf, -np.inf, 1e308, 0.])
    bound = np.array([0., 1., 2., -1e308, 3.])
    for variant in (0, 1):
        z, t = R.censored_normal(1, R.STREAM_LATENT, psi, bound,
                                 [1, 2, 1, 1, 2], 4., variant, trace=True)
        # (the fourth: psi - b overflows, psi' is not finite)
        assert np.all(np.isnan(z[:4])) and np.all(t[:4] == 0)
        assert z[4] <= 3. and t[4] >= 1
        z = R.censored_normal(1, R.STREAM_LATENT, psi, bound, np.zeros(5), 4.,
                              variant)
        assert np.array_equal(z, bound)


def test_the_oracle_agrees_with_itself_and_recovers_the_planted_slopes():
    """A sanity check of the yardstick: two runs of the NumPy chain on one
    censored problem, compared by batch-means z-scores; and the slopes it finds
    are the planted ones where the bounds taken as observed are not."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((300, 6))
    beta = np.array([1., -1., .5, 0., 0., 0.])
    z = .3 + X @ beta + rng.standard_normal(300)
    status = (z > .5).astype(np.uint8)
    bound = np.where(status == 1, .5, z)
    ora = O.CensoredOracle(bound, status, X)
    a, b = (ora.run(3000, 500, seed) for seed in (1, 2))
    zs = O.z_scores([a], [b])
    print("oracle against itself: largest z %.2f" % zs.max())
    assert zs.shape == (16,) and zs.max() < 4.5
    naive = O.CensoredOracle(bound, np.zeros(300, dtype=np.uint8), X) \
        .run(3000, 500, 3)
    err = np.abs(a.mean(axis=0)[1:4] - beta[:3]).max()
    err_naive = np.abs(naive.mean(axis=0)[1:4] - beta[:3]).max()
    print("slopes: error %.3f, with the bounds taken as observed %.3f"
          % (err, err_naive))
    assert err < .25 and err_naive > .3


def test_oracle_loglik_is_the_sum_of_its_parts():
    rng = np.random.default_rng(4)
    psi, b = rng.normal(0., 2., 50), rng.normal(0., 2., 50)
    status = rng.integers(0, 3, 50)
    tau = 2.5
    a = (b - psi) * math.sqrt(tau)
    want = np.where(status == 0, .5 * math.log(tau) - .5 * a * a,
                    np.where(status == 1, stats.norm.logsf(a),
                             stats.norm.logcdf(a))).sum()
    assert abs(O.loglik(psi, b, status, tau) - want) <= 1e-12 * abs(want)
