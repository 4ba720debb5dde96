"""CPU: the Cox model's host side -- the NumPy oracle against the reference's
fixtures and the brute-force definition (a tied latest event time included,
where the reference fails), the vectorised preprocessing against the
reference's, the sampler-option rules of the Cox model, and the register
budget of the kernels in csrc/cox.hip (no spills, no scratch)."""
import os
import warnings

import numpy as np
import pytest

import cox_cases as cc
import cox_oracle as co
from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table


def _fixture(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _risk(p):
    return (int(p['n_event']), p['start'], p['end'], p['n_app'])


def test_oracle_matches_reference_likelihood(golden_dir):
    """Tie-free event times: with tied events the reference sums risk set k
    from k instead of start_k (see make_cox_golden.py)."""
    from bayesbridge_amd.model import cox_risk_sets
    g = _fixture(golden_dir, 'cox_likelihood.npz')
    X, risk = g['X'], cox_risk_sets(g['event_time'], g['censoring_time'])
    for k in range(len(g['beta'])):
        ll, grad = co.loglik_grad(X, g['beta'][k], *risk)
        assert ll == pytest.approx(g['loglik'][k], rel=1e-12)
        np.testing.assert_allclose(grad, g['grad'][k], rtol=1e-10,
                                   atol=1e-10 * np.abs(g['grad'][k]).max())
        hv = co.hessian_matvec(X, g['beta'][k], g['v'][k], *risk)
        np.testing.assert_allclose(hv, g['hessian_matvec'][k], rtol=1e-9,
                                   atol=1e-10 * np.abs(hv).max())


def _check_against_brute(X, risk, betas, vs):
    n_event, start, end, n_app = risk
    for beta, v in zip(betas, vs):
        ll, grad = co.loglik_grad(X, beta, *risk)
        bl, bg = co.brute_loglik_grad(X, beta, n_event, start, end)
        assert ll == pytest.approx(bl, rel=1e-12)
        np.testing.assert_allclose(grad, bg, rtol=1e-9,
                                   atol=1e-11 * np.abs(bg).max())
        hv = co.hessian_matvec(X, beta, v, *risk)
        bh = co.brute_hessian_matvec(X, beta, v, n_event, start, end)
        np.testing.assert_allclose(hv, bh, rtol=1e-9,
                                   atol=1e-11 * np.abs(bh).max())


def _tied_last_event(n=60, p=5, seed=4):
    rs = np.random.RandomState(seed)
    event = np.round(rs.exponential(1., n), 1)
    cens = np.full(n, np.inf)
    c = rs.rand(n) < .3
    cens[c] = np.round(rs.exponential(1., c.sum()), 1) + 10.
    event[c] = np.inf
    top = event[np.isfinite(event)].max()
    event[np.flatnonzero(np.isfinite(event))[:3]] = top   # three-way tie, last
    return event, cens, rs.randn(n, p)


def test_oracle_matches_brute_force_including_a_tied_last_event(golden_dir):
    p = _fixture(golden_dir, 'cox_preprocess.npz')
    rs = np.random.RandomState(0)
    _check_against_brute(p['sorted_X'], _risk(p),
                         rs.randn(3, p['sorted_X'].shape[1]),
                         rs.randn(3, p['sorted_X'].shape[1]))
    from bayesbridge_amd.model import cox_preprocess, cox_risk_sets
    event, cens, X = _tied_last_event()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        et, ct, Xs, _ = cox_preprocess(event, cens, X)
    risk = cox_risk_sets(et, ct)
    n_event, start, end, _ = risk
    n_tied = np.sum(et[:n_event] == et[n_event - 1])
    assert n_tied >= 3 and start[-1] == n_event - n_tied
    _check_against_brute(Xs, risk, rs.randn(3, X.shape[1]),
                         rs.randn(3, X.shape[1]))


def test_vectorised_preprocessing_equals_the_reference(golden_dir):
    from bayesbridge_amd.model import cox_preprocess, cox_risk_sets
    p = _fixture(golden_dir, 'cox_preprocess.npz')
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        et, ct, Xs, keep = cox_preprocess(p['event_time'], p['censoring_time'],
                                          p['X'])
    assert len(w) == 2          # sorted, and uninformative rows removed
    np.testing.assert_array_equal(et, p['sorted_event_time'])
    np.testing.assert_array_equal(ct, p['sorted_censoring_time'])
    np.testing.assert_array_equal(Xs, p['sorted_X'])
    np.testing.assert_array_equal(p['X'][keep], p['sorted_X'])
    n_event, start, end, n_app = cox_risk_sets(et, ct)
    assert n_event == int(p['n_event'])
    for a, b in ((start, 'start'), (end, 'end'), (n_app, 'n_app')):
        np.testing.assert_array_equal(a, p[b])


@pytest.mark.parametrize('seed', range(5))
def test_vectorised_risk_sets_equal_the_loops(seed):
    from bayesbridge_amd.model import cox_preprocess, cox_risk_sets
    rs = np.random.RandomState(seed)
    n = 300
    event = np.round(rs.exponential(1., n), 1)      # many ties
    cens = np.full(n, np.inf)
    c = rs.rand(n) < .5
    cens[c] = np.round(rs.exponential(1., c.sum()), 1)
    event[c] = np.inf
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        et, ct, _, _ = cox_preprocess(event, cens, None)
    got = cox_risk_sets(et, ct)
    want = co.risk_sets_by_loops(et, ct)
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(a, b)


def test_unsorted_rows_are_refused_by_the_risk_sets():
    from bayesbridge_amd.model import cox_risk_sets
    with pytest.raises(ValueError):
        cox_risk_sets(np.array([2., 1., np.inf]), np.array([np.inf] * 2 + [1.]))
    from bayesbridge_amd.model import cox_sort_permutation
    with pytest.raises(ValueError):
        cox_sort_permutation(np.array([1., np.inf]), np.array([np.inf, np.inf]))


# (ne, n_cens) at the scans' partition edges: one chunk element, ragged and
# empty trailing chunks (255, 257, 2047, 2049 = 256 * 8 + 1), exact chunks
BUILDER_SIZES = [(1, 0), (2, 1), (3, 0), (1, 2), (255, 2), (256, 1),
                 (257, 256), (2047, 0), (2048, 2049), (2049, 2047)]


def _builder_case(ne, n_cens, values='normal'):
    b = cc.event_boundaries(ne)
    hot = [b[len(b) // 2] if len(b) else 0] + ([ne] if n_cens else [])
    return cc.cox_case(ne, n_cens, values=values, hot=hot)


@pytest.mark.parametrize('ne,n_cens', BUILDER_SIZES)
def test_case_builder_risk_sets_equal_the_loops(ne, n_cens):
    from bayesbridge_amd.model import cox_risk_sets, cox_sort_permutation
    case = _builder_case(ne, n_cens)
    et, ct = case.event_time, case.censoring_time
    assert cox_sort_permutation(et, ct) is None
    assert not np.any(ct < np.min(et))        # nothing for preprocess to drop
    got = cox_risk_sets(et, ct)
    want = co.risk_sets_by_loops(et, ct)
    assert got[0] == want[0] == ne
    for a, b in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('ne,n_cens', BUILDER_SIZES + [(524289, 1)])
def test_case_builder_places_ties_and_hot_rows(ne, n_cens):
    from bayesbridge_amd.model import cox_risk_sets
    case = _builder_case(ne, n_cens)
    et = case.event_time[:ne]
    # the chunk and tile boundaries of the event scans, forward and reversed
    L = cc.chunk_len(ne)
    bounds = cc.event_boundaries(ne)
    assert set(bounds) == {t for t in range(1, ne) if t % L == 0
                           or (t % L) % cc.SCAN_TILE == 0
                           or (ne - t) % L == 0
                           or ((ne - t) % L) % cc.SCAN_TILE == 0}
    runs = cc.tie_runs(ne)
    if L > 8:                                  # every boundary inside a run
        assert np.all(et[bounds - 1] == et[bounds])
    for a, b in runs:
        assert a < b and np.all(et[a:b] == et[a])
    if ne >= 255:
        assert len(np.unique(et)) > ne // 5    # runs, not one big tie
    _, start, end, _ = cox_risk_sets(case.event_time, case.censoring_time)
    if n_cens:
        ct = case.censoring_time[ne:]
        assert ct[0] == et[-1]
        assert np.any(np.isin(ct, et))         # a censored time tied
        if n_cens > 100:
            assert np.any(~np.isin(ct, et))
        if np.any(et < et[-1]) and n_cens > 1:
            assert np.any(end == ne)
    eta = case.X @ case.beta
    np.testing.assert_allclose(eta[case.hot], eta.max(), rtol=1e-12)
    rest = np.setdiff1d(np.arange(ne + n_cens), case.hot)
    if len(rest):
        assert eta[rest].max() < eta.max() - .5
    assert case.hot[0] in bounds or ne == 1
    # sparse hot rows: the columns with beta > 0
    sp = _builder_case(ne, n_cens, 'binary') if ne < 10000 else None
    if sp is not None:
        e2 = sp.X @ sp.beta
        assert np.all(e2[sp.hot] == np.sum(np.maximum(sp.beta, 0)))
        assert np.all(e2 <= e2[sp.hot[0]])


def test_steep_case_spans_1e30_across_tiles():
    case = cc.steep_case(1048577, 1)
    from bayesbridge_amd.model import cox_risk_sets
    risk = cox_risk_sets(case.event_time, case.censoring_time)
    eta = case.X @ case.beta
    inv_H = 1. / co.risk_sums(np.exp(eta - eta.max()), *risk[:3])
    L = cc.chunk_len(risk[0])
    assert L > cc.SCAN_TILE
    assert inv_H.max() / inv_H.min() > 1e30
    # somewhere, 8 consecutive events see 1/H grow by more than 2^53
    assert np.max(inv_H[8:] / inv_H[:-8]) > 2. ** 53 * 1e3


@pytest.mark.parametrize('ne,n_cens', BUILDER_SIZES)
@pytest.mark.parametrize('values', ['normal', 'binary', 'valued'])
def test_extended_reference_bounds_the_float64_oracle(ne, n_cens, values):
    """The float64 oracle (sequential cumsums) lies within EDGE_TOL times the
    componentwise bound of the extended-precision reference; the two faults
    the GPU tests must see -- a hot row at a scan boundary dropped from its
    risk sets, end_k > ne for end_k >= ne -- lie 100 x EDGE_TOL beyond it."""
    from bayesbridge_amd.model import cox_risk_sets
    case = _builder_case(ne, n_cens, values)
    risk = cox_risk_sets(case.event_time, case.censoring_time)
    X = case.X.toarray() if values != 'normal' else case.X
    rs = np.random.RandomState(1)
    for scale in (.1, 1., 3.):
        beta = case.beta * scale
        v = rs.randn(len(beta))
        ll, grad = co.loglik_grad(X, beta, *risk)
        el, eg, lb, gb = co.loglik_grad_ext(case.X, beta, *risk)
        assert abs(ll - el) <= co.EDGE_TOL * lb
        assert np.all(np.abs(grad - eg) <= co.EDGE_TOL * gb)
        hv = co.hessian_matvec(X, beta, v, *risk)
        eh, hb = co.hessian_matvec_ext(case.X, beta, v, *risk)
        assert np.all(np.abs(hv - eh) <= co.EDGE_TOL * hb)
        if ne == 1 and n_cens == 0:
            continue            # grad == 0 exactly: nothing to perturb
        far = co.distance_in_tolerances(
            co.loglik_grad_ext(case.X, beta, *risk, drop=case.hot[0]),
            (el, eg, lb, gb))
        assert far > 100.
        if np.any(risk[2] == ne):
            far = co.distance_in_tolerances(
                co.loglik_grad_ext(case.X, beta, *risk, strict_end=True),
                (el, eg, lb, gb))
            assert far > 100.


class _Design:
    shape = (50, 5)
    use_hip = True
    is_sparse = True


def test_cox_options_fall_back_to_hmc_with_the_reference_stream():
    from bayesbridge_amd import SamplerOptions
    opt = SamplerOptions.pick_default_and_create(None, None, 'cox', _Design())
    assert opt.coef_sampler_type == 'hmc' and opt.rng == 'reference'
    for other in ('cg', 'cholesky'):
        with pytest.warns(UserWarning, match='Will use HMC'):
            opt = SamplerOptions.pick_default_and_create(other, None, 'cox',
                                                         _Design())
        assert opt.coef_sampler_type == 'hmc'
    with pytest.raises(ValueError):
        SamplerOptions.pick_default_and_create('hmc', {'rng': 'device'}, 'cox',
                                               _Design())
    with pytest.raises(ValueError):
        SamplerOptions(coef_sampler_type='hmc', rng='device')
    again = SamplerOptions.pick_default_and_create(None, opt.get_info(), 'cox',
                                                   _Design())
    assert again.get_info() == opt.get_info()


def test_linear_and_logit_still_refuse_hmc():
    from bayesbridge_amd import SamplerOptions
    for family in ('linear', 'logit'):
        with pytest.raises(ValueError):
            SamplerOptions.pick_default_and_create('hmc', None, family,
                                                   _Design())
        opt = SamplerOptions.pick_default_and_create(None, None, family,
                                                     _Design())
        assert opt.coef_sampler_type == 'cg' and opt.rng == 'device'


def test_step_size_adapter_and_direction_summary():
    """stepsize_adapter.py / reg_coef_posterior_summarizer.py restated: the
    adapter's first steps and the sign-aligned running direction."""
    from bayesbridge_amd.hmc import (DirectionSummarizer,
                                     HamiltonianBasedStepsizeAdapter)
    a = HamiltonianBasedStepsizeAdapter(init_stepsize=.3,
                                        target_accept_prob=.95)
    assert a.get_current_stepsize() == pytest.approx(.3)
    a.adapt_stepsize(-float('inf'))          # instability: halve-ish step
    assert a.get_current_stepsize() == pytest.approx(.3 * np.exp(-1.))
    a.adapt_stepsize(0.)                      # exact: grow
    assert a.get_current_stepsize() > .3 * np.exp(-1.)
    d = DirectionSummarizer()
    d.update(np.array([1., 0.]))
    d.update(np.array([-1., -1.]))
    np.testing.assert_allclose(d.get_mean(), [1., .5])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cox_kernels_do_not_spill(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "cox.hip"), tmp_path)
    for k in ("cox_max_kernel", "cox_risk_sum_kernel", "cox_event_sum_kernel",
              "cox_scan_out_kernel", "cox_row_weight_kernel",
              "cox_loglik_kernel", "cox_reset_kernel",
              "cox_step1_kernel", "cox_post_a_kernel", "cox_post_b_kernel",
              "cox_sumsq_kernel", "cox_traj_init_kernel", "cox_finish_kernel"):
        assert any(k in name for name in table), (k, sorted(table))
    for k in ("cox_risk_sum_kernel", "cox_event_sum_kernel",
              "cox_row_weight_kernel"):
        assert sum(k in name for name in table) == 2, (k, sorted(table))
    for name, res in table.items():
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
