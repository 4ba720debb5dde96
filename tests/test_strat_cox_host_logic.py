"""CPU: the host side of the stratified Cox model -- the vectorised
preprocessing and risk sets against loop implementations, the sum-over-strata
oracle (tests/strat_cox_oracle.py) against the brute-force definition, the
argument errors, the ABI version and the register budget of the kernels in
csrc/cox_strat.hpp (no spills, no scratch)."""
import os
import re
import warnings

import numpy as np
import pytest

import cox_oracle as co
import strat_cox_oracle as so
from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table


def _raw_case(seed, labels='int', n=240):
    """Shuffled rows with ties within and across strata, one stratum with no
    event and a row censored before its stratum's first event."""
    rs = np.random.RandomState(seed)
    event = np.round(rs.exponential(1., n), 1) + .1
    cens = np.full(n, np.inf)
    c = rs.rand(n) < .5
    cens[c] = np.round(rs.exponential(1., c.sum()), 1)
    event[c] = np.inf
    lab = rs.randint(0, 9, n)
    dead = lab == 4                     # stratum 4: censored rows only
    event[dead] = np.inf
    cens[dead] = np.round(rs.exponential(1., dead.sum()), 1)
    cens[np.flatnonzero(c & ~dead)[0]] = 0.     # before every event
    if labels == 'str':
        lab = np.array(['site-%s' % 'fhbadceig'[k] for k in lab])
    return event, cens, lab, rs.randn(n, 4)


@pytest.mark.parametrize('labels', ['int', 'str'])
@pytest.mark.parametrize('seed', range(3))
def test_preprocessing_equals_the_loops(seed, labels):
    from bayesbridge_amd.model import (cox_preprocess_stratified,
                                       cox_stratified_risk_sets)
    event, cens, lab, X = _raw_case(seed, labels)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        et, ct, st, Xs, keep = cox_preprocess_stratified(event, cens, lab, X)
    # sorted, strata without an event removed, uninformative rows removed
    assert len(w) == 3 and len({str(x.message) for x in w}) == 3
    want = so.preprocess_by_loops(event, cens, lab)
    np.testing.assert_array_equal(keep, want)
    assert len(keep) < len(event)
    np.testing.assert_array_equal(et, event[keep])
    np.testing.assert_array_equal(ct, cens[keep])
    np.testing.assert_array_equal(st, lab[keep])
    np.testing.assert_array_equal(Xs, X[keep])
    eventless = [x for x in np.unique(lab)
                 if not np.any(np.isfinite(event[lab == x]))]
    assert len(eventless) == 1 and not np.any(st == eventless[0])
    # a second pass has nothing to do and says nothing
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        again = cox_preprocess_stratified(et, ct, st)
    assert len(w) == 0
    np.testing.assert_array_equal(again[4], np.arange(len(et)))
    # risk sets: the unstratified loops of the oracle, stratum by stratum
    pieces = so.split(et, ct, st)
    got = cox_stratified_risk_sets(et, ct, st)
    loops = []
    for sl, *_ in pieces:
        ne, s, e, n_app = co.risk_sets_by_loops(et[sl], ct[sl])
        loops.append((sl, ne, s, e, n_app))
    for a, b in zip(got, so.global_risk_sets(loops)):
        np.testing.assert_array_equal(a, b)
    assert len(got[0]) == len(np.unique(st)) + 1
    # ties inside a stratum and the same time in two strata
    ev = np.isfinite(et)
    assert np.any((et[1:] == et[:-1]) & (st[1:] == st[:-1]) & ev[1:])
    code = np.unique(st, return_inverse=True)[1]
    pairs = np.unique(np.stack((et[ev], code[ev])), axis=1)
    assert len(np.unique(et[ev])) < pairs.shape[1]


def test_one_stratum_is_the_unstratified_preprocessing():
    from bayesbridge_amd.model import (cox_preprocess,
                                       cox_preprocess_stratified,
                                       cox_risk_sets,
                                       cox_stratified_risk_sets)
    rs = np.random.RandomState(7)
    n = 200
    event = rs.exponential(1., n)             # no ties: the order is unique
    cens = np.full(n, np.inf)
    c = rs.rand(n) < .4
    cens[c] = rs.exponential(1., c.sum())
    event[c] = np.inf
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        et, ct, _, keep = cox_preprocess(event, cens)
        et2, ct2, _, _, keep2 = cox_preprocess_stratified(
            event, cens, np.full(n, 'all'))
    np.testing.assert_array_equal(keep, keep2)
    ne, start, end, n_app = cox_risk_sets(et, ct)
    sptr, sne, s2, e2, last = cox_stratified_risk_sets(et2, ct2,
                                                       np.zeros(len(et2)))
    np.testing.assert_array_equal(sptr, [0, len(et)])
    np.testing.assert_array_equal(sne, [ne])
    np.testing.assert_array_equal(s2, start)
    np.testing.assert_array_equal(e2, end)
    np.testing.assert_array_equal(last, n_app - 1)


@pytest.mark.parametrize('seed', range(3))
def test_oracle_equals_the_brute_force_definition(seed):
    sizes = [1, 2, 3, 7, 12, 1, 5, 20, 2]
    et, ct, lab, X, order = so.make_strata(
        sizes, 3, seed=seed, only_events=[0, 4], all_tied=[3])
    from bayesbridge_amd.model import cox_stratified_risk_sets
    pieces = so.split(et, ct, lab)
    sptr, sne, start, end, last = cox_stratified_risk_sets(et, ct, lab)
    for a, b in zip((sptr, sne, start, end, last),
                    so.global_risk_sets(pieces)):
        np.testing.assert_array_equal(a, b)
    rs = np.random.RandomState(seed)
    for scale in (0., .5, 3.):
        beta, v = rs.randn(3) * scale, rs.randn(3)
        ll, grad = so.loglik_grad(X, beta, pieces)
        hv = so.hessian_matvec(X, beta, v, pieces)
        bl, bg, bh = so.brute(X, beta, v, sptr, sne, start, end)
        assert ll == pytest.approx(bl, rel=1e-12)
        np.testing.assert_allclose(grad, bg, rtol=1e-9,
                                   atol=1e-11 * np.abs(bg).max())
        np.testing.assert_allclose(hv, bh, rtol=1e-9,
                                   atol=1e-11 * np.abs(bh).max())
        el, eg, lb, gb = so.loglik_grad_ext(X, beta, pieces)
        assert abs(ll - el) <= co.EDGE_TOL * lb
        assert np.all(np.abs(grad - eg) <= co.EDGE_TOL * gb)
        eh, hb = so.hessian_matvec_ext(X, beta, v, pieces)
        assert np.all(np.abs(hv - eh) <= co.EDGE_TOL * hb)


def test_shift_per_stratum_and_the_global_max_mutant():
    """Two strata 800 apart in eta: the sum over strata is finite; with one
    global max every hazard of the lower stratum underflows."""
    et, ct, lab, X, _ = so.make_strata([30, 40], 2, seed=1, shuffle=False)
    X = np.column_stack((X, (lab == 1) * 1.))
    beta = np.array([.3, -.2, 800.])
    pieces = so.split(et, ct, lab)
    ll, grad = so.loglik_grad(X, beta, pieces)
    assert np.isfinite(ll) and np.all(np.isfinite(grad))
    # the intercept-like column moves nothing: the same as without it
    ll0, grad0 = so.loglik_grad(X, beta * [1, 1, 0], pieces)
    assert ll == pytest.approx(ll0, rel=1e-12)
    assert so.loglik_grad_global_max(X, beta, pieces)[0] == -np.inf
    assert so.loglik_grad_global_max(X, beta * [1, 1, 0], pieces)[0] \
        == pytest.approx(ll0, rel=1e-12)


def test_argument_errors():
    from bayesbridge_amd.model import (cox_preprocess_stratified,
                                       cox_stratified_risk_sets)
    inf = np.inf
    et = np.array([1., 2., inf, 1., inf])
    ct = np.array([inf, inf, 3., inf, 2.])
    lab = np.array([0, 0, 0, 1, 1])
    cox_stratified_risk_sets(et, ct, lab)
    with pytest.raises(ValueError, match='one label'):
        cox_stratified_risk_sets(et, ct, lab[:4])
    with pytest.raises(ValueError, match='one label'):
        cox_preprocess_stratified(et, ct, lab.reshape(5, 1))
    with pytest.raises(ValueError, match='sorted by stratum'):
        cox_stratified_risk_sets(et, ct, lab[::-1])
    with pytest.raises(ValueError, match='event times'):
        cox_stratified_risk_sets(np.array([2., 1., inf, 1., inf]), ct, lab)
    with pytest.raises(ValueError, match='censoring times'):
        cox_stratified_risk_sets(np.array([1., inf, inf, 1., inf]),
                                 np.array([inf, 2., 3., inf, 2.]), lab)
    with pytest.raises(ValueError, match='no event'):
        cox_stratified_risk_sets(np.array([1., 2., inf, inf, inf]),
                                 np.array([inf, inf, 3., 4., 2.]), lab)
    with pytest.raises(ValueError, match='never appear'):
        cox_stratified_risk_sets(et, np.array([inf, inf, .5, inf, 2.]), lab)
    with pytest.raises(ValueError, match='infinity'):
        cox_preprocess_stratified(np.array([1., inf]), np.array([inf, inf]),
                                  [0, 0])
    with pytest.raises(ValueError, match='same length'):
        cox_preprocess_stratified(et, ct[:4], lab)


def test_header_binding_and_library_are_at_110():
    from bayesbridge_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    assert re.search(r'\bbbx_cox_create_stratified\s*\(', header)
    lib = _lib.load()
    assert 'bbx_cox_create_stratified' in _lib.EXPORTED_SYMBOLS
    sigs = _lib._declare(lib)
    assert len(sigs['bbx_cox_create_stratified'][0]) == 8
    assert lib.bbx_cox_create_stratified.restype is not None
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 110


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_stratified_kernels_do_not_spill(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "cox.hip"), tmp_path)
    # five modes of pass A, three outputs of pass B, gradient / Hessian weights
    assert sum("coxs_agg_kernel" in k for k in table) == 5
    assert sum("coxs_out_kernel" in k for k in table) == 3
    assert sum("coxs_weight_kernel" in k for k in table) == 2
    for name, res in table.items():
        if "coxs_" not in name:
            continue
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
