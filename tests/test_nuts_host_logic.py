"""CPU: the host side of the 'nuts' coefficient sampler -- the unrolled
schedule the device runs (leaf, the merges due at step t, termination)
against a recursive restatement of nuts.py on a toy Gaussian target, the
draw-ahead / advance bookkeeping of the uniforms on the NumPy stream, the
sampler options and info keys, the exported symbols and the register budget of
the new kernels in csrc/cox.hip."""
import math
import os
import re

import numpy as np
import pytest

import nuts_oracle as no
from conftest import ROOT
from test_cholesky_kernel_resources import HIPCC, _resource_table


def _gaussian(P, seed):
    prec = np.exp(np.random.RandomState(seed).randn(P))

    def f(q):
        return -0.5 * np.sum(prec * q ** 2), -prec * q
    return f


class _Feed:
    """A fixed sequence of uniforms; counts what is consumed."""

    def __init__(self, seed):
        self.u = np.random.RandomState(seed).rand(4096)
        self.k = 0

    def __call__(self):
        self.k += 1
        return self.u[self.k - 1]


def _half_trees(h, d, dt, seed, tol):
    """The same half-tree by the recursion and by the unrolled schedule."""
    P = 7
    f = _gaussian(P, seed)
    rs = np.random.RandomState(100 + seed)
    q, p = rs.randn(P), rs.randn(P)
    logp, grad = f(q)
    joint = -no.hamiltonian(logp, p)
    thr = joint - rs.exponential()
    out = []
    for build in ('recursive', 'unrolled'):
        feed = _Feed(seed)
        sh = no.Shared(f, dt, joint, thr, tol, feed)
        if build == 'recursive':
            root = no.Tree(sh, q, p, logp, grad, joint)
            t = root.build(q, p, grad, h, d)
            res = (no.tree_scalars(t), t.sample, t.end(d), t.terminated)
        else:
            res = no.unrolled_half_tree(sh, q, p, grad, h, d)
        out.append((res, sh.n_step, sh.n_uniform, feed.k))
    return out


@pytest.mark.parametrize('h', range(7))
def test_unrolled_schedule_equals_the_recursion_bit_for_bit(h):
    """Step sizes from well inside the stability limit (trees run to 2^h
    leaves or meet a U-turn on the way) to past it (instability stops); a
    small tolerance makes the min / max rule fire inside half-trees too."""
    seen = set()
    for seed in range(12):
        for d in (1, -1):
            for dt, tol in ((.05, 100.), (.4, 100.), (.9, 100.), (1.3, .5),
                            (2.5, 100.)):
                rec, unr = _half_trees(h, d, dt, seed, tol)
                (sr, sampr, endr, termr), nr, ur, kr = rec
                (su, sampu, endu, stopu), nu, uu, ku = unr
                assert sr == su, (seed, d, dt, sr, su)      # exact floats
                assert (nr, ur, kr) == (nu, uu, ku)
                assert bool(termr) == bool(stopu)
                assert nr <= 2 ** h and (termr or nr == 2 ** h)
                if not termr:
                    assert ur == 2 ** h - 1
                    for a, b in zip(sampr, sampu):
                        np.testing.assert_array_equal(a, b)
                    for a, b in zip(endr, endu):
                        np.testing.assert_array_equal(a, b)
                seen.add((bool(termr), bool(sr['u_turn']), nr < 2 ** h))
    if h >= 3:
        # complete trees, U-turn stops and instability stops, some early
        assert (False, False, False) in seen
        assert any(s[0] and s[1] for s in seen)
        assert any(s[0] and not s[1] for s in seen)
        assert any(s[2] for s in seen)


def test_buffer_assignment_never_overlaps():
    """The tree whose first leaf is step i + 1 lives in buffer tz(i) (h for
    i = 0) from step i + 1 until it is absorbed at step i + 2^tz(i): no two
    live trees share a buffer, and at most h + 1 buffers are used."""
    for h in range(1, 8):
        live = {}
        for t in range(1, 2 ** h + 1):
            if t & 1:
                b = no.buffer_of(t - 1, h)
                assert 0 <= b <= h and b not in live
                live[b] = t - 1
                continue
            lev = 0
            while lev < h and t % (2 << lev) == 0:
                absorbed = 'leaf' if lev == 0 else lev
                if lev:
                    assert live.pop(absorbed) == t - (1 << lev)
                assert live[no.buffer_of(t - (2 << lev), h)] == t - (2 << lev)
                lev += 1
        assert live == {h: 0}


def test_draw_ahead_leaves_the_stream_where_the_recursion_leaves_it():
    """A draw through draw_ahead / advance per doubling (what nuts.py does
    around the device call) against the same draw taking its uniforms one by
    one from np.random: same result, same generator state afterwards."""
    from bayesbridge_amd import nuts
    P = 5
    f = _gaussian(P, 3)
    early = 0
    for seed in range(20):
        rs = np.random.RandomState(seed)
        q, dt = rs.randn(P), (.3, .8, 1.2)[seed % 3]
        logp, grad = f(q)
        np.random.seed(seed)
        q1, i1 = no.generate_next_state(f, dt, q, logp, grad, max_height=6)
        after1 = np.random.get_state()
        tail1 = np.random.rand(3)
        # the same draw, the uniforms of every doubling drawn ahead
        np.random.seed(seed)
        p = np.random.randn(P)
        joint = -no.hamiltonian(logp, p)
        thr = joint - np.random.exponential()
        directions = 2 * (np.random.rand(6) < 0.5) - 1
        np.testing.assert_array_equal(directions, i1['directions'])
        pool = []
        sh = no.Shared(f, dt, joint, thr, 100., lambda: pool.pop(0))
        tree = no.Tree(sh, q, p, logp, grad, joint)
        for height, rec in enumerate(i1['doublings']):
            ahead, state = nuts.draw_ahead(2 ** height)
            pool[:] = list(ahead)
            used = sh.n_uniform
            tree.double(height, directions[height])
            used = sh.n_uniform - used
            assert used == rec['n_uniform'] <= 2 ** height
            early += used < 2 ** height
            nuts.advance(state, used)
        np.testing.assert_array_equal(tree.sample[0], q1)
        assert no.tree_scalars(tree) == {
            k: i1['doublings'][-1][k] for k in no.tree_scalars(tree)}
        after2 = np.random.get_state()
        assert after1[2] == after2[2] and np.array_equal(after1[1], after2[1])
        np.testing.assert_array_equal(np.random.rand(3), tail1)
    assert early >= 5       # half-trees that consumed fewer than 2^h


class _Design:
    shape = (50, 5)
    use_hip = True
    is_sparse = True


def test_nuts_options_and_info_keys():
    from bayesbridge_amd import SamplerOptions
    from bayesbridge_amd.bayesbridge import HMC_INFO_KEYS, NUTS_INFO_KEYS
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')              # accepted without warning
        opt = SamplerOptions.pick_default_and_create('nuts', None, 'cox',
                                                     _Design())
        via_dict = SamplerOptions.pick_default_and_create(
            None, {'coef_sampler_type': 'nuts'}, 'cox', _Design())
    assert opt.coef_sampler_type == 'nuts' and opt.rng == 'reference'
    assert via_dict.get_info() == opt.get_info()
    again = SamplerOptions.pick_default_and_create(None, opt.get_info(),
                                                   'cox', _Design())
    assert again.get_info() == opt.get_info()
    for family in ('linear', 'logit'):
        with pytest.raises(ValueError):
            SamplerOptions.pick_default_and_create('nuts', None, family,
                                                   _Design())
    with pytest.raises(ValueError):
        SamplerOptions.pick_default_and_create('nuts', {'rng': 'device'},
                                               'cox', _Design())
    with pytest.raises(ValueError):
        SamplerOptions(coef_sampler_type='nuts', rng='device')
    # the default for the Cox model stays 'hmc'
    assert SamplerOptions.pick_default_and_create(
        None, None, 'cox', _Design()).coef_sampler_type == 'hmc'
    shared = ('stepsize', 'n_hessian_matvec', 'n_grad_evals',
              'stability_limit_est', 'stability_adjustment_factor',
              'instability_detected')              # gibbs_util.py:150-159
    assert set(NUTS_INFO_KEYS) == set(shared) | {'tree_height',
                                                 'ave_accept_prob'}
    assert set(HMC_INFO_KEYS) == set(shared) | {'n_integrator_step',
                                                'accepted', 'accept_prob'}


def test_nuts_entry_points_are_declared_and_versions_agree():
    from bayesbridge_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'bbx.h')).read()
    declared = set(re.findall(r'\b(bbx_cox_nuts_\w+)\s*\(', header))
    assert declared == {'bbx_cox_nuts_begin', 'bbx_cox_nuts_doubling',
                        'bbx_cox_nuts_sample'}
    lib = _lib.load()
    assert declared <= set(_lib.EXPORTED_SYMBOLS)
    for name in declared:
        assert getattr(lib, name).restype is not None
    version = int(re.search(r'#define BBX_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == lib.bbx_version() >= 107


NUTS_KERNELS = ("cox_nuts_init_kernel", "cox_nuts_start_kernel",
                "cox_nuts_leaf_kernel", "cox_nuts_store_kernel",
                "cox_nuts_merge_a_kernel", "cox_nuts_merge_b_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_nuts_kernels_use_no_scratch(tmp_path):
    table = _resource_table(
        os.path.join(ROOT, "bayes-bridge_amd", "csrc", "cox.hip"), tmp_path)
    for k in NUTS_KERNELS:
        assert any(k in name for name in table), (k, sorted(table))
    # the inner and the top-level form of both merge kernels
    assert sum("cox_nuts_merge_a_kernel" in k for k in table) == 2
    assert sum("cox_nuts_merge_b_kernel" in k for k in table) == 2
    for name, res in table.items():
        if "cox_nuts_" not in name:
            continue
        assert res["VGPRs"] <= 256, (name, res)
        assert res["VGPRs Spill"] == 0, (name, res)
        assert res["SGPRs Spill"] == 0, (name, res)
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)


def test_schedule_enqueues_the_trailing_zeros_of_t():
    """At most h merges at one step, 2^h - 1 in a half-tree."""
    for h in range(10):
        total = 0
        for t in range(1, 2 ** h + 1):
            due = 0
            while due < h and t % (2 << due) == 0:
                due += 1
            assert due == min(h, (t & -t).bit_length() - 1)
            total += due
        assert total == 2 ** h - 1
    assert int(math.log2(512)) == 9


def test_restatement_reproduces_the_reference_fixtures(golden_dir):
    """tests/nuts_oracle.py on tests/cox_oracle.py against the reference's
    recorded draws: the same decisions, uniforms and stream position."""
    import cox_oracle as co
    from bayesbridge_amd.model import cox_preprocess, cox_risk_sets
    import warnings
    g = np.load(os.path.join(golden_dir, 'nuts_calls.npz'))
    fs = {}
    for problem in ('chain_dense', 'chain_sparse', 'small'):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            et, ct, X, _ = cox_preprocess(g[problem + '_event_time'],
                                          g[problem + '_censoring_time'],
                                          g[problem + '_X'])
        fs[problem] = co.precond_f(X, g[problem + '_scale'],
                                   g[problem + '_prior_prec'],
                                   cox_risk_sets(et, ct))
    assert int(g['n_call']) >= 60 and float(g['min_margin']) > 1e-9
    for k in range(int(g['n_call'])):
        pre = 'call%03d_' % k
        f = fs[str(g[pre + 'problem'])]
        np.random.seed(int(g[pre + 'seed']))
        with np.errstate(all='ignore'):
            q, info = no.generate_next_state(
                f, float(g[pre + 'dt']), g[pre + 'q'], *f(g[pre + 'q']),
                p=g[pre + 'p'], max_height=int(g[pre + 'max_height']),
                tol=float(g[pre + 'tol']))
        assert np.random.rand() == float(g[pre + 'next_number'])
        np.testing.assert_array_equal(info['uniforms'], g[pre + 'uniforms'])
        assert info['tree_height'] == int(g[pre + 'tree_height'])
        assert info['n_grad_evals'] + 1 == int(g[pre + 'n_grad_evals'])
        for key in ('u_turn_detected', 'instability_detected',
                    'last_doubling_rejected'):
            assert info[key] == bool(g[pre + key])
        np.testing.assert_allclose(q, g[pre + 'q_out'], rtol=1e-8, atol=1e-11)
        for key in ('ave_accept_prob', 'ave_hamiltonian_error'):
            assert info[key] == pytest.approx(float(g[pre + key]), rel=1e-9)
