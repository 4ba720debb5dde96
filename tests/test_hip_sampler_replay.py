"""GPU: the device samplers pinned DRAW BY DRAW to a sequential host replay of
their Philox streams (bayesbridge_amd.replay, csrc/replay_impl.hpp).

test_hip_chain.py tests the samplers' distributions (KS at p > 1e-3, 6 sigma
moments): that notices a distortion of a percent.  The kernels' hand-built
structure -- E elements per lane and `__ffs` walks over masks in
csrc/pg_queue.hpp; LDS lists compacted by atomicAdd, up to 16 speculative
candidates per item, lowest-accepted-wins by atomicMin and the `s_tried`
bookkeeping in tilted_stable_block (csrc/chain.hip) -- can slip in ways that
still give positive, finite, plausible draws.  But every draw is a function of
(seed, stream, element, inputs) alone, so identical inputs go to
`bbx_device_*` and to a plain loop over the same sub-streams, and the results
are compared element by element.

Inputs, tolerances and the cap on excluded draws: tests/replay_cases.py (the
tolerance is 1000 x what the replay alone moves by between the reference's
arithmetic and the kernels', measured in tests/test_replay_cpu.py; a draw
whose uniform sits within rounding of a threshold may take another branch on
the device: at most max(2, 1e-5 n) such draws per case, each printed).

Measured on the MI355X (largest difference device against replay; no draw was
excluded in any case; LABNOTES.md "Sampler replay"):
  normals        8.9e-16 absolute                     bound 1e-14
  Polya-Gamma    4.2e-15 relative                     tolerance 1e-12
  tilted stable  1.56e-14 / 3.3e-15 / 1.0e-15 at a = 1/8, 1/4, 1/2
                                                      1.6e-11 / 3.5e-12 / 1e-12
  Gamma          8.0e-15 relative                     tolerance 1e-12
Not covered: the budget-exhaustion branch of the tilted-stable kernel
(`trial >= 4095`) and Polya-Gamma attempts past 125 cannot be reached with
honest inputs; BBX_PG_ELEMS=0 and the in-place `dr_trial` (negative cost
threshold) are diagnostics with other stream orders; E = 4 runs in the chain
only (tests/test_hip_chain_pin.py pins it there).
"""
import ctypes

import numpy as np
import pytest

import replay_cases as C
from bayesbridge_amd import replay as R

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dev_normal(seed, stream, n):
    from bayesbridge_amd import _lib
    out = np.empty(n)
    _lib.check(_lib.load().bbx_device_normal(0, seed, stream, n, _ptr(out)))
    return out


def _dev_pg(seed, shape, tilt):
    from bayesbridge_amd import _lib
    out = np.empty(len(tilt))
    _lib.check(_lib.load().bbx_device_polya_gamma(
        0, seed, len(tilt), _ptr(shape), _ptr(tilt), _ptr(out)))
    return out


def _dev_ts(seed, a, tilt):
    from bayesbridge_amd import _lib
    out = np.empty(len(tilt))
    _lib.check(_lib.load().bbx_device_tilted_stable(
        0, seed, len(tilt), float(a), _ptr(tilt), _ptr(out)))
    return out


@pytest.mark.parametrize("stream", [
    R.STREAM_ETA1, R.STREAM_ETA2,
    R.iter_stream(R.STREAM_ETA1, (1 << 24) + 3)])   # high stream bits: ctr[3]
def test_device_normals_equal_the_replay(stream):
    n = 100003
    dev = _dev_normal(2024, stream, n)
    rep = R.normal(2024, stream, n)
    err = np.abs(dev - rep)
    print("normals, stream %#x: largest absolute difference %.3g, relative "
          "%.3g" % (stream, err.max(), (err / np.abs(rep)).max()))
    assert err.max() <= C.NORMAL_ATOL


@pytest.mark.parametrize("n", C.PG_SIZES)
def test_device_polya_gamma_equals_the_replay(n):
    """n = 255 / 256 / 257: the one-element kernel with a ragged last block;
    49 999 -> 50 000: the switch to eight elements per lane; 51 500: a block of
    the latter whose upper element slots are partly past n.  Tilts ~ N(0, 3^2),
    every 11th N(0, 30^2); planted 0, +-1e-8, +-39.9999, +-40, +-40.0001 (the
    z > 20 switch of right_mass_direct), +-700 and three non-finite ones, in
    the first block and again in the last 250 elements; every 7th shape 2..5
    (the sequential sampler)."""
    shape, tilt, bad = C.pg_inputs(n)
    seed = C.PG_SEEDS[n]
    rep, att, rst = R.polya_gamma(seed, R.STREAM_PG, shape, tilt, 0,
                                  trace=True)
    # the case exercises what it is meant to: a second inverse-Gaussian
    # attempt of one element, and a series test that makes a draw start over
    assert att.max() > 1 and rst.sum() >= 1
    dev = _dev_pg(seed, shape, tilt)
    assert np.array_equal(np.flatnonzero(np.isnan(rep)), bad)
    assert np.array_equal(np.flatnonzero(np.isnan(dev)), bad)
    ok = np.ones(n, dtype=bool)
    ok[bad] = False
    assert np.all(dev[ok] > 0) and np.all(np.isfinite(dev[ok]))
    C.compare("polya-gamma n = %d" % n, dev, rep,
              C.tolerance(C.PG_VARIANT_SPREAD),
              lambda i: "shape %d tilt %.17g attempts %d restart %d"
              % (shape[i], tilt[i], att[i], rst[i]))


def _ts_case(name, a, tilt, seed=9):
    rep, win = R.tilted_stable(seed, R.STREAM_LSCALE, a, tilt, 0, trace=True)
    dev = _dev_ts(seed, a, tilt)
    assert np.all(dev > 0) and np.all(np.isfinite(dev))
    C.compare("tilted stable a = %g %s" % (a, name), dev, rep,
              C.tolerance(C.TS_VARIANT_SPREAD[a]),
              lambda i: "tilt %.17g tilt^a %.17g winner %d"
              % (tilt[i], tilt[i] ** a, win[i]))
    return win


@pytest.mark.parametrize("a", C.TS_EXPONENTS)
def test_device_tilted_stable_equals_the_replay(a):
    """Ragged and full blocks of tilts spread over both regimes, then six
    blocks of a kind each (replay_cases.ts_blocks): all plain rejection, all
    double rejection, one item of the other regime among 255, planted tilts at
    and next to the regime switch, very large tilts."""
    for n in (1, 255, 256, 257):
        _ts_case("mixed %d" % n, a, C.ts_mixed(a, n))
    tilt = C.ts_blocks(a)
    win = _ts_case("blocks", a, tilt)
    # what the replay's winners say the kernel went through: an item that won
    # with a candidate >= 16 (its block ran more than one round at full
    # speculation), and rounds with 1, with 2..15 and with 16 candidates per
    # item inside one block
    assert win.max() >= 16
    rounds = C.ts_rounds(win)
    assert any(sum(1 for c, _ in r if c == 16) >= 2 for r in rounds)
    assert any({1, 16} <= {c for c, _ in r} and
               any(1 < c < 16 for c, _ in r) for r in rounds)
    # the kinds are what they claim to be
    tp = tilt ** a
    assert np.all(tp[:256] < 2) and np.all(tp[256:512] >= 2)
    assert (tp[512:768] >= 2).sum() == 1 and (tp[768:1024] < 2).sum() == 1
    assert tilt[1280:].max() >= 1e20 and tilt[1024 + 5] == 0.


def test_device_tilted_stable_equals_the_replay_past_the_grid_cap():
    """bbx_device_tilted_stable launches at most 4096 blocks of 256 items:
    1 048 576 + 300 items is the first size at which a block comes back for a
    second `base` (blocks 0 and 1, the second one ragged)."""
    a = .25
    tilt = C.ts_mixed(a, C.TS_BIG)
    win = _ts_case("mixed %d" % C.TS_BIG, a, tilt)
    assert win.max() >= 16


@pytest.mark.parametrize("shape", C.GAMMA_SHAPES)
def test_device_gamma_equals_the_replay(shape):
    from bayesbridge_amd import _lib
    n = C.GAMMA_N
    dev = np.empty(n)
    _lib.check(_lib.load().bbx_device_gamma(0, 7, n, shape, _ptr(dev)))
    rep = R.gamma(7, R.STREAM_GSCALE, shape, n=n)
    C.compare("gamma shape %g" % shape, dev, rep, C.GAMMA_TOL)
