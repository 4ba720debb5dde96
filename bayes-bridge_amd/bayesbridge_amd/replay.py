"""Sequential host replay of the device chain's Philox draws
(`bbx_replay_*` of libbbx_hostrng.so, csrc/replay_impl.hpp): what the tests
pin the sampler kernels to, draw by draw.  NumPy marshalling only.

`stream` is the kernel's stream word: `iter_stream(STREAM_PG, it)` for the
chain's iteration `it`, the bare stream id for the stand-alone
`bbx_device_*` entry points.  `variant` 0 is the reference's arithmetic, 1 the
kernels' forms evaluated by the host's libm."""
import ctypes
from ctypes import c_double, c_int, c_int64, c_uint32, c_uint64, c_void_p

import numpy as np

from . import hostrng

# csrc/philox.hpp PhiloxStream
STREAM_ETA1, STREAM_ETA2, STREAM_PG, STREAM_GSCALE, STREAM_LSCALE, \
    STREAM_OBSVAR = 1, 2, 3, 4, 5, 6
STREAM_LATENT = 7
STREAM_MIX = 8
STREAM_QMIX = 9

_SIGS = {
    "bbx_replay_philox_block": [c_void_p, c_void_p, c_void_p],
    "bbx_replay_philox_counter": [c_uint64, c_uint64, c_uint64, c_uint32,
                                  c_void_p, c_void_p],
    "bbx_replay_uniform": [c_uint64, c_uint64, c_uint64, c_uint32, c_int64,
                           c_void_p],
    "bbx_replay_normal": [c_uint64, c_uint64, c_int64, c_void_p],
    "bbx_replay_polya_gamma": [c_uint64, c_uint64, c_int64, c_int, c_void_p,
                               c_void_p, c_int, c_void_p, c_void_p, c_void_p],
    "bbx_replay_tilted_stable": [c_uint64, c_uint64, c_int64, c_double,
                                 c_void_p, c_int, c_void_p, c_void_p],
    "bbx_replay_truncated_normal": [c_uint64, c_uint64, c_int64, c_void_p,
                                    c_void_p, c_int, c_void_p, c_void_p],
    "bbx_replay_inverse_gaussian": [c_uint64, c_uint64, c_int64, c_void_p,
                                    c_double, c_int, c_void_p, c_void_p,
                                    c_void_p],
    "bbx_host_log_norm_cdf": [c_int64, c_void_p, c_void_p],
    "bbx_replay_gamma": [c_uint64, c_uint64, c_uint64, c_int64, c_double,
                         c_void_p],
}
_declared = False


def _lib():
    global _declared
    lib = hostrng.load()
    if not _declared:
        for name, argtypes in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = c_int
        _declared = True
    return lib


def _check(status, what):
    if status != 0:
        raise ValueError("invalid arguments to the %s replay" % what)


def _p(a):
    return a.ctypes.data_as(c_void_p)


def iter_stream(stream, iteration):
    """The stream word of chain iteration `iteration` (csrc/chain.hip)."""
    return (int(stream) | (int(iteration) << 8)) & 0xFFFFFFFFFFFFFFFF


def philox_block(counter, key):
    """One Philox4x32-10 block: counter[4], key[2] -> four 32-bit words."""
    c = np.ascontiguousarray(counter, dtype=np.uint32)
    k = np.ascontiguousarray(key, dtype=np.uint32)
    assert c.shape == (4,) and k.shape == (2,)
    out = np.empty(4, dtype=np.uint32)
    _check(_lib().bbx_replay_philox_block(_p(c), _p(k), _p(out)), 'Philox')
    return out


def philox_counter(seed, stream, index, trial=0):
    """(counter[4], key[2]) of a freshly made Philox(seed, stream, index,
    trial)."""
    c, k = np.empty(4, dtype=np.uint32), np.empty(2, dtype=np.uint32)
    _check(_lib().bbx_replay_philox_counter(seed, stream, index, trial,
                                            _p(c), _p(k)), 'Philox')
    return c, k


def uniform(seed, stream, index, trial, n):
    out = np.empty(n)
    _check(_lib().bbx_replay_uniform(seed, stream, index, trial, n, _p(out)),
           'uniform')
    return out


def normal(seed, stream, n):
    out = np.empty(n)
    _check(_lib().bbx_replay_normal(seed, stream, n, _p(out)), 'normal')
    return out


def polya_gamma(seed, stream, shape, tilt, variant=0, trace=False):
    """Draws; with trace, (draws, attempts, restarts): the inverse-Gaussian
    proposals each element took and whether its series test made it start
    over.  `shape`: an integer array (int32, as bbx_device_polya_gamma takes
    it) or a float one (double, as the chain holds n_trial)."""
    shape = np.asarray(shape)
    is_double = not np.issubdtype(shape.dtype, np.integer)
    shape = np.ascontiguousarray(
        shape, dtype=np.float64 if is_double else np.int32)
    tilt = np.ascontiguousarray(tilt, dtype=np.float64)
    assert shape.shape == tilt.shape and tilt.ndim == 1
    out = np.empty(tilt.size)
    att = np.zeros(tilt.size, dtype=np.int32)
    rst = np.zeros(tilt.size, dtype=np.int32)
    _check(_lib().bbx_replay_polya_gamma(
        seed, stream, tilt.size, int(is_double), _p(shape), _p(tilt),
        int(variant), _p(out), _p(att), _p(rst)), 'Polya-Gamma')
    return (out, att, rst) if trace else out


def tilted_stable(seed, stream, char_exp, tilt, variant=0, trace=False):
    """Draws; with trace, (draws, winner): the number of the accepted
    candidate of each element."""
    tilt = np.ascontiguousarray(tilt, dtype=np.float64)
    assert tilt.ndim == 1
    out = np.empty(tilt.size)
    win = np.zeros(tilt.size, dtype=np.int32)
    _check(_lib().bbx_replay_tilted_stable(
        seed, stream, tilt.size, float(char_exp), _p(tilt), int(variant),
        _p(out), _p(win)), 'tilted-stable')
    return (out, win) if trace else out


def truncated_normal(seed, stream, psi, positive, variant=0, trace=False):
    """N(psi_i, 1) on z > 0 where positive[i], else on z <= 0, as
    the probit row policy draws it (csrc/probit.hip); with trace, (draws,
    trials): the trials each element took (0: psi was not finite, the draw is
    a NaN).  `stream`: `iter_stream(STREAM_LATENT, it)` for the chain's
    iteration `it` (`it = -1`: the state of a chain that has not run), the
    bare STREAM_LATENT for bbx_device_truncated_normal."""
    psi = np.ascontiguousarray(psi, dtype=np.float64)
    positive = np.ascontiguousarray(np.asarray(positive) != 0, dtype=np.uint8)
    assert psi.ndim == 1 and positive.shape == psi.shape
    out = np.empty(psi.size)
    trials = np.zeros(psi.size, dtype=np.int32)
    _check(_lib().bbx_replay_truncated_normal(
        seed, stream, psi.size, _p(psi), _p(positive), int(variant), _p(out),
        _p(trials)), 'truncated-normal')
    return (out, trials) if trace else out


def censored_normal(seed, stream, psi, bound, status, tau, variant=0,
                    trace=False):
    """The censored model's latents as the censored row policy draws them
    (csrc/censored.hip): bound_i where status_i == 0, else bound_i + u /
    sqrt(tau) with u = truncated_normal at psi' = (psi_i - bound_i) sqrt(tau),
    positive where status_i == 1; with trace, (draws, trials) -- 0 trials on an
    observed row and where psi' is not finite (the draw is then a NaN on a
    censored row).  `variant` is truncated_normal's; the kernel forms psi' and
    u / sqrt(tau) with the same product and the same true division as this
    function, so no further form belongs to variant 1.  `stream` as for
    truncated_normal; the bare STREAM_LATENT for bbx_device_censored_normal."""
    psi = np.ascontiguousarray(psi, dtype=np.float64)
    bound = np.ascontiguousarray(bound, dtype=np.float64)
    status = np.asarray(status)
    assert psi.ndim == 1 and bound.shape == psi.shape \
        and status.shape == psi.shape
    rt = np.sqrt(np.float64(tau))
    with np.errstate(invalid='ignore', over='ignore'):
        scaled = (psi - bound) * rt
    u, trials = truncated_normal(seed, stream, scaled, status == 1, variant,
                                 trace=True)
    censored = status != 0
    with np.errstate(invalid='ignore'):
        out = np.where(censored, bound + u / rt, bound)
    trials = np.where(censored, trials, 0).astype(np.int32)
    return (out, trials) if trace else out


def inverse_gaussian(seed, stream, m, lam, variant=0, trace=False,
                     margin=False):
    """InverseGaussian(mean 1 / m_i, shape lam) as the quantile row policy
    draws it (csrc/quantile.hip, InverseGaussian of csrc/samplers.hpp): one
    normal and one uniform of Philox(seed, stream, i); m_i = 0 is Levy's law.
    With trace, (draws, branch): 0 where the smaller root was taken, 1 for the
    other; with margin as well, (draws, branch, u (1 + m x)): the number the
    draw compares with 1.  The draw has no device form of its own, so
    `variant` 1 is variant 0.  `stream`: `iter_stream(STREAM_QMIX, it)` for
    the chain's iteration `it` (`it = -1`: a chain that has not run), the
    bare STREAM_LATENT for bbx_device_inverse_gaussian."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    assert m.ndim == 1
    out = np.empty(m.size)
    branch = np.zeros(m.size, dtype=np.int32)
    mar = np.zeros(m.size)
    _check(_lib().bbx_replay_inverse_gaussian(
        seed, stream, m.size, _p(m), float(lam), int(variant), _p(out),
        _p(branch), _p(mar)), 'inverse-Gaussian')
    if trace and margin:
        return out, branch, mar
    return (out, branch) if trace else out


def log_norm_cdf(x):
    """log Phi(x) in the host form of csrc/samplers.hpp."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(x.shape)
    _check(_lib().bbx_host_log_norm_cdf(x.size, _p(x), _p(out)),
           'log_norm_cdf')
    return out


def gamma(seed, stream, shape, n=1, index=0):
    """gamma_draw on Philox(seed, stream, index + k), k < n."""
    out = np.empty(n)
    _check(_lib().bbx_replay_gamma(seed, stream, index, n, float(shape),
                                   _p(out)), 'Gamma')
    return out
