"""The update of the negative-binomial model's dispersion inside the Gibbs
loop: Neal's univariate slice sampler (Neal 2003, "Slice sampling", figures 3
and 5) on theta = log r, and the conditional log-density it is run on.

The sampler is written against a callable, so that the identical code runs on
the device model (one bbx_negbin_dispersion_loglik launch per call of the
callable, whatever the number of points) and on the NumPy oracle of the
tests."""
import math

import numpy as np

WIDTH = 1.              # of the initial interval, on the log scale
MAX_EXPANSIONS = 10     # stepping-out: expansions of both ends together
MAX_SHRINKAGES = 1000   # shrinkage halts by acceptance; this is a safety net
DEFAULT_PRIOR = {'shape': 2., 'rate': .1}    # r ~ Gamma(shape, rate)


def slice_update(theta, logdensity, uniform, width=WIDTH,
                 max_expansions=MAX_EXPANSIONS):
    """One slice-sampling update of a scalar theta with log-density
    `logdensity` (up to a constant): stepping out with an initial interval of
    `width` and at most `max_expansions` expansions in total, then shrinkage
    until a point is accepted.  The update leaves the density invariant.

    logdensity(points) takes a 1-D array of up to 8 points and returns their
    log-densities: the points of one call cost one pass over the data.
    uniform() returns one number in [0, 1).

    The uniforms are consumed in this order, which is part of the contract (a
    seeded chain depends on it):
      1. the slice level: log y = f(theta) + log u
      2. the position of the initial interval: L = theta - width u, R = L + width
      3. the split of the expansion limit: J = floor(max_expansions u) to the
         left, max_expansions - 1 - J to the right
      4. one per shrinkage proposal: x = L + u (R - L)
    No uniform is drawn while stepping out.  The first call of logdensity is
    at (theta, L, R); every stepping-out round evaluates the ends that still
    expand in one call (the two ends step out independently of each other, so
    this is Neal's procedure, not a variant of it); every shrinkage proposal
    is one call.  Returns the new theta."""
    theta = float(theta)
    u_level, u_pos, u_split = uniform(), uniform(), uniform()
    left = theta - width * u_pos
    right = left + width
    n_left = int(math.floor(max_expansions * u_split))
    n_right = (max_expansions - 1) - n_left
    f0, f_left, f_right = (float(v) for v in logdensity(
        np.array([theta, left, right])))
    if not math.isfinite(f0):
        raise ValueError("The log-density at the current state is not "
                         "finite: %r at %r." % (f0, theta))
    level = f0 + (math.log(u_level) if u_level > 0. else -math.inf)
    # stepping out: an end expands while it is inside the slice
    go_left = n_left > 0 and level < f_left
    go_right = n_right > 0 and level < f_right
    while go_left or go_right:
        points = []
        if go_left:
            left -= width
            n_left -= 1
            points.append(left)
        if go_right:
            right += width
            n_right -= 1
            points.append(right)
        values = [float(v) for v in logdensity(np.array(points))]
        if go_left:
            go_left = n_left > 0 and level < values[0]
        if go_right:
            go_right = n_right > 0 and level < values[-1]
    # shrinkage
    for _ in range(MAX_SHRINKAGES):
        x = left + uniform() * (right - left)
        if level < float(logdensity(np.array([x]))[0]):
            return x
        if x < theta:
            left = x
        else:
            right = x
    raise RuntimeError("The slice sampler's interval shrank %d times without "
                       "an accepted point." % MAX_SHRINKAGES)


def check_gamma_prior(prior, option, default):
    """A Gamma prior given as the option `option`: None (a copy of `default`)
    or a dict with 'shape' and 'rate', both finite and positive."""
    if prior is None:
        return dict(default)
    try:
        shape, rate = float(prior['shape']), float(prior['rate'])
        extra = set(prior) - {'shape', 'rate'}
    except (TypeError, KeyError, ValueError):
        raise ValueError("%s must be a dict with 'shape' and 'rate'."
                         % option) from None
    if extra or not (math.isfinite(shape) and math.isfinite(rate)
                     and shape > 0. and rate > 0.):
        raise ValueError("%s takes a finite, positive 'shape' and 'rate' and "
                         "nothing else." % option)
    return {'shape': shape, 'rate': rate}


def log_scale_conditional(model, loglik, coef, prior, jacobian=True):
    """f(theta) = L(x) + shape theta - rate x, x = exp(theta): the log of the
    conditional density of a positive parameter x on the log scale, the
    Jacobian included (Gamma(shape, rate) on x has density x^(shape - 1)
    exp(-rate x), and dx = x dtheta).  L comes from the model's method named
    `loglik`: the first call forms the linear predictor at `coef`, the later
    ones reuse it.  jacobian=False drops the Jacobian's theta: the wrong
    target, for the tests' negative control."""
    shape = prior['shape'] - (0. if jacobian else 1.)
    rate = prior['rate']
    state = {'coef': coef}

    def f(thetas):
        thetas = np.asarray(thetas, dtype=np.float64)
        with np.errstate(over='ignore', under='ignore'):
            x = np.exp(thetas)
        # an x that left the doubles' range has no density to speak of
        ok = np.isfinite(x) & (x > 0.)
        out = np.full(thetas.shape, -np.inf)
        if ok.any():
            L = np.asarray(getattr(model, loglik)(state['coef'], x[ok]))
            state['coef'] = None
            out[ok] = L + shape * thetas[ok] - rate * x[ok]
        return out

    return f


def check_prior(prior):
    """dispersion_prior: None (the default Gamma(2, 0.1)) or a dict with
    'shape' and 'rate', both finite and positive."""
    return check_gamma_prior(prior, 'dispersion_prior', DEFAULT_PRIOR)


def log_conditional(model, coef, prior, jacobian=True):
    """log_scale_conditional of r = exp(theta) with L from
    model.dispersion_loglik."""
    return log_scale_conditional(model, 'dispersion_loglik', coef, prior,
                                 jacobian)


def update_dispersion(model, coef, r, prior, uniform):
    """The Gibbs step: r | coef by one slice update on log r."""
    theta = slice_update(math.log(r), log_conditional(model, coef, prior),
                         uniform)
    return math.exp(theta)
