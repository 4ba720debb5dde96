"""The update of the Weibull model's shape inside the Gibbs loop: the slice
sampler of dispersion.py on theta = log k, and the conditional log-density it
is run on.  The sampler itself is dispersion.slice_update, which states the
order in which the uniforms are consumed; it is written against a callable,
so the identical code runs on the device model (one bbx_weibull_shape_loglik
launch per call of the callable, whatever the number of points) and on the
NumPy oracle of the tests."""
import math

import numpy as np

from .dispersion import slice_update

DEFAULT_PRIOR = {'shape': 2., 'rate': 1.}    # k ~ Gamma(shape, rate)


def check_prior(prior):
    """weibull_shape_prior: None (the default Gamma(2, 1): mean 2, mode 1 --
    the exponential model -- and no mass at k = 0) or a dict with 'shape' and
    'rate', both finite and positive."""
    if prior is None:
        return dict(DEFAULT_PRIOR)
    try:
        shape, rate = float(prior['shape']), float(prior['rate'])
        extra = set(prior) - {'shape', 'rate'}
    except (TypeError, KeyError, ValueError):
        raise ValueError("weibull_shape_prior must be a dict with 'shape' "
                         "and 'rate'.") from None
    if extra or not (math.isfinite(shape) and math.isfinite(rate)
                     and shape > 0. and rate > 0.):
        raise ValueError("weibull_shape_prior takes a finite, positive "
                         "'shape' and 'rate' and nothing else.")
    return {'shape': shape, 'rate': rate}


def log_conditional(model, coef, prior, jacobian=True):
    """f(theta) = L(k) + shape theta - rate k, k = exp(theta): the log of the
    shape's conditional density on the log scale, the Jacobian included
    (Gamma(shape, rate) on k has density k^(shape - 1) exp(-rate k), and
    dk = k dtheta).  L is the whole log density summed over the rows, from
    model.shape_loglik: the first call forms the linear predictor at `coef`,
    the later ones reuse it.  jacobian=False drops the Jacobian's theta: the
    wrong target, for the tests' negative control."""
    shape = prior['shape'] - (0. if jacobian else 1.)
    rate = prior['rate']
    state = {'coef': coef}

    def f(thetas):
        thetas = np.asarray(thetas, dtype=np.float64)
        with np.errstate(over='ignore', under='ignore'):
            k = np.exp(thetas)
        # a k that left the doubles' range has no density to speak of
        ok = np.isfinite(k) & (k > 0.)
        out = np.full(thetas.shape, -np.inf)
        if ok.any():
            loglik = np.asarray(model.shape_loglik(state['coef'], k[ok]))
            state['coef'] = None
            out[ok] = loglik + shape * thetas[ok] - rate * k[ok]
        return out

    return f


def update_shape(model, coef, k, prior, uniform):
    """The Gibbs step: k | coef by one slice update on log k."""
    theta = slice_update(math.log(k), log_conditional(model, coef, prior),
                         uniform)
    return math.exp(theta)
