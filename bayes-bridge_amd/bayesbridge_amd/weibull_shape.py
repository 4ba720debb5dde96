"""The update of the Weibull model's shape inside the Gibbs loop: the slice
sampler of dispersion.py on theta = log k, and the conditional log-density it
is run on.  The sampler itself is dispersion.slice_update, which states the
order in which the uniforms are consumed; it is written against a callable,
so the identical code runs on the device model (one bbx_weibull_shape_loglik
launch per call of the callable, whatever the number of points) and on the
NumPy oracle of the tests."""
import math

from .dispersion import (check_gamma_prior, log_scale_conditional,
                         slice_update)

DEFAULT_PRIOR = {'shape': 2., 'rate': 1.}    # k ~ Gamma(shape, rate)


def check_prior(prior):
    """weibull_shape_prior: None (the default Gamma(2, 1): mean 2, mode 1 --
    the exponential model -- and no mass at k = 0) or a dict with 'shape' and
    'rate', both finite and positive."""
    return check_gamma_prior(prior, 'weibull_shape_prior', DEFAULT_PRIOR)


def log_conditional(model, coef, prior, jacobian=True):
    """dispersion.log_scale_conditional of k = exp(theta) with L, the whole
    log density summed over the rows, from model.shape_loglik."""
    return log_scale_conditional(model, 'shape_loglik', coef, prior, jacobian)


def update_shape(model, coef, k, prior, uniform):
    """The Gibbs step: k | coef by one slice update on log k."""
    theta = slice_update(math.log(k), log_conditional(model, coef, prior),
                         uniform)
    return math.exp(theta)
