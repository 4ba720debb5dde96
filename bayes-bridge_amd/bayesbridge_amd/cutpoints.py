"""The update of the ordinal model's cutpoints inside the Gibbs loop: one
univariate slice update (dispersion.slice_update, unchanged, width 1) per
cutpoint, in increasing order, on the cutpoint itself, and the conditional
log-density it is run on.

The prior is c_k ~ N(0, sd^2) restricted to the ordered cone c_1 < ... <
c_{K-1}, so the conditional of c_k given the others and the coefficients is

    f(c_k) = L(c) - c_k^2 / (2 sd^2)   inside (c_{k-1}, c_{k+1}), -inf outside,

with L the log-likelihood at the whole cutpoint vector.  L comes from
model.cutpoint_loglik: the points of one call of the slice sampler's callable
are whole candidate vectors that differ in entry k and cost one pass over the
rows (bbx_ordinal_cutpoint_loglik on the device model, the NumPy oracle in the
tests).  Points outside the bracket are answered here, without a launch."""
import math

import numpy as np

from .dispersion import slice_update

DEFAULT_PRIOR = {'sd': 10.}    # c_k ~ N(0, sd^2) on the ordered cone


def check_prior(prior):
    """cutpoint_prior: None (the default sd = 10) or a dict with 'sd', finite
    and positive, and nothing else."""
    if prior is None:
        return dict(DEFAULT_PRIOR)
    try:
        sd = float(prior['sd'])
        extra = set(prior) - {'sd'}
    except (TypeError, KeyError, ValueError):
        raise ValueError("cutpoint_prior must be a dict with 'sd'.") from None
    if extra or not (math.isfinite(sd) and sd > 0.):
        raise ValueError("cutpoint_prior takes a finite, positive 'sd' and "
                         "nothing else.")
    return {'sd': sd}


def check_cutpoints(cuts, n_category):
    """K - 1 finite, strictly increasing numbers as a float64 array."""
    try:
        cuts = np.array(cuts, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("The cutpoints must be numbers.") from None
    if cuts.shape != (n_category - 1,):
        raise ValueError(
            "%d categories take %d cutpoints: shape %s."
            % (n_category, n_category - 1, cuts.shape))
    if not np.all(np.isfinite(cuts)) or np.any(np.diff(cuts) <= 0.):
        raise ValueError(
            "The cutpoints must be finite and strictly increasing.")
    return cuts


def initial_cutpoints(y, n_category):
    """The empirical logits of the cumulative category proportions (every
    category holds a row, so they are finite and strictly increasing)."""
    counts = np.bincount(np.asarray(y).astype(np.intp), minlength=n_category)
    cum = np.cumsum(counts)[:-1] / float(len(y))
    return np.log(cum) - np.log1p(-cum)


def log_conditional(model, coef, cuts, k, prior, state=None, gap_term=True):
    """f of cutpoint k (0-based) given the others: a callable on a 1-D array of
    up to 8 points.  `state`: {'coef': coef} shared by the K - 1 conditionals
    of one sweep, so that only the sweep's first launch forms the linear
    predictor and the later ones reuse it.  gap_term=False evaluates L
    through model.cutpoint_loglik(..., gap_term=False) -- the wrong target,
    for the tests' negative control; only the oracle takes it."""
    cuts = np.array(cuts, dtype=np.float64)
    lower = cuts[k - 1] if k > 0 else -math.inf
    upper = cuts[k + 1] if k + 1 < len(cuts) else math.inf
    half_prec = .5 / prior['sd'] ** 2
    if state is None:
        state = {'coef': coef}
    extra = {} if gap_term else {'gap_term': False}

    def f(points):
        points = np.asarray(points, dtype=np.float64)
        ok = (points > lower) & (points < upper)
        out = np.full(points.shape, -np.inf)
        if ok.any():
            cand = np.repeat(cuts[None, :], int(ok.sum()), axis=0)
            cand[:, k] = points[ok]
            loglik = np.asarray(model.cutpoint_loglik(state['coef'], cand,
                                                      **extra))
            state['coef'] = None
            out[ok] = loglik - half_prec * points[ok] ** 2
        return out

    return f


def update_cutpoints(model, coef, cuts, prior, uniform, gap_term=True):
    """The Gibbs step: for k = 1 ... K - 1 in that order, c_k | coef and the
    other cutpoints by one slice update on c_k itself.  The uniforms are
    consumed in slice_update's documented order, cutpoint by cutpoint.
    Returns the new cutpoints; the model's own are not touched."""
    cuts = np.array(cuts, dtype=np.float64)
    state = {'coef': coef}
    for k in range(len(cuts)):
        f = log_conditional(model, coef, cuts, k, prior, state, gap_term)
        cuts[k] = slice_update(cuts[k], f, uniform)
    return cuts
