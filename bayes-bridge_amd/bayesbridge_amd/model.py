"""Likelihood models on top of the HIP design operator
(model/factory.py:10-68, linear_model.py:6-45, logistic_model.py:6-116,
cox_model.py:7-303).  The Cox likelihood, its gradient and its Hessian-vector
products run on the device (csrc/cox.hip); its coefficients are drawn by HMC
(hmc.py).  The logit model has the same device path (csrc/logit.hip) for the
'hmc' and 'nuts' coefficient samplers, and the Poisson model (csrc/poisson.hip;
with strata the conditional Poisson model, csrc/cpoisson.hip) has no other.
With entry times the Cox model is the counting-process form
(csrc/cox_interval.hip); with ties='efron' tied event times take Efron's
approximation (csrc/cox_efron.hip); with weights= every row carries a case
weight (the weighted partial likelihood, csrc/cox_weighted.hip).  Every Cox
model also gives its cumulative baseline hazard, its martingale residuals and
the posterior survival of new rows (csrc/cox_family.hpp,
csrc/cox_predict.hip).  The linear, logit and Poisson models predict from
their draws -- posterior mean and spread, log pointwise predictive density,
WAIC -- with the draws' linear predictors kept on the device
(csrc/predict.hip).  The negative-binomial model (csrc/negbin.hip) is the
Poisson model's overdispersed sibling: the same device path, one more
parameter -- the dispersion, updated by dispersion.py inside the Gibbs loop --
and the same prediction (csrc/negbin_predict.hip).  The Weibull model
(csrc/weibull.hip) is the parametric proportional-hazards model of
right-censored times on the same device path: its shape is updated by
weibull_shape.py inside the Gibbs loop, and it predicts median survival times
(csrc/weibull_predict.hip) and survival curves.  The ordinal model
(csrc/ordinal.hip) is the proportional-odds model of an ordered outcome on the
same device path: its K - 1 cutpoints are updated by cutpoints.py inside the
Gibbs loop, and it predicts the K category probabilities
(csrc/ordinal_predict.hip)."""
import math
from ctypes import byref, c_double, c_int, c_void_p
from warnings import catch_warnings, simplefilter, warn

import numpy as np
import scipy.sparse as sparse

from . import _lib
from .device_chain import checked_quantile as _checked_quantile
from .design_matrix import (HipDenseDesignMatrix, HipDesignMatrix,
                            HipSparseDesignMatrix)


class _Model():

    @property
    def n_obs(self):
        return self.design.shape[0]

    @property
    def n_pred(self):
        return self.design.shape[1]

    @property
    def intercept_added(self):
        return self.design.intercept_added


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _coef_draws(coef, n_pred):
    """coef (P,) or (P, S) as (the draws (S, P) C-contiguous, whether a draw
    axis was given)."""
    coef = np.asarray(coef, dtype=np.float64)
    if coef.ndim not in (1, 2) or coef.shape[0] != n_pred or coef.size == 0:
        raise ValueError(
            "coef must have shape (%d,) or (%d, n_draw): %s."
            % (n_pred, n_pred, coef.shape))
    many = coef.ndim == 2
    coef = coef.reshape(n_pred, -1)
    # draw-major, 256 coefficients at a time: a block stays in cache, which
    # halves the time of the strided copy at 50 000 x 256
    draws = np.empty(coef.shape[::-1])
    for j in range(0, n_pred, 256):
        draws[:, j:j + 256] = coef[j:j + 256].T
    return draws, many


def _new_design(train, X_new, add_intercept):
    """X_new (raw columns) as a design centred with the TRAINING design's
    column offsets, by the constructors that keep constant columns."""
    offset = train.column_offset if train.centered else None
    if sparse.issparse(X_new):
        X_new = X_new.tocsr().copy()
        X_new.sort_indices()
        return HipSparseDesignMatrix.from_csr_arrays(
            X_new.shape, X_new.indptr, X_new.indices, X_new.data,
            column_offset=offset, add_intercept=add_intercept,
            device=train.device)
    import torch
    dev = 'cuda:%d' % train.device
    X_dev = torch.from_numpy(
        np.ascontiguousarray(X_new, dtype=np.float64)).to(dev)
    off_dev = None
    if offset is not None:
        off_dev = torch.from_numpy(
            np.ascontiguousarray(offset, dtype=np.float64)).to(dev)
    torch.cuda.synchronize(train.device)
    # (the arrays are copied: the tensors may go once it returns)
    return HipDenseDesignMatrix.from_device_array(
        X_new.shape[0], X_new.shape[1], X_dev.data_ptr(),
        off_dev.data_ptr() if off_dev is not None else None,
        add_intercept=add_intercept, device=train.device, in_dtype='float64',
        storage_dtype=getattr(train, 'storage_dtype', 'float64'))


def _binomial_outcome(n_success, n_trial, n_row):
    """The outcome checks of logistic_model.py:10-47 on n_row rows:
    (n_success, n_trial, whether n_trial was left out)."""
    n_success = np.asarray(n_success, dtype=np.float64)
    binary_default = n_trial is None
    if binary_default:
        if n_success.size and n_success.max() > 1:
            raise ValueError(
                "n_trial is required when the outcome is not binary.")
        n_trial = np.ones(n_success.shape)
    else:
        n_trial = np.asarray(n_trial, dtype=np.float64)
    if not (n_success.shape == n_trial.shape == (n_row,)):
        raise ValueError(
            "Outcome vectors and design matrix have incompatible sizes: "
            "%s successes, %s trials, %d rows."
            % (n_success.shape, n_trial.shape, n_row))
    if not binary_default:
        if (n_trial <= 0).any():
            raise ValueError("Every n_trial must be strictly positive.")
        if (n_success > n_trial).any():
            raise ValueError("n_success exceeds n_trial in some row.")
    return n_success, n_trial, binary_default


def _count_outcome(y, exposure, n_row):
    """The outcome checks of the Poisson model on n_row rows: (y, exposure)."""
    y = np.asarray(y, dtype=np.float64)
    if exposure is None:
        exposure = np.ones(y.shape)
    else:
        exposure = np.asarray(exposure, dtype=np.float64)
    if not (y.shape == exposure.shape == (n_row,)):
        raise ValueError(
            "Outcome vectors and design matrix have incompatible sizes: "
            "%s counts, %s exposures, %d rows."
            % (y.shape, exposure.shape, n_row))
    if not np.all(np.isfinite(y)) or (y < 0).any() \
            or (y != np.floor(y)).any():
        raise ValueError("Every count must be a non-negative integer.")
    if not np.all(np.isfinite(exposure)) or (exposure <= 0).any():
        raise ValueError(
            "Every exposure must be strictly positive and finite.")
    return y, exposure


def _log_factorial(x):
    """gammaln(x + 1).  Counts are small integers over and over: they take
    the value from a table of gammaln itself (the same bits) instead of one
    evaluation per row."""
    from scipy.special import gammaln
    x = np.asarray(x, dtype=np.float64)
    if x.size and np.all(np.isfinite(x)) and 0 <= x.min() \
            and x.max() <= 1 << 20:
        k = x.astype(np.intp)
        if np.array_equal(k, x):
            return gammaln(np.arange(k.max() + 1) + 1.)[k]
    return gammaln(x + 1.)


class _Predictive():
    """Posterior prediction and pointwise predictive scores of the linear,
    logit, Poisson, negative-binomial and ordinal models
    (bbx_design_predictive_summary and its two siblings, csrc/predict.hip):
    the draws' linear predictors stay on the device, one kernel reduces them
    per row, n-vectors come back.  A model checks its own outcome arguments
    in its `predict`, which ends in `_predictive_summary`; `_pred_call` names
    its entry point (the linear, logit and Poisson models: the shared one,
    under their `_pred_family`)."""

    def _predict_rows(self, coef, X_new):
        """The shared checks of every predict: (draws (S, P), X_new as an
        array or SciPy matrix or None, the number of rows)."""
        draws, _ = _coef_draws(coef, self.n_pred)
        if X_new is None:
            return draws, None, self.n_obs
        if not sparse.issparse(X_new):
            X_new = np.asarray(X_new, dtype=np.float64)
        n_col = self.n_pred - int(bool(self.intercept_added))
        if X_new.ndim != 2 or X_new.shape[1] != n_col \
                or X_new.shape[0] == 0:
            raise ValueError(
                "X_new must have at least one row and the model's %d "
                "columns: shape %s." % (n_col, X_new.shape))
        train = self.design
        if train.centered and train.column_offset is None:
            raise TypeError(
                "The training design was adopted from device pointers "
                "and keeps no host copy of its column offsets: X_new "
                "cannot be centred with them.")
        return draws, X_new, X_new.shape[0]

    def _pred_call(self, n_draw, draws, obs_prec, offset, y, n_trial,
                   ll_const):
        """(The entry point, its integers after the design, its input
        arrays): what stands before draws_per_pass in the C call."""
        return 'bbx_design_predictive_summary', (self._pred_family, n_draw), \
            (draws, obs_prec, offset, y, n_trial, ll_const)

    def _predictive_summary(self, draws, X_new, n_row, y=None, obs_prec=None,
                            offset=None, n_trial=None, ll_const=None,
                            return_draws=False, draws_per_pass=0,
                            n_plane=None, tail=()):
        """Every check is done: the device from here on.  obs_prec is the
        family's per-draw input (the negative binomial's dispersion, the
        ordinal model's cutpoints (S, K - 1)).  n_plane=K: 'mean' and 'sd'
        are (n, K), and the entry point has no argument for the draws.  tail:
        what the entry point takes after the draws (the censored model's
        survival summary)."""
        n_draw = len(draws)
        if y is not None and n_draw < 2:
            raise ValueError(
                "Scoring an outcome needs at least 2 draws (loglik_var is a "
                "variance over the draws): coef holds %d." % n_draw)
        if X_new is None:
            design = self.design
        else:
            design = _new_design(self.design, X_new,
                                 bool(self.intercept_added))
        if not getattr(design, 'use_hip', False):
            raise TypeError("prediction needs a HipDesignMatrix")
        obs_prec, offset, y, n_trial, ll_const = (
            None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            for a in (obs_prec, offset, y, n_trial, ll_const))
        entry, integers, arrays = self._pred_call(
            n_draw, draws, obs_prec, offset, y, n_trial, ll_const)
        shape = (n_row,) if n_plane is None else (n_plane, n_row)
        mean, sd = np.empty(shape), np.empty(shape)
        score = [np.empty(n_row) if y is not None else None for _ in range(3)]
        out = np.empty((n_draw, n_row)) if return_draws else None
        _lib.check(getattr(_lib.load(), entry)(
            design.handle, *integers, *[_ptr(a) for a in arrays],
            int(draws_per_pass), _ptr(mean), _ptr(sd),
            *[_ptr(a) for a in score], *([_ptr(out)] if n_plane is None
                                         else []), *tail))
        res = {'mean': mean, 'sd': sd} if n_plane is None \
            else {'mean': mean.T, 'sd': sd.T}
        if y is not None:
            lpd, ll_mean, ll_var = score
            lppd, p_waic = float(np.sum(lpd)), float(np.sum(ll_var))
            res.update({'lpd': lpd, 'loglik_mean': ll_mean,
                        'loglik_var': ll_var, 'lppd': lppd, 'p_waic': p_waic,
                        'waic': -2. * (lppd - p_waic)})
        if return_draws:
            res['draws'] = out.T
        return res


def _training_rows_only(X_new, **given):
    """With X_new=None the rows are the training rows and their outcome is
    the model's own: no outcome argument may be given."""
    if X_new is None:
        for name, value in given.items():
            if value is not None:
                raise ValueError(
                    "%s is an argument of new rows only: without X_new the "
                    "training rows are predicted, with the model's own "
                    "outcome." % name)


class LinearModel(_Predictive, _Model):

    _pred_family = _lib.PRED_LINEAR

    def __init__(self, y, design):
        self.y = np.asarray(y, dtype=np.float64)
        self.design = design
        self.name = 'linear'
        if len(self.y) != design.shape[0]:
            raise ValueError(
                "Incompatible sizes of the outcome and design matrix.")

    def compute_loglik_and_gradient(self, beta, obs_prec, loglik_only=False):
        X_beta = self.design.dot(beta)              # linear_model.py:13-22
        loglik = (len(self.y) * math.log(obs_prec) / 2
                  - obs_prec * np.sum((self.y - X_beta) ** 2) / 2)
        grad = None
        if not loglik_only:
            grad = obs_prec * self.design.Tdot(self.y - X_beta)
        return loglik, grad

    def calc_intercept_mle(self):
        return self.y.mean()

    def predict(self, coef, X_new=None, y_new=None, obs_prec=None,
                return_draws=False, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is -- with obs_prec (S,) -- samples['obs_prec'].
        X_new=None: the training rows with the model's own outcome;
        otherwise n_new rows of the model's raw columns (NumPy or SciPy),
        centred with the TRAINING design's column means, with y_new or
        without.  A dict: 'mean' and 'sd' (n,), the posterior mean of
        E[y | x] and its population standard deviation over the draws; with
        an outcome 'lpd' (the log pointwise predictive density of every
        row), 'loglik_mean' and 'loglik_var' (n,) and the floats 'lppd' =
        sum lpd, 'p_waic' = sum loglik_var and 'waic' = -2 (lppd - p_waic),
        the log density being the normal's with precision obs_prec; with
        return_draws 'draws' (n, S).  One device call for all the draws."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new)
        y = self.y if X_new is None else y_new
        if y is not None:
            y = np.asarray(y, dtype=np.float64)
            if y.shape != (n_row,):
                raise ValueError(
                    "Incompatible sizes of the outcome and design matrix.")
        if obs_prec is None:
            raise ValueError(
                "obs_prec (one observation precision per draw, "
                "samples['obs_prec']) is required.")
        obs_prec = np.asarray(obs_prec, dtype=np.float64).reshape(-1)
        if obs_prec.shape != (len(draws),):
            raise ValueError(
                "obs_prec must hold one value per draw: %d values, %d draws."
                % (len(obs_prec), len(draws)))
        if not np.all(np.isfinite(obs_prec)) or (obs_prec <= 0).any():
            raise ValueError(
                "Every obs_prec must be strictly positive and finite.")
        ll_const = None
        if y is not None:
            ll_const = np.full(n_row, -.5 * math.log(2. * math.pi))
        return self._predictive_summary(
            draws, X_new, n_row, y=y, obs_prec=obs_prec, ll_const=ll_const,
            return_draws=return_draws, draws_per_pass=_draws_per_pass)

    @staticmethod
    def simulate_outcome(X, beta, noise_sd, seed=None):
        if seed is not None:
            np.random.seed(seed)
        return X.dot(beta) + noise_sd * np.random.randn(X.shape[0])


class _DeviceHamiltonian():
    """The device trajectory and No-U-Turn tree of a likelihood handle
    (csrc/hamiltonian.hpp): the same calls on bbx_cox_*, bbx_logit_*,
    bbx_poisson_* and bbx_cpoisson_*.  A model names its family in
    `_ham_prefix`, gives its handle as `handle` and keeps it in the attribute
    that `_handle_attr` names."""

    def _ham_fn(self, name):
        return getattr(_lib.load(), self._ham_prefix + name)

    def __del__(self):
        h = getattr(self, self._handle_attr, None)
        if h and not _lib.finalizing:
            self._ham_fn('destroy')(h)
        setattr(self, self._handle_attr, c_void_p())

    def _device_loglik_and_gradient(self, beta, loglik_only=False,
                                    inf_has_no_gradient=True):
        """bbx_<family>_loglik_grad at beta: (loglik, gradient or None);
        (-inf, None) where the likelihood is -inf, unless told otherwise."""
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        if beta.shape != (self.n_pred,):
            raise ValueError("beta must have length %d" % self.n_pred)
        loglik = c_double()
        grad = None if loglik_only else np.empty(self.n_pred)
        _lib.check(self._ham_fn('loglik_grad')(
            self.handle, _ptr(beta), byref(loglik), _ptr(grad)))
        if inf_has_no_gradient and loglik.value == -float('inf'):
            return -float('inf'), None
        return loglik.value, grad

    def _hessian_operator(self, beta):
        """The handle holds one location: an operator stops working once a
        later call has moved it."""
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        if beta.shape != (self.n_pred,):
            raise ValueError("beta must have length %d" % self.n_pred)
        st = self._ham_fn('set_location')(self.handle, _ptr(beta))
        self._location_serial += 1
        if st == _lib.ERR_NUMERIC:
            raise ValueError(
                'Hessian operator cannot be computed likely due to an '
                'unreasonable value of regression coefficients. This could '
                'be caused by the likelihood and prior both being too weak '
                'or by a poor initialization of the Markov chain.')
        _lib.check(st)
        serial = self._location_serial
        matvec, handle = self._ham_fn('hessian_matvec'), self.handle

        def hessian_op(v):
            if serial != self._location_serial:
                raise RuntimeError("the Hessian location has moved since this "
                                   "operator was made")
            v = np.ascontiguousarray(np.ravel(v), dtype=np.float64)
            if v.shape != (self.n_pred,):
                raise ValueError("v must have length %d" % self.n_pred)
            out = np.empty(self.n_pred)
            _lib.check(matvec(handle, _ptr(v), _ptr(out)))
            return out

        return hessian_op

    def hmc_trajectory(self, dt, n_step, precond_scale, prior_prec, q0, p0,
                       logp0, grad0, hamiltonian_tol=100.):
        """n_step velocity-Verlet steps on the device (bbx_<family>_hmc_trajectory,
        one host synchronisation).  Returns a dict: q, p, logp, grad (None if
        logp is not finite), n_steps (steps taken), instability and
        hamiltonian = [H at the start, H at the end]."""
        P = self.n_pred
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (
            precond_scale, prior_prec, q0, p0, grad0)]
        if any(a.shape != (P,) for a in arrays):
            raise ValueError("trajectory vectors must have length %d" % P)
        q, p, grad, ham = np.empty(P), np.empty(P), np.empty(P), np.empty(2)
        logp, n_steps, instab = c_double(), c_int(), c_int()
        _lib.check(self._ham_fn('hmc_trajectory')(
            self.handle, float(dt), int(n_step), *[_ptr(a) for a in arrays[:4]],
            float(logp0), _ptr(arrays[4]), float(hamiltonian_tol), _ptr(q),
            _ptr(p), byref(logp), _ptr(grad), byref(n_steps), byref(instab),
            _ptr(ham)))
        return {'q': q, 'p': p, 'logp': logp.value,
                'grad': grad if math.isfinite(logp.value) else None,
                'n_steps': n_steps.value, 'instability': bool(instab.value),
                'hamiltonian': ham}

    def nuts_begin(self, precond_scale, prior_prec, q0, p0, logp0, grad0,
                   joint_logp0, joint_logp_threshold, hamiltonian_tol=100.):
        """Installs the single-state trajectory tree of a NUTS draw on the
        handle (bbx_<family>_nuts_begin; see nuts.py)."""
        P = self.n_pred
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (
            precond_scale, prior_prec, q0, p0, grad0)]
        if any(a.shape != (P,) for a in arrays):
            raise ValueError("trajectory vectors must have length %d" % P)
        _lib.check(self._ham_fn('nuts_begin')(
            self.handle, *[_ptr(a) for a in arrays[:4]], float(logp0),
            _ptr(arrays[4]), float(joint_logp0), float(joint_logp_threshold),
            float(hamiltonian_tol)))

    def nuts_doubling(self, dt, direction, height, uniforms):
        """Doubles the tree by a half-tree of 2^height leapfrog steps in
        `direction` (bbx_<family>_nuts_doubling: one enqueue, one host wait).
        uniforms: the 2^height numbers the merges may consume."""
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        if height < 0 or uniforms.shape != (2 ** height,):
            raise ValueError("a half-tree of height h takes 2^h uniforms")
        n_unif, n_steps = c_int(), c_int()
        flags, tree = np.zeros(3, np.int32), np.zeros(2, np.int32)
        ave = np.zeros(2)
        _lib.check(self._ham_fn('nuts_doubling')(
            self.handle, float(dt), int(direction), int(height), _ptr(uniforms),
            byref(n_unif), byref(n_steps), _ptr(flags), _ptr(tree),
            _ptr(ave)))
        return {'n_uniform': n_unif.value, 'n_steps': n_steps.value,
                'u_turn_detected': bool(flags[0]),
                'instability_detected': bool(flags[1]),
                'doubling_rejected': bool(flags[2]),
                'height': int(tree[0]), 'n_acceptable_state': int(tree[1]),
                'ave_hamiltonian_error': float(ave[0]),
                'ave_accept_prob': float(ave[1])}

    def nuts_sample(self):
        """(q, logp, grad) of the tree's sample (bbx_<family>_nuts_sample)."""
        q, grad = np.empty(self.n_pred), np.empty(self.n_pred)
        logp = c_double()
        _lib.check(self._ham_fn('nuts_sample')(
            self.handle, _ptr(q), byref(logp), _ptr(grad)))
        return q, logp.value, grad


class LogisticModel(_DeviceHamiltonian, _Predictive, _Model):

    _handle_attr = '_logit'
    _pred_family = _lib.PRED_LOGIT

    def __init__(self, n_success, n_trial, design):
        """Outcome checks of logistic_model.py:10-47: counts must line up with
        the rows of the design, 0 < n_trial, n_success <= n_trial; without
        n_trial the outcome has to be 0/1."""
        n_success, n_trial, binary_default = _binomial_outcome(
            n_success, n_trial, design.shape[0])
        if binary_default:
            warn("n_trial not given: treating the outcome as binary.")
        self.n_success = n_success
        self.n_trial = n_trial
        self.design = design
        self.name = 'logit'
        # the device likelihood of the 'hmc' / 'nuts' samplers: one bbx_logit
        # handle, made by the first call that needs it
        self._ham_prefix = 'bbx_logit_'
        self._logit = c_void_p()
        self._location_serial = 0

    @property
    def handle(self):
        if not self._logit:
            if not getattr(self.design, 'use_hip', False):
                raise TypeError("the device likelihood needs a HipDesignMatrix")
            y = np.ascontiguousarray(self.n_success, dtype=np.float64)
            m = np.ascontiguousarray(self.n_trial, dtype=np.float64)
            _lib.check(_lib.load().bbx_logit_create(
                self.design.handle, _ptr(y), _ptr(m), byref(self._logit)))
        return self._logit

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        logit_prob = self.design.dot(beta)           # logistic_model.py:49-60
        loglik = np.sum(self.n_success * logit_prob
                        - self.n_trial * np.logaddexp(0, logit_prob))
        grad = None
        if not loglik_only:
            prob = 1 / (1 + np.exp(-logit_prob))
            grad = self.design.Tdot(self.n_success - self.n_trial * prob)
        return loglik, grad

    def hamiltonian_loglik_and_gradient(self, beta, loglik_only=False):
        """The same likelihood on the device (bbx_logit_loglik_grad: fixed
        summation orders, the gradient's X~^T product without a host round
        trip): what the 'hmc' and 'nuts' samplers evaluate.  The other
        samplers keep compute_loglik_and_gradient."""
        return self._device_loglik_and_gradient(beta, loglik_only,
                                                inf_has_no_gradient=False)

    def get_hessian_matvec_operator(self, beta):
        """logistic_model.py:68-74 on the device."""
        return self._hessian_operator(beta)

    def calc_intercept_mle(self):
        p_hat = self.n_success.mean() / self.n_trial.mean()
        return np.log(p_hat / (1 - p_hat))

    def predict(self, coef, X_new=None, y_new=None, n_trial_new=None,
                return_draws=False, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is.  X_new=None: the training rows with the model's
        own successes and trials; otherwise n_new rows of the model's raw
        columns (NumPy or SciPy), centred with the TRAINING design's column
        means, with y_new (successes; n_trial_new as in the constructor) or
        without.  A dict: 'mean' and 'sd' (n,), the posterior mean of the
        success probability per trial and its population standard deviation
        over the draws; with an outcome 'lpd' (the log pointwise predictive
        density of every row), 'loglik_mean' and 'loglik_var' (n,) and the
        floats 'lppd' = sum lpd, 'p_waic' = sum loglik_var and 'waic' =
        -2 (lppd - p_waic), the log density being the binomial's with its
        coefficient; with return_draws 'draws' (n, S).  One device call for
        all the draws."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new, n_trial_new=n_trial_new)
        y = m = ll_const = None
        if X_new is None:
            y, m = self.n_success, self.n_trial
        elif y_new is not None:
            y, m, _ = _binomial_outcome(y_new, n_trial_new, n_row)
            # (what bbx_logit_create refuses)
            if not np.all(np.isfinite(y)) or not np.all(np.isfinite(m)) \
                    or (y < 0).any():
                raise ValueError(
                    "Every count must be finite and non-negative.")
        elif n_trial_new is not None:
            raise ValueError("n_trial_new is an argument of scoring only: "
                             "y_new is not given.")
        if y is not None:
            ll_const = (_log_factorial(m) - _log_factorial(y)
                        - _log_factorial(m - y))
        return self._predictive_summary(
            draws, X_new, n_row, y=y, n_trial=m, ll_const=ll_const,
            return_draws=return_draws, draws_per_pass=_draws_per_pass)

    @staticmethod
    def compute_polya_gamma_mean(shape, tilt):
        """logistic_model.py:80-87 (including its b/2 value at |tilt| <= 1e-5)."""
        pg_mean = shape.copy() / 2
        nz = (np.abs(tilt) > 1e-5)
        pg_mean[nz] *= 1 / tilt[nz] * (np.exp(tilt[nz]) - 1) \
            / (np.exp(tilt[nz]) + 1)
        return pg_mean

    @staticmethod
    def simulate_outcome(n_trial, X, beta, seed=None):
        prob = 1 / (1 + np.exp(-X.dot(beta)))
        if seed is not None:
            np.random.seed(seed)
        return np.random.binomial(n_trial, prob)


def _binary_outcome(y, n_row):
    """The outcome check of the probit model on n_row rows: y in {0, 1}."""
    if isinstance(y, tuple):
        raise ValueError(
            "The probit model takes a binary outcome y, not (n_success, "
            "n_trial): a binomial outcome is the logit model's "
            "(family='logit').")
    y = np.asarray(y, dtype=np.float64)
    if y.shape != (n_row,):
        raise ValueError(
            "Incompatible sizes of the outcome and design matrix: %s "
            "outcomes, %d rows." % (y.shape, n_row))
    bad = np.flatnonzero(~((y == 0.) | (y == 1.)))
    if bad.size:
        raise ValueError(
            "The probit model takes a binary outcome: y[%d] = %r is not 0 "
            "or 1." % (bad[0], float(y[bad[0]])))
    return y


class ProbitModel(_Predictive, _Model):
    """Binary regression with the probit link, P(y_i = 1) = Phi(eta_i), no
    counterpart in the reference.  Under Albert & Chib's augmentation, z_i |
    beta ~ N(eta_i, 1) truncated to z > 0 (y_i = 1) or z <= 0 (y_i = 0), the
    coefficients' conditional is the linear model's with outcome z and the
    observation precision fixed at 1: the chain draws them with 'cg',
    'cholesky' or 'woodbury' on the device (csrc/probit.hip draws z).  The
    augmentation mixes slowly on very imbalanced outcomes, as Polya-Gamma
    does."""

    def __init__(self, y, design):
        self.y = _binary_outcome(y, design.shape[0])
        self.n_success = self.y          # what the device chain is handed
        self.design = design
        self.name = 'probit'

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        """sum_i log Phi(s_i eta_i), s_i = 2 y_i - 1, and its gradient
        X~^T (s phi(eta) / Phi(s eta))."""
        from scipy.special import log_ndtr
        eta = self.design.dot(beta)
        s = 2. * self.y - 1.
        ll = log_ndtr(s * eta)
        grad = None
        if not loglik_only:
            hazard = np.exp(-.5 * eta * eta - .5 * math.log(2. * math.pi) - ll)
            grad = self.design.Tdot(s * hazard)
        return float(np.sum(ll)), grad

    def calc_intercept_mle(self):
        from scipy.special import ndtri
        return float(ndtri(self.y.mean()))

    def _pred_call(self, n_draw, draws, obs_prec, offset, y, n_trial,
                   ll_const):
        return 'bbx_design_predictive_summary_probit', (n_draw,), \
            (draws, offset, y, ll_const)

    def predict(self, coef, X_new=None, y_new=None, return_draws=False,
                _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is.  X_new=None: the training rows with the model's
        own outcome; otherwise n_new rows of the model's raw columns (NumPy or
        SciPy), centred with the TRAINING design's column means, with a
        binary y_new or without.  A dict: 'mean' and 'sd' (n,), the posterior
        mean of Phi(eta) and its population standard deviation over the
        draws; with an outcome 'lpd', 'loglik_mean' and 'loglik_var' (n,) and
        the floats 'lppd' = sum lpd, 'p_waic' = sum loglik_var and 'waic' =
        -2 (lppd - p_waic), the log density being log Phi(eta) for y = 1 and
        log Phi(-eta) for y = 0; with return_draws 'draws' (n, S).  One
        device call for all the draws."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new)
        y = self.y if X_new is None else y_new
        if y is not None:
            y = _binary_outcome(y, n_row)
        return self._predictive_summary(
            draws, X_new, n_row, y=y, return_draws=return_draws,
            draws_per_pass=_draws_per_pass)

    @staticmethod
    def simulate_outcome(X, beta, seed=None):
        """y_i = 1 when eta_i + a standard normal is positive."""
        rng = np.random.default_rng(seed)
        return (X.dot(beta) + rng.standard_normal(X.shape[0]) > 0.) \
            .astype(np.float64)


def _finite_outcome(y, n_row, who='Student-t'):
    """The outcome check of the Student-t and quantile models (`who`) on n_row
    rows: y finite."""
    if isinstance(y, tuple):
        raise ValueError(
            "The %s model takes a continuous outcome y, not a tuple." % who)
    y = np.asarray(y, dtype=np.float64)
    if y.shape != (n_row,):
        raise ValueError(
            "Incompatible sizes of the outcome and design matrix: %s "
            "outcomes, %d rows." % (y.shape, n_row))
    bad = np.flatnonzero(~np.isfinite(y))
    if bad.size:
        raise ValueError(
            "The %s model takes a finite outcome: y[%d] = %r."
            % (who, bad[0], float(y[bad[0]])))
    return y


def _checked_df(df):
    try:
        value = float(df)
    except (TypeError, ValueError):
        value = float('nan')
    if not (value > 0. and math.isfinite(value)):
        raise ValueError(
            "The degrees of freedom df must be finite and positive: %r."
            % (df,))
    return value


class StudentTModel(_Predictive, _Model):
    """Linear regression with Student-t errors, y_i = eta_i + e_i with
    e_i sqrt(tau) ~ t on `df` degrees of freedom (fixed; Gelman's default 4),
    no counterpart in the reference.  As a scale mixture of normals, omega_i
    ~ Gamma(df/2, rate df/2) and y_i | omega_i ~ N(eta_i, 1 / (tau omega_i)),
    the coefficients' conditional is Gaussian with the per-row precision tau
    omega_i: the chain draws them with 'cg', 'cholesky' or 'woodbury' on the
    device (csrc/student_t.hip draws tau and omega).  An outlying row gets a
    small omega_i and with it a small say in the fit."""

    def __init__(self, y, design, df=4.):
        self.y = _finite_outcome(y, design.shape[0])
        self.df = _checked_df(df)
        self.design = design
        self.name = 'student_t'

    def compute_loglik_and_gradient(self, beta, obs_prec=1.,
                                    loglik_only=False):
        """The chain's log-likelihood, sum_i [1/2 log tau - (df+1)/2
        log1p(tau r_i^2 / df)] + n [lgamma((df+1)/2) - lgamma(df/2) -
        1/2 log(df/2)] (the linear model's convention: -n/2 log 2 pi
        dropped), and its gradient X~^T ((df+1) tau r / (df + tau r^2))."""
        nu, tau = self.df, float(obs_prec)
        r = self.y - self.design.dot(beta)
        const = math.lgamma((nu + 1.) / 2.) - math.lgamma(nu / 2.) \
            - .5 * math.log(nu / 2.)
        loglik = float(np.sum(.5 * math.log(tau) - (nu + 1.) / 2.
                              * np.log1p(tau * r * r / nu))
                       + len(r) * const)
        grad = None
        if not loglik_only:
            grad = self.design.Tdot((nu + 1.) * tau * r / (nu + tau * r * r))
        return loglik, grad

    def calc_intercept_mle(self):
        """The median of y: what a heavy tail does not drag."""
        return float(np.median(self.y))

    def _pred_call(self, n_draw, draws, obs_prec, offset, y, n_trial,
                   ll_const):
        return 'bbx_design_predictive_summary_student_t', \
            (n_draw, self.df), (draws, obs_prec, offset, y, ll_const)

    def predict(self, coef, obs_prec=None, X_new=None, y_new=None,
                return_draws=False, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is -- with obs_prec (S,) -- samples['obs_prec'], the
        draws' tau.  X_new=None: the training rows with the model's own
        outcome; otherwise n_new rows of the model's raw columns (NumPy or
        SciPy), centred with the TRAINING design's column means, with y_new or
        without.  A dict: 'mean' and 'sd' (n,), the posterior mean of eta
        (E[y | x] for df > 1) and its population standard deviation over the
        draws; with an outcome 'lpd', 'loglik_mean' and 'loglik_var' (n,) and
        the floats 'lppd' = sum lpd, 'p_waic' = sum loglik_var and 'waic' =
        -2 (lppd - p_waic), the log density being the full t-density on df
        degrees of freedom with precision obs_prec; with return_draws 'draws'
        (n, S).  One device call for all the draws."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new)
        y = self.y if X_new is None else y_new
        if y is not None:
            y = _finite_outcome(y, n_row)
        if obs_prec is None:
            raise ValueError(
                "obs_prec (one observation precision per draw, "
                "samples['obs_prec']) is required.")
        obs_prec = np.asarray(obs_prec, dtype=np.float64).reshape(-1)
        if obs_prec.shape != (len(draws),):
            raise ValueError(
                "obs_prec must hold one value per draw: %d values, %d draws."
                % (len(obs_prec), len(draws)))
        if not np.all(np.isfinite(obs_prec)) or (obs_prec <= 0).any():
            raise ValueError(
                "Every obs_prec must be strictly positive and finite.")
        return self._predictive_summary(
            draws, X_new, n_row, y=y, obs_prec=obs_prec,
            return_draws=return_draws, draws_per_pass=_draws_per_pass)

    @staticmethod
    def simulate_outcome(X, beta, df=4., noise_scale=1., seed=None):
        """y_i = eta_i + noise_scale times a Student-t variate on df degrees
        of freedom."""
        rng = np.random.default_rng(seed)
        return np.asarray(X.dot(beta)).ravel() \
            + noise_scale * rng.standard_t(_checked_df(df), X.shape[0])


class QuantileModel(_Predictive, _Model):
    """Regression of the q-th conditional quantile, q = `quantile` fixed in
    (0, 1), no counterpart in the reference: the asymmetric-Laplace
    likelihood p(y_i) = q (1 - q) tau exp(-tau rho_q(y_i - eta_i)) with the
    check function rho_q(u) = u (q - 1[u < 0]), whose mode in eta_i is the
    quantile.  As a scale mixture of normals (Kozumi & Kobayashi 2011), v_i ~
    Exp(rate tau) and y_i | v_i ~ N(eta_i + theta v_i, kappa2 v_i / tau) with
    theta = (1 - 2q) / (q (1 - q)) and kappa2 = 2 / (q (1 - q)), the
    coefficients' conditional is Gaussian with the per-row precision tau /
    (kappa2 v_i): the chain draws them with 'cg', 'cholesky' or 'woodbury' on
    the device (csrc/quantile.hip draws tau and w = 1 / v).  Several levels
    are several fits."""

    def __init__(self, y, design, quantile=.5):
        self.y = _finite_outcome(y, design.shape[0], 'quantile')
        self.quantile = _checked_quantile(quantile)
        self.design = design
        self.name = 'quantile'

    def compute_loglik_and_gradient(self, beta, obs_prec=1.,
                                    loglik_only=False):
        """The chain's log-likelihood, sum_i [log tau - tau rho_q(r_i)] + n
        log(q (1 - q)), and its gradient tau X~^T (q - 1[r < 0]) (a
        subgradient where a residual is zero)."""
        q, tau = self.quantile, float(obs_prec)
        r = self.y - self.design.dot(beta)
        side = np.where(r < 0., q - 1., q)
        loglik = float(np.sum(math.log(tau) - tau * (r * side))
                       + len(r) * math.log(q * (1. - q)))
        grad = None
        if not loglik_only:
            grad = self.design.Tdot(tau * side)
        return loglik, grad

    def calc_intercept_mle(self):
        """The sample q-quantile of y."""
        return float(np.quantile(self.y, self.quantile))

    def _pred_call(self, n_draw, draws, obs_prec, offset, y, n_trial,
                   ll_const):
        return 'bbx_design_predictive_summary_quantile', \
            (n_draw, self.quantile), (draws, obs_prec, offset, y, ll_const)

    def predict(self, coef, obs_prec=None, X_new=None, y_new=None,
                return_draws=False, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is -- with obs_prec (S,) -- samples['obs_prec'], the
        draws' tau.  X_new=None: the training rows with the model's own
        outcome; otherwise n_new rows of the model's raw columns (NumPy or
        SciPy), centred with the TRAINING design's column means, with y_new or
        without.  A dict: 'mean' and 'sd' (n,), the posterior mean of eta
        (the conditional q-quantile) and its population standard deviation
        over the draws; with an outcome 'lpd', 'loglik_mean' and 'loglik_var'
        (n,) and the floats 'lppd' = sum lpd, 'p_waic' = sum loglik_var and
        'waic' = -2 (lppd - p_waic), the log density being the full
        asymmetric-Laplace density at level q with precision obs_prec; with
        return_draws 'draws' (n, S).  One device call for all the draws."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new)
        y = self.y if X_new is None else y_new
        if y is not None:
            y = _finite_outcome(y, n_row, 'quantile')
        if obs_prec is None:
            raise ValueError(
                "obs_prec (one observation precision per draw, "
                "samples['obs_prec']) is required.")
        obs_prec = np.asarray(obs_prec, dtype=np.float64).reshape(-1)
        if obs_prec.shape != (len(draws),):
            raise ValueError(
                "obs_prec must hold one value per draw: %d values, %d draws."
                % (len(obs_prec), len(draws)))
        if not np.all(np.isfinite(obs_prec)) or (obs_prec <= 0).any():
            raise ValueError(
                "Every obs_prec must be strictly positive and finite.")
        return self._predictive_summary(
            draws, X_new, n_row, y=y, obs_prec=obs_prec,
            return_draws=return_draws, draws_per_pass=_draws_per_pass)

    @staticmethod
    def simulate_outcome(X, beta, quantile=.5, noise_scale=1., seed=None):
        """y_i = eta_i + noise_scale times an asymmetric-Laplace variate at
        level q (precision 1), whose q-quantile is 0: e = E1 / q - E2 / (1 -
        q) with two standard exponentials."""
        q = _checked_quantile(quantile)
        rng = np.random.default_rng(seed)
        n = X.shape[0]
        noise = rng.standard_exponential(n) / q \
            - rng.standard_exponential(n) / (1. - q)
        return np.asarray(X.dot(beta)).ravel() + noise_scale * noise


def _censored_outcome(y, status, n_row):
    """The outcome checks of the censored-normal model on n_row rows: y
    finite, status in {0, 1, 2}; (y as float64, status as uint8)."""
    y = np.asarray(y, dtype=np.float64)
    st = np.asarray(status)
    if y.shape != (n_row,) or st.shape != (n_row,):
        raise ValueError(
            "Incompatible sizes of the outcome and design matrix: %s values, "
            "%s status codes, %d rows." % (y.shape, st.shape, n_row))
    bad = np.flatnonzero(~np.isfinite(y))
    if bad.size:
        raise ValueError(
            "The censored model takes finite values: y[%d] = %r."
            % (bad[0], float(y[bad[0]])))
    bad = np.flatnonzero(~((st == 0) | (st == 1) | (st == 2)))
    if bad.size:
        raise ValueError(
            "status must be 0 (observed), 1 (right-censored) or 2 "
            "(left-censored): status[%d] = %r." % (bad[0], st[bad[0]]))
    return y, st.astype(np.uint8)


def _obs_prec_draws(obs_prec, n_draw):
    """One strictly positive, finite observation precision per draw."""
    if obs_prec is None:
        raise ValueError(
            "obs_prec (one observation precision per draw, "
            "samples['obs_prec']) is required.")
    obs_prec = np.asarray(obs_prec, dtype=np.float64).reshape(-1)
    if obs_prec.shape != (n_draw,):
        raise ValueError(
            "obs_prec must hold one value per draw: %d values, %d draws."
            % (len(obs_prec), n_draw))
    if not np.all(np.isfinite(obs_prec)) or (obs_prec <= 0).any():
        raise ValueError(
            "Every obs_prec must be strictly positive and finite.")
    return obs_prec


class CensoredNormalModel(_Predictive, _Model):
    """Linear regression of an outcome that is censored in some rows (the
    Tobit model; no counterpart in the reference): z_i = eta_i + e_i, e_i ~
    N(0, 1 / tau), and row i shows y_i with status_i: 0 -- observed, z_i =
    y_i; 1 -- right-censored, z_i > y_i; 2 -- left-censored, z_i <= y_i.  The
    chain augments the censored rows with truncated-normal latents (Chib
    1992; csrc/censored.hip), after which the coefficients' conditional is the
    linear model's with z for y: 'cg', 'cholesky' and 'woodbury' draw them on
    the device.  The augmentation mixes slowly when most rows are censored:
    the latents and the coefficients then move together in small steps.
    Interval censoring is not supported.  Agreement with R's AER::tobit is
    not tested."""

    _exp_mean = 0

    def __init__(self, y, status, design):
        self.y, self.status = _censored_outcome(y, status, design.shape[0])
        self.design = design
        self.name = 'tobit'

    def compute_loglik_and_gradient(self, beta, obs_prec=1.,
                                    loglik_only=False):
        """The chain's log-likelihood -- sum over observed rows of 1/2 log
        tau - 1/2 tau (y - eta)^2 (the linear model's convention: -1/2 log
        2 pi dropped), over right-censored rows of log Phi(-a) and over
        left-censored rows of log Phi(a), a = (y - eta) sqrt(tau) -- and its
        gradient X~^T g, g = tau (y - eta), sqrt(tau) phi(a) / Phi(-a) and
        -sqrt(tau) phi(a) / Phi(a)."""
        from scipy.special import log_ndtr
        tau = float(obs_prec)
        rt = math.sqrt(tau)
        a = (self.y - self.design.dot(beta)) * rt
        obs, right = self.status == 0, self.status == 1
        sign = np.where(right, -1., 1.)
        tail = log_ndtr(sign * a)
        loglik = float(np.sum(np.where(
            obs, .5 * math.log(tau) - .5 * a * a, tail)))
        grad = None
        if not loglik_only:
            ratio = np.exp(-.5 * a * a - .5 * math.log(2. * math.pi) - tail)
            grad = self.design.Tdot(np.where(obs, rt * a, -sign * rt * ratio))
        return loglik, grad

    def calc_intercept_mle(self):
        """The mean of the values, censored ones at their bounds: a starting
        point, not the maximiser."""
        return float(np.mean(self.y))

    def _pred_call(self, n_draw, draws, obs_prec, offset, y, n_trial,
                   ll_const):
        # (n_trial's place holds the status)
        status = None if n_trial is None else n_trial.astype(np.uint8)
        return 'bbx_design_predictive_summary_censored', \
            (n_draw, self._exp_mean), \
            (draws, obs_prec, offset, y, status, ll_const)

    def _predict_censored(self, coef, obs_prec, X_new, y, status,
                          ll_const=None, return_draws=False,
                          draws_per_pass=0, points=None):
        """predict and predict_survival behind their checks of the outcome:
        y and status on the latent scale or None; points: where the survival
        summary is asked for (the result then has 'surv_mean' and 'surv_sd',
        (n, T))."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        obs_prec = _obs_prec_draws(obs_prec, len(draws))
        if points is None:
            tail = (0, None, None, None)
        else:
            points = np.ascontiguousarray(points, dtype=np.float64)
            surv = np.empty((2, len(points), n_row))
            tail = (len(points), _ptr(points), _ptr(surv[0]), _ptr(surv[1]))
        res = self._predictive_summary(
            draws, X_new, n_row, y=y, obs_prec=obs_prec, n_trial=status,
            ll_const=ll_const, return_draws=return_draws,
            draws_per_pass=draws_per_pass, tail=tail)
        if points is not None:
            res['surv_mean'], res['surv_sd'] = surv[0].T, surv[1].T
        return res

    def predict(self, coef, obs_prec=None, X_new=None, y_new=None,
                status_new=None, return_draws=False, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is -- with obs_prec (S,) -- samples['obs_prec'], the
        draws' tau.  X_new=None: the training rows with the model's own
        outcome; otherwise n_new rows of the model's raw columns (NumPy or
        SciPy), centred with the TRAINING design's column means, with y_new
        and status_new (both) or without.  A dict: 'mean' and 'sd' (n,), the
        posterior mean of eta (the mean of the uncensored outcome) and its
        population standard deviation over the draws; with an outcome 'lpd',
        'loglik_mean' and 'loglik_var' (n,) and the floats 'lppd' = sum lpd,
        'p_waic' = sum loglik_var and 'waic' = -2 (lppd - p_waic), the log
        density being the full one: the normal density with -1/2 log 2 pi on
        an observed row, the log tail probability on a censored one; with
        return_draws 'draws' (n, S).  One device call for all the draws."""
        _training_rows_only(X_new, y_new=y_new, status_new=status_new)
        y = status = None
        if X_new is None:
            y, status = self.y, self.status
        elif y_new is not None or status_new is not None:
            if y_new is None or status_new is None:
                raise ValueError(
                    "y_new and status_new are given together or not at all.")
            y, status = _censored_outcome(y_new, status_new,
                                          np.shape(X_new)[0])
        return self._predict_censored(
            coef, obs_prec, X_new, y, status, return_draws=return_draws,
            draws_per_pass=_draws_per_pass)

    @staticmethod
    def simulate_outcome(X, beta, noise_sd=1., lower=None, upper=None,
                         seed=None):
        """(y, status): z = X beta + noise_sd N(0, 1); a z <= lower is shown
        as lower with status 2, a z > upper as upper with status 1."""
        rng = np.random.default_rng(seed)
        z = np.asarray(X.dot(beta)).ravel() \
            + noise_sd * rng.standard_normal(X.shape[0])
        y, status = z.copy(), np.zeros(len(z), dtype=np.uint8)
        if lower is not None:
            left = z <= lower
            y[left], status[left] = lower, 2
        if upper is not None:
            right = z > upper
            y[right], status[right] = upper, 1
        return y, status


class LogNormalAFTModel(CensoredNormalModel):
    """Accelerated-failure-time regression of right-censored times with
    log-normal errors: log T_i = eta_i + e_i, e_i ~ N(0, 1 / tau), on the
    Weibull model's outcome (event_time, censoring_time).  It is the
    censored-normal model on log t with status 1 for the censored rows, so
    the Gaussian samplers 'cg', 'cholesky' and 'woodbury' draw its
    coefficients.  The coefficients are log TIME ratios: a positive one
    lengthens survival, the opposite sign to the log hazard ratios of the Cox
    and Weibull models.  The augmentation mixes slowly under heavy
    censoring.  Agreement with R's survreg(dist='lognormal') is not
    tested."""

    _exp_mean = 1

    def __init__(self, event_time, censoring_time, design):
        event, time = _survival_outcome(event_time, censoring_time,
                                        design.shape[0])
        super().__init__(np.log(time), (event == 0.).astype(np.uint8), design)
        self.event = event
        self.time = time
        self.log_time = self.y
        self.event_time = np.asarray(event_time, dtype=np.float64)
        self.censoring_time = np.asarray(censoring_time, dtype=np.float64)
        self.name = 'lognormal'

    def predict(self, coef, obs_prec=None, X_new=None, event_time_new=None,
                censoring_time_new=None, return_draws=False,
                _draws_per_pass=0):
        """CensoredNormalModel.predict for times: 'mean' and 'sd' are the
        posterior mean of the median survival time exp(eta) and its population
        standard deviation over the draws; with an outcome (the training
        rows' own, or event_time_new and censoring_time_new together) the
        scores are under the density of t -- the normal density of log t
        with the Jacobian -log t on an event row, log(1 - Phi((log t - eta)
        sqrt(tau))) on a censored one -- which makes 'lppd' and 'waic'
        comparable with WeibullModel.predict's."""
        _training_rows_only(X_new, event_time_new=event_time_new,
                            censoring_time_new=censoring_time_new)
        y = status = None
        if X_new is None:
            y, status = self.y, self.status
        elif event_time_new is not None or censoring_time_new is not None:
            if event_time_new is None or censoring_time_new is None:
                raise ValueError(
                    "event_time_new and censoring_time_new are given "
                    "together or not at all.")
            event, time = _survival_outcome(
                event_time_new, censoring_time_new, np.shape(X_new)[0])
            y, status = np.log(time), (event == 0.).astype(np.uint8)
        jacobian = None if y is None else np.where(status == 0, -y, 0.)
        return self._predict_censored(
            coef, obs_prec, X_new, y, status, ll_const=jacobian,
            return_draws=return_draws, draws_per_pass=_draws_per_pass)

    def predict_survival(self, coef, obs_prec, X_new=None, times=None):
        """Posterior survival S(t | x) = 1 - Phi((log t - x~ . beta)
        sqrt(tau)) over the draws coef (P,) or (P, S) with obs_prec (S,): a
        dict with 'time' (T,), 'mean' and 'sd' (n, T), the mean and the
        population standard deviation over the draws.  X_new=None: the
        training rows; otherwise rows of the model's raw columns, centred
        with the training design's column means.  times: strictly positive
        and increasing (None: the distinct event times of the training
        rows); any t may be asked for, before the first and past the last
        observed time too."""
        if times is None:
            times = np.unique(self.time[self.event == 1.])
        times = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float64)
        if times.ndim != 1 or times.size == 0 \
                or not np.all(np.isfinite(times)) or (times <= 0).any() \
                or np.any(np.diff(times) <= 0):
            raise ValueError("times must be finite, strictly positive and "
                             "strictly increasing.")
        res = self._predict_censored(coef, obs_prec, X_new, None, None,
                                     points=np.log(times))
        return {'time': times, 'mean': res['surv_mean'],
                'sd': res['surv_sd']}

    @staticmethod
    def simulate_outcome(X, beta, noise_sd=1., censoring_frac=.5, seed=None):
        """(event_time, censoring_time) with log T = X beta + noise_sd N(0, 1)
        and independent log-normal censoring times of the same spread whose
        common location is chosen so that the expected censored fraction is
        censoring_frac; exactly one of a row's two times is finite."""
        from scipy.special import ndtr
        if not 0. <= censoring_frac < 1.:
            raise ValueError("censoring_frac must lie in [0, 1).")
        rng = np.random.default_rng(seed)
        eta = np.asarray(X.dot(beta), dtype=np.float64).ravel()
        log_t = eta + noise_sd * rng.standard_normal(len(eta))
        log_c = np.full(len(eta), np.inf)
        if censoring_frac > 0.:
            # P(C < T) = mean Phi((eta - q) / (sd sqrt 2)), decreasing in q
            lo, hi = eta.min() - 40. * noise_sd, eta.max() + 40. * noise_sd
            for _ in range(200):
                q = .5 * (lo + hi)
                frac = np.mean(ndtr((eta - q) / (noise_sd * math.sqrt(2.))))
                lo, hi = (q, hi) if frac > censoring_frac else (lo, q)
            log_c = .5 * (lo + hi) + noise_sd * rng.standard_normal(len(eta))
        censored = log_c < log_t
        return np.where(censored, np.inf, np.exp(log_t)), \
            np.where(censored, np.exp(log_c), np.inf)


class PoissonModel(_DeviceHamiltonian, _Predictive, _Model):
    """Incidence-rate regression: counts y_i with mean exposure_i exp(eta_i).
    The likelihood, its gradient and the Hessian-vector products run on the
    device through one bbx_poisson handle (csrc/poisson.hip); the coefficients
    are drawn by 'hmc' or 'nuts', as the Cox model's are.  With `strata` (one
    label per row, the rows in cpoisson_preprocess's order) the likelihood is
    the conditional Poisson likelihood: one nuisance baseline rate per
    stratum, conditioned on the stratum's total count, through one
    bbx_cpoisson handle (csrc/cpoisson.hip) on a design without an intercept
    column."""

    _handle_attr = '_poisson'
    _pred_family = _lib.PRED_POISSON

    def __init__(self, y, exposure, design, strata=None):
        """Counts must line up with the rows of the design and be
        non-negative integers (integer-valued floats are accepted); exposure
        (None: 1 for every row) must be strictly positive and finite.  With
        strata the rows must be stratum-major, the strata in the sorted order
        of their labels, and every stratum must hold a positive count."""
        n_row = design.shape[0]
        y, exposure = _count_outcome(y, exposure, n_row)
        self.y = y
        self.exposure = exposure
        self.log_exposure = np.log(exposure)
        self.design = design
        self.name = 'poisson'
        self.strata = None
        # one bbx_poisson (with strata: bbx_cpoisson) handle, made by the
        # first call that needs it
        self._ham_prefix = 'bbx_poisson_'
        if strata is not None:
            if design.intercept_added:
                raise ValueError("The conditional Poisson model takes a "
                                 "design without an intercept column.")
            labels, codes = _stratum_codes(strata, n_row)
            if np.any(codes[:-1] > codes[1:]):
                raise ValueError(
                    "The observations need to be sorted by stratum, the "
                    "strata in the increasing order of their labels.")
            n_strata = len(labels)
            stratum_ptr = np.zeros(n_strata + 1, dtype=np.int64)
            np.cumsum(np.bincount(codes, minlength=n_strata),
                      out=stratum_ptr[1:])
            total = np.bincount(codes, weights=y, minlength=n_strata)
            if n_strata == 0 or np.any(total <= 0):
                raise ValueError(
                    "Some strata have no positive count. They have to be "
                    "removed before using the PoissonModel class.")
            self.strata = np.asarray(strata)
            self.stratum_ptr = stratum_ptr
            self.stratum_total = total
            self._ham_prefix = 'bbx_cpoisson_'
        self._poisson = c_void_p()
        self._location_serial = 0

    @property
    def handle(self):
        if not self._poisson:
            if not getattr(self.design, 'use_hip', False):
                raise TypeError("the device likelihood needs a HipDesignMatrix")
            y = np.ascontiguousarray(self.y, dtype=np.float64)
            o = np.ascontiguousarray(self.log_exposure, dtype=np.float64)
            if self.strata is None:
                _lib.check(_lib.load().bbx_poisson_create(
                    self.design.handle, _ptr(y), _ptr(o),
                    byref(self._poisson)))
            else:
                sptr = np.ascontiguousarray(self.stratum_ptr, dtype=np.int64)
                _lib.check(_lib.load().bbx_cpoisson_create(
                    self.design.handle, _ptr(y), _ptr(o), len(sptr) - 1,
                    _ptr(sptr), byref(self._poisson)))
        return self._poisson

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        """sum y eta - mu and X~^T (y - mu), mu = exposure exp(eta) (the terms
        constant in beta are dropped); (-inf, None) where a mean overflows.
        With strata: sum y (a - L_s) and X~^T (y - N_s pi), a = eta +
        log(exposure), L_s = log sum_s exp(a), pi = exp(a - L_s); finite for
        every finite beta."""
        return self._device_loglik_and_gradient(beta, loglik_only)

    # the trajectory's f(q0) (hmc.py:95-97) is the model's own likelihood
    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        """v -> -X~^T (mu .* (X~ v)) at beta (with strata: v -> -X~^T (N_s pi
        .* (u - ubar_s)), u = X~ v, ubar_s = sum_s pi u).  The handle holds
        one location: an operator stops working once a later call has moved
        it."""
        return self._hessian_operator(beta)

    def calc_intercept_mle(self):
        return np.log(self.y.sum() / self.exposure.sum())

    def predict(self, coef, X_new=None, y_new=None, exposure_new=None,
                return_draws=False, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is.  X_new=None: the training rows with the model's
        own counts and exposure; otherwise n_new rows of the model's raw
        columns (NumPy or SciPy), centred with the TRAINING design's column
        means, with exposure_new (None: 1) and with y_new or without.  A
        dict: 'mean' and 'sd' (n,), the posterior mean of the expected count
        exposure * rate and its population standard deviation over the
        draws; with an outcome 'lpd' (the log pointwise predictive density
        of every row), 'loglik_mean' and 'loglik_var' (n,) and the floats
        'lppd' = sum lpd, 'p_waic' = sum loglik_var and 'waic' =
        -2 (lppd - p_waic), the log density being the Poisson's with its
        -log y!; with return_draws 'draws' (n, S).  One device call for all
        the draws.  The conditional Poisson model (strata) refuses: its
        baseline rates are conditioned away."""
        if self.strata is not None:
            raise ValueError(
                "The conditional Poisson model has nothing to predict: the "
                "baseline rates of its strata are conditioned away.")
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new, exposure_new=exposure_new)
        y = ll_const = None
        if X_new is None:
            y, offset = self.y, self.log_exposure
        else:
            y, exposure = _count_outcome(
                np.zeros(n_row) if y_new is None else y_new, exposure_new,
                n_row)
            y = None if y_new is None else y
            offset = None if exposure_new is None else np.log(exposure)
        if y is not None:
            ll_const = -_log_factorial(y)
        return self._predictive_summary(
            draws, X_new, n_row, y=y, offset=offset, ll_const=ll_const,
            return_draws=return_draws, draws_per_pass=_draws_per_pass)

    @staticmethod
    def simulate_outcome(X, beta, exposure=None, seed=None):
        rate = np.exp(np.asarray(X.dot(beta), dtype=np.float64).ravel())
        if exposure is not None:
            rate = rate * np.asarray(exposure, dtype=np.float64)
        if seed is not None:
            np.random.seed(seed)
        return np.random.poisson(rate)


def _positive_scalar(x, what):
    """x as a float: a finite, positive number; `what`: 'dispersion'."""
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise ValueError("The %s must be a number." % what) from None
    if not (math.isfinite(x) and x > 0.):
        raise ValueError("The %s must be finite and positive." % what)
    return x


def _positive_draws(x, n_draw, what):
    """x, a scalar or one value per draw, as n_draw finite, positive numbers."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 0:
        x = np.full(n_draw, float(x))
    if x.shape != (n_draw,):
        raise ValueError(
            "%s must be a scalar or hold one value per draw: "
            "%s, %d draws." % (what, x.shape, n_draw))
    if not np.all(np.isfinite(x)) or (x <= 0).any():
        raise ValueError(
            "Every %s must be strictly positive and finite." % what)
    return np.ascontiguousarray(x)


def _candidate_loglik(model, entry, coef, cand, single):
    """The C ABI's candidate sums (`entry`: bbx_negbin_dispersion_loglik and
    its siblings) at the coefficients coef, or None for the linear predictor
    of the previous call, for the 1 to 8 candidates that the caller has
    checked: a float where `single`, else an array, one sum per candidate."""
    if coef is not None:
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.shape != (model.n_pred,):
            raise ValueError("coef must have length %d" % model.n_pred)
    out = np.empty(len(cand))
    _lib.check(getattr(_lib.load(), entry)(
        model.handle, _ptr(coef), len(cand), _ptr(cand), _ptr(out)))
    return float(out[0]) if single else out


def _scalar_candidates(x, name):
    """(1 to 8 values as an array, whether x was a scalar)"""
    single = np.ndim(x) == 0
    x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
    if x.ndim != 1 or not 1 <= x.size <= 8:
        raise ValueError("%s must be a scalar or hold 1 to 8 values." % name)
    return x, single


class NegBinModel(_DeviceHamiltonian, _Predictive, _Model):
    """Negative-binomial regression: counts y_i with mean mu_i = exposure_i
    exp(eta_i) and variance mu_i + mu_i^2 / r.  The dispersion r > 0 is a
    "size": r -> inf is the Poisson model.  The likelihood, its gradient and
    the Hessian-vector products run on the device through one bbx_negbin
    handle (csrc/negbin.hip); the coefficients are drawn by 'hmc' or 'nuts',
    as the Poisson model's are, and the dispersion by a slice update on log r
    (dispersion.py) right after them, unless it is given and held fixed.

    With t = eta + log(exposure) - log r the log density of a row is
    G(y, r) - log y! + y t - (y + r) softplus(t), G(y, r) = lgamma(y + r) -
    lgamma(r).  compute_loglik_and_gradient and the samplers see the part
    that depends on the coefficients, y t - (y + r) softplus(t): G - log y! is
    constant in them and is left out, as the Poisson model leaves out its
    constant.  dispersion_loglik adds G; predict scores with the full
    density."""

    _handle_attr = '_negbin'

    def __init__(self, y, exposure, design, dispersion=None,
                 dispersion_prior=None):
        """The outcome checks of the Poisson model.  dispersion: None -- the
        dispersion is a parameter of the chain, with the prior
        dispersion_prior = {'shape': a0, 'rate': b0} (None: Gamma(2, 0.1),
        whose shape keeps mass off r = 0), and starts at 1 -- or a finite,
        positive number that is held fixed."""
        from .dispersion import check_prior
        n_row = design.shape[0]
        y, exposure = _count_outcome(y, exposure, n_row)
        self.y = y
        self.exposure = exposure
        self.log_exposure = np.log(exposure)
        self.design = design
        self.name = 'negbin'
        self.dispersion_fixed = dispersion is not None
        if dispersion is None:
            dispersion = 1.
        elif dispersion_prior is not None:
            raise ValueError("dispersion_prior is the prior of a sampled "
                             "dispersion: dispersion is given and held fixed.")
        self._dispersion = _positive_scalar(dispersion, 'dispersion')
        self.dispersion_prior = check_prior(dispersion_prior)
        # one bbx_negbin handle, made by the first call that needs it
        self._ham_prefix = 'bbx_negbin_'
        self._negbin = c_void_p()
        self._location_serial = 0

    @property
    def handle(self):
        if not self._negbin:
            if not getattr(self.design, 'use_hip', False):
                raise TypeError("the device likelihood needs a HipDesignMatrix")
            y = np.ascontiguousarray(self.y, dtype=np.float64)
            o = np.ascontiguousarray(self.log_exposure, dtype=np.float64)
            _lib.check(_lib.load().bbx_negbin_create(
                self.design.handle, _ptr(y), _ptr(o), self._dispersion,
                byref(self._negbin)))
        return self._negbin

    @property
    def dispersion(self):
        return self._dispersion

    @dispersion.setter
    def dispersion(self, r):
        """bbx_negbin_set_dispersion: a Hessian operator made before it stops
        working, as after a move of its location."""
        r = _positive_scalar(r, 'dispersion')
        if self._negbin:
            _lib.check(_lib.load().bbx_negbin_set_dispersion(self._negbin, r))
            self._location_serial += 1
        self._dispersion = r

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        """sum y t - (y + r) softplus(t) and X~^T (y - (y + r) sigma(t)), t =
        eta + log(exposure) - log r, at the model's dispersion.  The terms
        constant in beta (sum G(y, r) - log y!) are dropped.  Finite for
        every finite beta: there is no exp(eta) to overflow; (-inf, None)
        where an infinite eta makes the likelihood -inf."""
        return self._device_loglik_and_gradient(beta, loglik_only)

    # the trajectory's f(q0) (hmc.py:95-97) is the model's own likelihood
    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        """v -> -X~^T (omega .* (X~ v)) at beta and the model's dispersion,
        omega = (y + r) sigma(t) (1 - sigma(t)).  The handle holds one
        location: an operator stops working once a later call has moved it or
        the dispersion has changed."""
        return self._hessian_operator(beta)

    def calc_intercept_mle(self):
        return np.log(self.y.sum() / self.exposure.sum())

    def dispersion_loglik(self, coef, r):
        """L(r) = sum_i G(y_i, r) + y_i t_i - (y_i + r) softplus(t_i) at the
        coefficients coef, for r a scalar or up to 8 values, in one pass over
        the rows (bbx_negbin_dispersion_loglik); a float or an array like r.
        coef=None reuses the linear predictor of the previous call.  The
        value for a given r depends neither on how many values are asked for
        nor on its place among them.  The model's own dispersion is not
        touched."""
        return _candidate_loglik(self, 'bbx_negbin_dispersion_loglik', coef,
                                 *_scalar_candidates(r, 'r'))

    def _pred_call(self, n_draw, draws, dispersion, offset, y, n_trial,
                   ll_const):
        return 'bbx_design_predictive_summary_negbin', (n_draw,), \
            (draws, dispersion, offset, y, ll_const)

    def predict(self, coef, dispersion, X_new=None, y_new=None,
                exposure_new=None, return_draws=False, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is -- with dispersion a scalar or one value per draw
        -- samples['dispersion'].  The arguments and the dict are those of
        PoissonModel.predict: 'mean' and 'sd' of the expected count exposure *
        rate over the draws and, with an outcome, 'lpd', 'loglik_mean',
        'loglik_var', 'lppd', 'p_waic' and 'waic' under the negative-binomial
        log density with all its terms, G(y, r) - log y! included, so that a
        WAIC compares with the Poisson model's.  One device call for all the
        draws."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new, exposure_new=exposure_new)
        r = _positive_draws(dispersion, len(draws), 'dispersion')
        y = ll_const = None
        if X_new is None:
            y, offset = self.y, self.log_exposure
        else:
            y, exposure = _count_outcome(
                np.zeros(n_row) if y_new is None else y_new, exposure_new,
                n_row)
            y = None if y_new is None else y
            offset = None if exposure_new is None else np.log(exposure)
        if y is not None:
            ll_const = -_log_factorial(y)
        return self._predictive_summary(
            draws, X_new, n_row, y=y, obs_prec=r, offset=offset,
            ll_const=ll_const, return_draws=return_draws,
            draws_per_pass=_draws_per_pass)

    @staticmethod
    def simulate_outcome(X, beta, dispersion, exposure=None, seed=None):
        """Counts with mean mu = exposure exp(X beta) and variance mu + mu^2 /
        dispersion: a Poisson count whose rate is mu times a Gamma(dispersion,
        1 / dispersion) factor."""
        mu = np.exp(np.asarray(X.dot(beta), dtype=np.float64).ravel())
        if exposure is not None:
            mu = mu * np.asarray(exposure, dtype=np.float64)
        if seed is not None:
            np.random.seed(seed)
        r = float(dispersion)
        return np.random.poisson(mu * np.random.gamma(r, 1. / r, mu.shape))


def _survival_outcome(event_time, censoring_time, n_row):
    """The outcome checks of the Weibull model on n_row rows: (event
    indicator d, time t = min of the two), the Cox model's convention --
    exactly one of a row's two times is finite."""
    et = np.asarray(event_time, dtype=np.float64)
    ct = np.asarray(censoring_time, dtype=np.float64)
    if not (et.shape == ct.shape == (n_row,)):
        raise ValueError(
            "Outcome vectors and design matrix have incompatible sizes: "
            "%s event times, %s censoring times, %d rows."
            % (et.shape, ct.shape, n_row))
    if np.any(np.isnan(et)) or np.any(np.isnan(ct)) \
            or np.any(np.isfinite(et) == np.isfinite(ct)):
        raise ValueError(
            "Exactly one of event_time and censoring_time must be finite in "
            "every row (inf marks the one that was not observed).")
    t = np.minimum(et, ct)
    if (t <= 0).any():
        raise ValueError("Every time must be strictly positive.")
    return np.isfinite(et).astype(np.float64), t


class WeibullModel(_DeviceHamiltonian, _Predictive, _Model):
    """Weibull proportional-hazards regression of right-censored times: the
    hazard of row i is h(t | x_i) = k t^(k - 1) exp(eta_i), eta = X~ beta with
    an intercept (the log rate is identifiable), so the coefficients are log
    hazard ratios and compare directly with a Cox fit of the same data; the
    shape k > 0 is a parameter of the chain, and k = 1 is the exponential
    model.  The likelihood, its gradient and the Hessian-vector products run
    on the device through one bbx_weibull handle (csrc/weibull.hip); the
    coefficients are drawn by 'hmc' or 'nuts' and the shape by a slice update
    on log k (weibull_shape.py) right after them, unless it is given and held
    fixed.

    With t = min(event_time, censoring_time), d = 1 for an event and lt =
    log t the log density of a row is d (log k + (k - 1) lt + eta) -
    exp(eta + k lt).  compute_loglik_and_gradient and the samplers see the
    part that depends on the coefficients, d eta - exp(eta + k lt);
    shape_loglik and predict use the whole density.

    R's survreg fits the same model in the accelerated-failure-time
    parametrisation: beta_aft = -beta_ph / k and scale = 1 / k.  Agreement
    with survreg is not tested."""

    _handle_attr = '_weibull'

    def __init__(self, event_time, censoring_time, design, shape=None,
                 shape_prior=None):
        """The times of the Cox model: exactly one of a row's event_time and
        censoring_time is finite, and it is strictly positive.  shape: None --
        the shape is a parameter of the chain, with the prior shape_prior =
        {'shape': a0, 'rate': b0} on k (None: Gamma(2, 1)), and starts at 1
        -- or a finite, positive number that is held fixed."""
        from .weibull_shape import check_prior
        n_row = design.shape[0]
        event, time = _survival_outcome(event_time, censoring_time, n_row)
        self.event = event
        self.time = time
        self.log_time = np.log(time)
        self.event_time = np.asarray(event_time, dtype=np.float64)
        self.censoring_time = np.asarray(censoring_time, dtype=np.float64)
        self.design = design
        self.name = 'weibull'
        self.shape_fixed = shape is not None
        if shape is None:
            shape = 1.
        elif shape_prior is not None:
            raise ValueError("shape_prior is the prior of a sampled shape: "
                             "shape is given and held fixed.")
        self._shape = _positive_scalar(shape, 'shape')
        self.shape_prior = check_prior(shape_prior)
        # one bbx_weibull handle, made by the first call that needs it
        self._ham_prefix = 'bbx_weibull_'
        self._weibull = c_void_p()
        self._location_serial = 0

    @property
    def handle(self):
        if not self._weibull:
            if not getattr(self.design, 'use_hip', False):
                raise TypeError("the device likelihood needs a HipDesignMatrix")
            d = np.ascontiguousarray(self.event, dtype=np.float64)
            lt = np.ascontiguousarray(self.log_time, dtype=np.float64)
            _lib.check(_lib.load().bbx_weibull_create(
                self.design.handle, _ptr(d), _ptr(lt), self._shape,
                byref(self._weibull)))
        return self._weibull

    @property
    def shape(self):
        return self._shape

    @shape.setter
    def shape(self, k):
        """bbx_weibull_set_shape: a Hessian operator made before it stops
        working, as after a move of its location."""
        k = _positive_scalar(k, 'shape')
        if self._weibull:
            _lib.check(_lib.load().bbx_weibull_set_shape(self._weibull, k))
            self._location_serial += 1
        self._shape = k

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        """sum d eta - m and X~^T (d - m), m = exp(eta + k log t), at the
        model's shape.  The terms constant in beta (sum d (log k + (k - 1)
        log t)) are dropped; (-inf, None) where an m overflows."""
        return self._device_loglik_and_gradient(beta, loglik_only)

    # the trajectory's f(q0) (hmc.py:95-97) is the model's own likelihood
    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        """v -> -X~^T (m .* (X~ v)) at beta and the model's shape.  The handle
        holds one location: an operator stops working once a later call has
        moved it or the shape has changed."""
        return self._hessian_operator(beta)

    def calc_intercept_mle(self):
        """log(sum d / sum t^k) at the model's current shape."""
        return math.log(self.event.sum() / np.sum(self.time ** self._shape))

    def shape_loglik(self, coef, k):
        """L(k) = sum_i d_i (log k + (k - 1) log t_i + eta_i) - exp(eta_i + k
        log t_i) at the coefficients coef, for k a scalar or up to 8 values,
        in one pass over the rows (bbx_weibull_shape_loglik); a float or an
        array like k.  coef=None reuses the linear predictor of the previous
        call.  The value for a given k depends neither on how many values are
        asked for nor on its place among them.  The model's own shape is not
        touched."""
        return _candidate_loglik(self, 'bbx_weibull_shape_loglik', coef,
                                 *_scalar_candidates(k, 'k'))

    def _pred_call(self, n_draw, draws, shape, offset, y, n_trial, ll_const):
        # (y is the event indicator and n_trial's place holds log t)
        return 'bbx_design_predictive_summary_weibull', (n_draw,), \
            (draws, shape, y, n_trial, ll_const)

    def predict(self, coef, shape, X_new=None, event_time_new=None,
                censoring_time_new=None, return_draws=False,
                _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is -- with shape a scalar or one value per draw --
        samples['weibull_shape'].  X_new=None: the training rows with the
        model's own times; otherwise n_new rows of the model's raw columns
        (NumPy or SciPy), centred with the TRAINING design's column means,
        with event_time_new and censoring_time_new (both, under the model's
        convention) or without.  A dict: 'mean' and 'sd' (n,), the posterior
        mean of the median survival time exp((log(log 2) - eta) / k) and its
        population standard deviation over the draws; with an outcome 'lpd',
        'loglik_mean' and 'loglik_var' (n,) and the floats 'lppd', 'p_waic'
        and 'waic' = -2 (lppd - p_waic) under the whole log density d (log k
        + (k - 1) log t + eta) - exp(eta + k log t); with return_draws 'draws'
        (n, S).  One device call for all the draws."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, event_time_new=event_time_new,
                            censoring_time_new=censoring_time_new)
        k = _positive_draws(shape, len(draws), 'shape')
        event = log_time = None
        if X_new is None:
            event, log_time = self.event, self.log_time
        elif event_time_new is not None or censoring_time_new is not None:
            if event_time_new is None or censoring_time_new is None:
                raise ValueError(
                    "event_time_new and censoring_time_new are given "
                    "together or not at all.")
            event, time = _survival_outcome(event_time_new,
                                            censoring_time_new, n_row)
            log_time = np.log(time)
        return self._predictive_summary(
            draws, X_new, n_row, y=event, obs_prec=k, n_trial=log_time,
            return_draws=return_draws, draws_per_pass=_draws_per_pass)

    def predict_survival(self, coef, shape, X_new=None, times=None,
                         return_draws=False):
        """Posterior survival S(t | x) = exp(-exp(k log t + x~ . beta)) over
        the draws coef (P,) or (P, S) with shape a scalar or one value per
        draw: a dict with 'time' (T,), 'mean' and 'sd' (n, T) -- the mean and
        the population standard deviation over the draws -- and, with
        return_draws, 'draws' (n, T, S).  X_new=None: the training rows;
        otherwise rows of the model's raw columns, centred with the training
        design's column means.  times: strictly positive and increasing
        (None: the distinct event times of the training rows).  The summary
        is bbx_cox_survival_summary with one group, whose log cumulative
        baseline hazard of draw s at time t is k_s log t: a parametric
        baseline, so any t may be asked for."""
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        n_draw = len(draws)
        k = _positive_draws(shape, n_draw, 'shape')
        if times is None:
            times = np.unique(self.time[self.event == 1.])
        times = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float64)
        if times.ndim != 1 or times.size == 0 \
                or not np.all(np.isfinite(times)) or (times <= 0).any() \
                or np.any(np.diff(times) <= 0):
            raise ValueError("times must be finite, strictly positive and "
                             "strictly increasing.")
        # every check is done: the device from here on
        design = self.design if X_new is None else _new_design(
            self.design, X_new, bool(self.intercept_added))
        if not getattr(design, 'use_hip', False):
            raise TypeError("prediction needs a HipDesignMatrix")
        eta = np.ascontiguousarray(np.stack([design.dot(b) for b in draws]))
        log_hazard = np.ascontiguousarray(k[:, None] * np.log(times)[None, :])
        n_time = len(times)
        mean, sd = np.empty((n_row, n_time)), np.empty((n_row, n_time))
        out = np.empty((n_row, n_time, n_draw)) if return_draws else None
        _lib.check(_lib.load().bbx_cox_survival_summary(
            design.device, n_row, n_time, n_draw, 1, _ptr(eta),
            _ptr(log_hazard), None, _ptr(mean), _ptr(sd), _ptr(out)))
        res = {'time': times, 'mean': mean, 'sd': sd}
        if return_draws:
            res['draws'] = out
        return res

    @staticmethod
    def _simulate_from_eta(eta, shape, censoring_frac, seed):
        """Event times with the cumulative hazard t^k exp(eta) -- t = (E /
        exp(eta))^(1 / k), E standard exponential, so that the median of row
        i is (log 2 / exp(eta_i))^(1 / k) -- and independent Weibull
        censoring times of the same shape whose common rate is chosen so that
        the expected censored fraction is censoring_frac."""
        if not 0. <= censoring_frac < 1.:
            raise ValueError("censoring_frac must lie in [0, 1).")
        if seed is not None:
            np.random.seed(seed)
        k = _positive_scalar(shape, 'shape')
        rate = np.exp(np.asarray(eta, dtype=np.float64))
        event_time = (np.random.exponential(size=rate.shape) / rate) \
            ** (1. / k)
        censoring_time = np.full(rate.shape, np.inf)
        if censoring_frac > 0.:
            # with t^k ~ Exp(rate_i) and c^k ~ Exp(nu): P(censored) =
            # mean of nu / (nu + rate_i), increasing in nu: bisection on log nu
            lo, hi = -80., 80.
            for _ in range(200):
                mid = .5 * (lo + hi)
                nu = math.exp(mid)
                if np.mean(nu / (nu + rate)) < censoring_frac:
                    lo = mid
                else:
                    hi = mid
            nu = math.exp(.5 * (lo + hi))
            censoring_time = (np.random.exponential(size=rate.shape) / nu) \
                ** (1. / k)
        censored = censoring_time < event_time
        event_time = np.where(censored, np.inf, event_time)
        censoring_time = np.where(censored, censoring_time, np.inf)
        return event_time, censoring_time

    @staticmethod
    def simulate_outcome(X, beta, shape, censoring_frac=.5, seed=None):
        """(event_time, censoring_time) under the hazard shape t^(shape - 1)
        exp(X beta), about censoring_frac of the rows censored; exactly one
        of a row's two times is finite."""
        eta = np.asarray(X.dot(beta), dtype=np.float64).ravel()
        return WeibullModel._simulate_from_eta(eta, shape, censoring_frac,
                                               seed)


def _ordinal_outcome(y, offset, n_row, n_category=None):
    """The outcome checks of the ordinal model on n_row rows: (y, offset,
    K).  n_category=None: K = max y + 1 and every category must hold a row;
    otherwise the categories of new rows, 0 ... n_category - 1."""
    y = np.asarray(y, dtype=np.float64)
    offset = np.zeros(y.shape) if offset is None \
        else np.asarray(offset, dtype=np.float64)
    if not (y.shape == offset.shape == (n_row,)):
        raise ValueError(
            "Outcome vectors and design matrix have incompatible sizes: "
            "%s categories, %s offsets, %d rows."
            % (y.shape, offset.shape, n_row))
    if not np.all(np.isfinite(y)) or (y < 0).any() \
            or (y != np.floor(y)).any():
        raise ValueError("Every category must be a non-negative integer.")
    if not np.all(np.isfinite(offset)):
        raise ValueError("Every offset must be finite.")
    top = int(y.max()) + 1 if y.size else 0
    if n_category is None:
        if not 2 <= top <= OrdinalModel.MAX_CATEGORY:
            raise ValueError(
                "The ordinal model takes 2 to %d categories, 0 ... K - 1: "
                "the outcome's largest is %d."
                % (OrdinalModel.MAX_CATEGORY, top - 1))
        counts = np.bincount(y.astype(np.intp), minlength=top)
        if (counts == 0).any():
            raise ValueError(
                "Category %d of 0 ... %d has no row: recode the outcome to "
                "consecutive categories." % (int(np.argmin(counts > 0)),
                                             top - 1))
        n_category = top
    elif top > n_category:
        raise ValueError("The model has the categories 0 ... %d: the "
                         "outcome holds %d." % (n_category - 1, top - 1))
    return y, offset, n_category


class OrdinalModel(_DeviceHamiltonian, _Predictive, _Model):
    """Proportional-odds (cumulative logit) regression of an ordered outcome:
    categories y_i in {0, ..., K - 1}, 2 <= K <= 16, with P(y_i <= k) =
    sigma(c_{k+1} - (eta_i + o_i)) for cutpoints c_1 < ... < c_{K-1} and an
    optional per-row offset o.  The design has no intercept column: the
    cutpoints are the intercepts (centring the predictors only shifts them).
    The likelihood, its gradient and the Hessian-vector products run on the
    device through one bbx_ordinal handle (csrc/ordinal.hip); the
    coefficients are drawn by 'hmc' or 'nuts' and the cutpoints by one slice
    update each (cutpoints.py) right after them, unless they are given and
    held fixed.

    With a = c_{y+1} - (eta + o) and b = c_y - (eta + o) the log-probability
    of a row is g_y - softplus(-a) - softplus(b), g_k = log(1 - exp(-(c_{k+1}
    - c_k))) for the inner categories and 0 for the two end ones (where the
    softplus term of the infinite cutpoint is absent): every term is kept, g
    depends on the cutpoints."""

    _handle_attr = '_ordinal'
    MAX_CATEGORY = 16

    def __init__(self, y, design, offset=None, cutpoints=None,
                 cutpoint_prior=None):
        """y: integers 0 ... K - 1, every category with at least one row;
        offset (None: 0) finite.  cutpoints: None -- they are parameters of
        the chain, with the prior cutpoint_prior = {'sd': s} (None: 10), c_k ~
        N(0, s^2) on the ordered cone, and start at the empirical logits of
        the cumulative proportions -- or K - 1 finite, strictly increasing
        numbers that are held fixed."""
        from .cutpoints import (check_cutpoints, check_prior,
                                initial_cutpoints)
        if design.intercept_added:
            raise ValueError("The ordinal model takes a design without an "
                             "intercept column: the cutpoints are the "
                             "intercepts.")
        y, offset, K = _ordinal_outcome(y, offset, design.shape[0])
        self.y = y
        self.offset = offset
        self.n_category = K
        self.design = design
        self.name = 'ordinal'
        self.cutpoints_fixed = cutpoints is not None
        if cutpoints is None:
            cutpoints = initial_cutpoints(y, K)
        elif cutpoint_prior is not None:
            raise ValueError("cutpoint_prior is the prior of sampled "
                             "cutpoints: cutpoints are given and held fixed.")
        self._cutpoints = check_cutpoints(cutpoints, K)
        self.cutpoint_prior = check_prior(cutpoint_prior)
        # one bbx_ordinal handle, made by the first call that needs it
        self._ham_prefix = 'bbx_ordinal_'
        self._ordinal = c_void_p()
        self._location_serial = 0

    @property
    def handle(self):
        if not self._ordinal:
            if not getattr(self.design, 'use_hip', False):
                raise TypeError("the device likelihood needs a HipDesignMatrix")
            y = np.ascontiguousarray(self.y, dtype=np.float64)
            o = np.ascontiguousarray(self.offset, dtype=np.float64) \
                if self.offset.any() else None
            _lib.check(_lib.load().bbx_ordinal_create(
                self.design.handle, _ptr(y), _ptr(o), self.n_category,
                _ptr(self._cutpoints), byref(self._ordinal)))
        return self._ordinal

    @property
    def cutpoints(self):
        return self._cutpoints.copy()

    @cutpoints.setter
    def cutpoints(self, cuts):
        self.set_cutpoints(cuts)

    def set_cutpoints(self, cuts):
        """bbx_ordinal_set_cutpoints: a Hessian operator made before it stops
        working, as after a move of its location."""
        from .cutpoints import check_cutpoints
        cuts = check_cutpoints(cuts, self.n_category)
        if self._ordinal:
            _lib.check(_lib.load().bbx_ordinal_set_cutpoints(
                self._ordinal, _ptr(cuts)))
            self._location_serial += 1
        self._cutpoints = cuts

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        """sum g_y - softplus(-a) - softplus(b) and X~^T (sigma(b) -
        sigma(-a)) at the model's cutpoints: the whole log-probability.
        Finite for every finite beta; (-inf, None) where an infinite eta
        gives a row's category the probability 0."""
        return self._device_loglik_and_gradient(beta, loglik_only)

    # the trajectory's f(q0) (hmc.py:95-97) is the model's own likelihood
    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    def get_hessian_matvec_operator(self, beta):
        """v -> -X~^T (d .* (X~ v)) at beta and the model's cutpoints, d =
        sigma(a) sigma(-a) + sigma(b) sigma(-b).  The handle holds one
        location: an operator stops working once a later call has moved it or
        the cutpoints have changed."""
        return self._hessian_operator(beta)

    def cutpoint_loglik(self, coef, cuts):
        """L(c) = sum_i ll_i at the coefficients coef, for one cutpoint
        vector (K - 1,) or up to 8 of them (n_c, K - 1), in one pass over the
        rows (bbx_ordinal_cutpoint_loglik); a float or an array (n_c,).
        coef=None reuses the linear predictor of the previous call.  The
        value of a given vector depends neither on how many are asked for nor
        on its place among them.  The model's own cutpoints are not
        touched."""
        cuts = np.ascontiguousarray(cuts, dtype=np.float64)
        single = cuts.ndim == 1
        if single:
            cuts = cuts[None, :]
        if cuts.ndim != 2 or cuts.shape[1] != self.n_category - 1 \
                or not 1 <= cuts.shape[0] <= 8:
            raise ValueError("cuts must hold 1 to 8 vectors of %d cutpoints: "
                             "shape %s." % (self.n_category - 1, cuts.shape))
        return _candidate_loglik(self, 'bbx_ordinal_cutpoint_loglik', coef,
                                 cuts, single)

    def calc_intercept_mle(self):
        raise ValueError("The ordinal model has no intercept: the cutpoints "
                         "are the intercepts.")

    def predict(self, coef, cutpoints, X_new=None, y_new=None,
                offset_new=None, _draws_per_pass=0):
        """Posterior prediction over the draws coef (P,) or (P, S) -- what
        samples['coef'] is -- with cutpoints (K - 1,) for every draw or
        (K - 1, S) -- samples['cutpoints'].  X_new=None: the training rows
        with the model's own outcome and offset; otherwise n_new rows of the
        model's raw columns (NumPy or SciPy), centred with the TRAINING
        design's column means, with offset_new (None: 0) and with y_new or
        without.  A dict: 'mean' and 'sd' (n, K), the posterior mean of every
        category's probability and its population standard deviation over the
        draws (the rows of 'mean' sum to 1); with an outcome 'lpd' (the log
        pointwise predictive density of every row), 'loglik_mean' and
        'loglik_var' (n,) and the floats 'lppd' = sum lpd, 'p_waic' = sum
        loglik_var and 'waic' = -2 (lppd - p_waic).  One device call for all
        the draws (bbx_design_predictive_summary_ordinal)."""
        from .cutpoints import check_cutpoints
        draws, X_new, n_row = self._predict_rows(coef, X_new)
        _training_rows_only(X_new, y_new=y_new, offset_new=offset_new)
        K, n_draw = self.n_category, len(draws)
        cuts = np.asarray(cutpoints, dtype=np.float64)
        if cuts.ndim == 1:
            cuts = np.repeat(cuts[:, None], n_draw, axis=1)
        if cuts.shape != (K - 1, n_draw):
            raise ValueError(
                "cutpoints must have shape (%d,) or (%d, n_draw): %s, %d "
                "draws." % (K - 1, K - 1, cuts.shape, n_draw))
        cuts = np.ascontiguousarray(cuts.T)
        for c in cuts:
            check_cutpoints(c, K)
        if X_new is None:
            y, offset = self.y, self.offset
        else:
            y, offset, _ = _ordinal_outcome(
                np.zeros(n_row) if y_new is None else y_new, offset_new,
                n_row, K)
            y = None if y_new is None else y
            offset = None if offset_new is None else offset
        # (the constructor refuses a design with an intercept column: the
        # shared tail's bool(self.intercept_added) is False here)
        return self._predictive_summary(
            draws, X_new, n_row, y=y, obs_prec=cuts, offset=offset,
            draws_per_pass=_draws_per_pass, n_plane=K)

    def _pred_call(self, n_draw, draws, cuts, offset, y, n_trial, ll_const):
        return 'bbx_design_predictive_summary_ordinal', \
            (n_draw, self.n_category), (draws, cuts, offset, y)

    @staticmethod
    def simulate_outcome(X, beta, cutpoints, offset=None, seed=None):
        """Categories 0 ... K - 1 with P(y <= k) = sigma(c_{k+1} - (X beta +
        offset)): the number of cutpoints below a logistic variate centred
        at X beta + offset."""
        eta = np.asarray(X.dot(beta), dtype=np.float64).ravel()
        if offset is not None:
            eta = eta + np.asarray(offset, dtype=np.float64)
        cuts = np.asarray(cutpoints, dtype=np.float64)
        if seed is not None:
            np.random.seed(seed)
        latent = eta + np.random.logistic(size=eta.shape)
        return np.searchsorted(cuts, latent, side='left')


def cox_sort_permutation(event_time, censoring_time):
    """The row order of cox_model.py:70-121 (None: already in order): events
    by increasing time, then censored rows by decreasing censoring time.  The
    reference ranks with np.argsort twice; argsort of those distinct ranks is
    the first argsort itself, so this is the same permutation, ties included."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    if event_time.shape != censoring_time.shape or event_time.ndim != 1:
        raise ValueError("event_time and censoring_time must be 1-d arrays of "
                         "the same length.")
    if not np.all(np.equal(event_time == float('inf'),
                           censoring_time < float('inf'))):
        raise ValueError("Either event or censoring time must be infinity for "
                         "each observation.")
    if np.all(event_time[:-1] <= event_time[1:]) \
            and np.all(censoring_time[:-1] >= censoring_time[1:]):
        return None
    n_event = int(np.sum(event_time < float('inf')))
    return np.concatenate((np.argsort(event_time)[:n_event],
                           np.argsort(censoring_time)[::-1][n_event:]))


def cox_preprocess(event_time, censoring_time, X=None):
    """CoxModel.preprocess_data (cox_model.py:57-142): sort, then drop the
    rows censored before the first event.  Returns (event_time,
    censoring_time, X, keep): keep[i] is the original index of row i."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    keep = np.arange(len(event_time))
    perm = cox_sort_permutation(event_time, censoring_time)
    if perm is not None:
        warn("The observations and design matrix will be sorted so that the "
             "event times are in the ascending order and censoring times in "
             "the descending order.")
        keep = keep[perm]
    event_time, censoring_time = event_time[keep], censoring_time[keep]
    informative = ~(censoring_time < np.min(event_time))
    if not np.all(informative):
        warn("Some observations do not contribute to the likelihood, so they "
             "are being removed.")
        keep = keep[informative]
        event_time = event_time[informative]
        censoring_time = censoring_time[informative]
    if X is not None and not np.array_equal(keep, np.arange(X.shape[0])):
        X = X.tocsr()[keep, :] if sparse.issparse(X) else X[keep, :]
    return event_time, censoring_time, X, keep


def cox_risk_sets(event_time, censoring_time):
    """Risk-set indices and appearance counts of sorted observations
    (cox_model.py:150-178) in O(n log n): start_k is the first event tied with
    event k, end_k = n - 1 - #(censored before t_k) (a tied censoring time is
    in the risk set), n_app[i] = #{k : start_k <= i <= end_k}."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    if np.any(event_time[:-1] > event_time[1:]):
        raise ValueError(
            "The observations need to be sorted so that the event times are "
            "in the increasing order, from the earliest to last events.")
    if np.any(censoring_time[:-1] < censoring_time[1:]):
        raise ValueError(
            "The observations need to be sorted so that the censoring times "
            "are in the decreasing order, from uncensored, last censored, to "
            "the earliest censored.")
    n = len(event_time)
    n_event = n - int(np.sum(np.isinf(event_time)))
    events = event_time[:n_event]
    start = np.searchsorted(events, events, side='left')
    censored_asc = np.flip(censoring_time[n_event:])
    end = n - 1 - np.searchsorted(censored_asc, events, side='left')
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, start, 1)
    np.add.at(diff, end + 1, -1)
    n_app = np.cumsum(diff[:n])
    if not np.all(n_app >= 1):
        raise ValueError(
            "Some individuals never appear in the risk set. They have to be "
            "removed before using the CoxModel class.")
    return n_event, start, end, n_app


def cox_tie_groups(event_time):
    """The tie group of every event of sorted observations: (gstart, gsize),
    gstart[k] the row of the first event tied with event k (cox_risk_sets'
    start_k) and gsize[k] = d the number of events that share its time.
    Event k is number l = k - gstart[k] of its group, and Efron's
    approximation leaves the fraction 1 - l/d of the group in its risk set."""
    event_time = np.asarray(event_time, dtype=np.float64)
    if np.any(event_time[:-1] > event_time[1:]):
        raise ValueError(
            "The observations need to be sorted so that the event times are "
            "in the increasing order, from the earliest to last events.")
    events = event_time[:len(event_time) - int(np.sum(np.isinf(event_time)))]
    gstart = np.searchsorted(events, events, side='left')
    gsize = np.searchsorted(events, events, side='right') - gstart
    return gstart, gsize


def _interval_times(entry_time, event_time, censoring_time):
    entry_time = np.asarray(entry_time, dtype=np.float64)
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    if not (entry_time.shape == event_time.shape == censoring_time.shape) \
            or event_time.ndim != 1:
        raise ValueError("entry_time, event_time and censoring_time must be "
                         "1-d arrays of the same length.")
    if not np.all(np.equal(event_time == float('inf'),
                           censoring_time < float('inf'))):
        raise ValueError("Either event or censoring time must be infinity for "
                         "each observation.")
    if np.any(np.isnan(entry_time)):
        raise ValueError("An entry time must not be NaN.")
    exit_time = np.minimum(event_time, censoring_time)
    if not np.all(entry_time < exit_time):
        raise ValueError("Every entry time must be strictly before the "
                         "observation's event or censoring time.")
    return entry_time, event_time, censoring_time, exit_time


def _n_risk_sets(entry_time, exit_time, event_time):
    """(p, q) of every row: the number of events at or before its exit time
    and at or before its entry time; the row is in p - q risk sets."""
    events = np.sort(event_time[np.isfinite(event_time)])
    return (np.searchsorted(events, exit_time, side='right'),
            np.searchsorted(events, entry_time, side='right'))


def cox_preprocess_interval(entry_time, event_time, censoring_time, X=None):
    """cox_preprocess for the counting-process form: row i is at risk on
    (entry_time[i], min(event_time[i], censoring_time[i])].  The rows are
    sorted by exit time ascending, events before censored rows at an equal
    exit (a stable sort: tied rows keep their relative order), then without
    the rows that are in no risk set.  Returns (entry_time, event_time,
    censoring_time, X, keep): keep[i] is the original index of row i."""
    entry_time, event_time, censoring_time, exit_time = _interval_times(
        entry_time, event_time, censoring_time)
    n = len(event_time)
    censored = event_time == float('inf')
    keep = np.lexsort((censored, exit_time))
    if not np.array_equal(keep, np.arange(n)):
        warn("The observations and design matrix will be sorted so that the "
             "event and censoring times are in the ascending order, events "
             "before the observations censored at the same time.")
    p, q = _n_risk_sets(entry_time[keep], exit_time[keep], event_time)
    informative = p > q
    if not np.all(informative):
        warn("Some observations do not contribute to the likelihood, so they "
             "are being removed.")
        keep = keep[informative]
    entry_time, event_time = entry_time[keep], event_time[keep]
    censoring_time = censoring_time[keep]
    if X is not None and not np.array_equal(keep, np.arange(X.shape[0])):
        X = X.tocsr()[keep, :] if sparse.issparse(X) else X[keep, :]
    return entry_time, event_time, censoring_time, X, keep


def cox_interval_risk_sets(entry_time, event_time, censoring_time):
    """The index arrays of the counting-process Cox handle, of rows already in
    cox_preprocess_interval's order, in O(n log n).  Returns (n_event, evrow,
    a, b, p, q, entry_perm): evrow[k] is the row of event k in time order;
    a[k] the first row whose exit time is >= t_k; entry_perm the rows in
    ascending entry order (stable) and b[k] the first position in it whose
    entry time is >= t_k (n if there is none), so that risk set k is the rows
    from a[k] on minus the rows entry_perm[b[k]:]; p[i] = #{k : t_k <= exit_i}
    and q[i] = #{k : t_k <= entry_i}."""
    entry_time, event_time, censoring_time, exit_time = _interval_times(
        entry_time, event_time, censoring_time)
    censored = event_time == float('inf')
    same = exit_time[:-1] == exit_time[1:]
    if np.any(exit_time[:-1] > exit_time[1:]) \
            or np.any(same & censored[:-1] & ~censored[1:]):
        raise ValueError(
            "The observations need to be sorted so that the event and "
            "censoring times are in the increasing order, events before the "
            "observations censored at the same time.")
    evrow = np.flatnonzero(~censored)
    n_event = len(evrow)
    events = event_time[evrow]
    p, q = _n_risk_sets(entry_time, exit_time, event_time)
    if not np.all(p > q):
        raise ValueError(
            "Some individuals never appear in the risk set. They have to be "
            "removed before using the CoxModel class.")
    a = np.searchsorted(exit_time, events, side='left')
    entry_perm = np.argsort(entry_time, kind='stable')
    b = np.searchsorted(entry_time[entry_perm], events, side='left')
    return n_event, evrow, a, b, p, q, entry_perm


def _finegray_times(event_time, censoring_time, competing_time):
    """(event, censoring, competing times as float64, the observed time T,
    the status: 0 event, 1 competing event, 2 censored)."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    competing_time = np.asarray(competing_time, dtype=np.float64)
    if not (event_time.shape == censoring_time.shape == competing_time.shape) \
            or event_time.ndim != 1:
        raise ValueError("event_time, censoring_time and competing_time must "
                         "be 1-d arrays of the same length.")
    times = np.stack((event_time, competing_time, censoring_time))
    if np.any(np.isnan(times)):
        raise ValueError("A time must not be NaN.")
    if not np.all(np.sum(times < float('inf'), axis=0) == 1) \
            or np.any(times == -float('inf')):
        raise ValueError("Exactly one of event, censoring and competing time "
                         "must be finite for each observation (the others "
                         "infinity).")
    return (event_time, censoring_time, competing_time, np.min(times, axis=0),
            np.argmin(times, axis=0))


def cox_finegray_censoring_survivor(event_time, censoring_time,
                                    competing_time):
    """G(T_i-) of every row: the Kaplan-Meier estimate of the censoring
    survivor function from the left, G(s-) = prod_{c < s} (1 - m_c / Y(c))
    over the distinct censoring times c, m_c rows censored at c and
    Y(c) = #{i : T_i >= c} rows of every status.  G(T_i-) > 0: row i is in
    Y(c) for every c <= T_i."""
    _, censoring_time, _, T, status = _finegray_times(
        event_time, censoring_time, competing_time)
    c, m = np.unique(T[status == 2], return_counts=True)
    Y = len(T) - np.searchsorted(np.sort(T), c, side='left')
    G = np.concatenate(([1.], np.cumprod(1. - m / Y)))
    return G[np.searchsorted(c, T, side='left')]


def cox_preprocess_finegray(event_time, censoring_time, competing_time,
                            X=None):
    """cox_preprocess for the Fine-Gray competing-risks model: every row has
    exactly one finite time out of event, censoring and competing time.  G is
    computed on all the rows as given (cox_finegray_censoring_survivor); the
    rows are then sorted by their time ascending, at an equal time events,
    then competing, then censored rows (a stable sort), and the rows censored
    before the first event are dropped (a competing row stays in every later
    risk set and is never dropped).  Returns (event_time, censoring_time,
    competing_time, X, keep, event_g, comp_rinv): keep[i] is the original
    index of row i, event_g[k] = G(t_k-) of the events in time order and
    comp_rinv[j] = 1 / G(T-) of the competing rows in row order."""
    event_time, censoring_time, competing_time, T, status = _finegray_times(
        event_time, censoring_time, competing_time)
    G = cox_finegray_censoring_survivor(event_time, censoring_time,
                                        competing_time)
    n = len(T)
    keep = np.lexsort((status, T))
    if not np.array_equal(keep, np.arange(n)):
        warn("The observations and design matrix will be sorted so that the "
             "event, competing and censoring times are in the ascending "
             "order, events before competing events before the observations "
             "censored at the same time.")
    first = np.min(event_time) if n else float('inf')
    informative = ~((status[keep] == 2) & (T[keep] < first))
    if not np.all(informative):
        warn("Some observations do not contribute to the likelihood, so they "
             "are being removed.")
        keep = keep[informative]
    event_time, censoring_time = event_time[keep], censoring_time[keep]
    competing_time = competing_time[keep]
    if X is not None and not np.array_equal(keep, np.arange(X.shape[0])):
        X = X.tocsr()[keep, :] if sparse.issparse(X) else X[keep, :]
    G, status = G[keep], status[keep]
    return (event_time, censoring_time, competing_time, X, keep,
            G[status == 0], 1. / G[status == 1])


def cox_finegray_risk_sets(event_time, censoring_time, competing_time):
    """The index arrays of the Fine-Gray handle, of rows already in
    cox_preprocess_finegray's order, in O(n log n).  Returns (n_event, evrow,
    a, b, p, comp_row): evrow[k] is the row of event k in time order; a[k] the
    first row whose time is >= t_k; comp_row the competing rows, ascending;
    b[k] the number of competing rows before row a[k], so that risk set k is
    the rows from a[k] on with weight 1 and the rows comp_row[:b[k]] with
    weight G(t_k-) / G(T-); p[i] = #{k : t_k <= T_i}."""
    event_time, censoring_time, competing_time, T, status = _finegray_times(
        event_time, censoring_time, competing_time)
    same = T[:-1] == T[1:]
    if np.any(T[:-1] > T[1:]) or np.any(same & (status[:-1] > status[1:])):
        raise ValueError(
            "The observations need to be sorted so that the event, competing "
            "and censoring times are in the increasing order, events before "
            "competing events before the observations censored at the same "
            "time.")
    evrow = np.flatnonzero(status == 0)
    comp_row = np.flatnonzero(status == 1)
    events = event_time[evrow]
    p = np.searchsorted(events, T, side='right')
    if np.any((p == 0) & (status == 2)):
        raise ValueError(
            "Some individuals never appear in the risk set. They have to be "
            "removed before using the CoxModel class.")
    a = np.searchsorted(T, events, side='left')
    b = np.searchsorted(comp_row, a, side='left')
    return len(evrow), evrow, a, b, p, comp_row


def _stratum_codes(strata, n):
    """(labels in np.unique order, the stratum number of every row)."""
    strata = np.asarray(strata)
    if strata.ndim != 1 or len(strata) != n:
        raise ValueError("strata must be a 1-d array with one label for each "
                         "observation.")
    labels, codes = np.unique(strata, return_inverse=True)
    return labels, np.asarray(codes, dtype=np.int64).ravel()


def cox_preprocess_stratified(event_time, censoring_time, strata, X=None):
    """cox_preprocess for a stratified model: the rows sorted stratum-major
    (strata in np.unique order of their labels; inside a stratum the events by
    increasing time, then the censored rows by decreasing censoring time; the
    sort is stable, so tied rows keep their relative order), then without the
    strata that have no event and without the rows censored before the first
    event of their stratum.  Returns (event_time, censoring_time, strata, X,
    keep): keep[i] is the original index of row i."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    if event_time.shape != censoring_time.shape or event_time.ndim != 1:
        raise ValueError("event_time and censoring_time must be 1-d arrays of "
                         "the same length.")
    if not np.all(np.equal(event_time == float('inf'),
                           censoring_time < float('inf'))):
        raise ValueError("Either event or censoring time must be infinity for "
                         "each observation.")
    n = len(event_time)
    strata = np.asarray(strata)
    labels, codes = _stratum_codes(strata, n)
    censored = event_time == float('inf')
    key = np.where(censored, -censoring_time, event_time)
    keep = np.lexsort((key, censored, codes))
    if not np.array_equal(keep, np.arange(n)):
        warn("The observations and design matrix will be sorted by stratum, "
             "and within each stratum so that the event times are in the "
             "ascending order and censoring times in the descending order.")
    event_time, censoring_time = event_time[keep], censoring_time[keep]
    strata, codes = strata[keep], codes[keep]
    first_event = np.full(len(labels), float('inf'))
    np.minimum.at(first_event, codes, event_time)
    has_event = np.isfinite(first_event)[codes]
    if not np.all(has_event):
        warn("Some strata have no event and do not contribute to the "
             "likelihood, so they are being removed.")
    informative = ~(censoring_time < first_event[codes])
    if not np.all(informative | ~has_event):
        warn("Some observations do not contribute to the likelihood, so they "
             "are being removed.")
    ok = has_event & informative
    if not np.all(ok):
        keep, strata = keep[ok], strata[ok]
        event_time, censoring_time = event_time[ok], censoring_time[ok]
    if X is not None and not np.array_equal(keep, np.arange(X.shape[0])):
        X = X.tocsr()[keep, :] if sparse.issparse(X) else X[keep, :]
    return event_time, censoring_time, strata, X, keep


def cpoisson_preprocess(y, exposure, strata, X=None):
    """The row order of the conditional Poisson model: the rows sorted
    stratum-major (strata in np.unique order of their labels; the sort is
    stable, so the rows of a stratum keep their relative order), then without
    the strata whose counts sum to 0 and without the strata of a single row
    -- both contribute a constant to the likelihood.  Returns (y, exposure,
    strata, X, keep): keep[i] is the original index of row i; exposure stays
    None if it was."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError("y must be a 1-d array.")
    n = len(y)
    if exposure is not None:
        exposure = np.asarray(exposure, dtype=np.float64)
        if exposure.shape != y.shape:
            raise ValueError("y and exposure must be 1-d arrays of the same "
                             "length.")
    strata = np.asarray(strata)
    labels, codes = _stratum_codes(strata, n)
    keep = np.argsort(codes, kind='stable')
    if not np.array_equal(keep, np.arange(n)):
        warn("The observations and design matrix will be sorted by stratum.")
    codes = codes[keep]
    total = np.bincount(codes, weights=y[keep], minlength=len(labels))
    size = np.bincount(codes, minlength=len(labels))
    has_count = (total > 0)[codes]
    if not np.all(has_count):
        warn("Some strata have no positive count and do not contribute to the "
             "likelihood, so they are being removed.")
    plural = (size > 1)[codes]
    if not np.all(plural | ~has_count):
        warn("Some strata have a single observation and do not contribute to "
             "the likelihood, so they are being removed.")
    keep = keep[has_count & plural]
    y, strata = y[keep], strata[keep]
    if exposure is not None:
        exposure = exposure[keep]
    if X is not None and not np.array_equal(keep, np.arange(X.shape[0])):
        X = X.tocsr()[keep, :] if sparse.issparse(X) else X[keep, :]
    return y, exposure, strata, X, keep


def cox_stratified_risk_sets(event_time, censoring_time, strata):
    """cox_risk_sets per stratum, in global indices, of rows already in
    cox_preprocess_stratified's order.  Returns (stratum_ptr, stratum_n_event,
    start, end, last_set): stratum s is rows stratum_ptr[s] ..
    stratum_ptr[s + 1] - 1; events are numbered in row order across strata;
    risk set k is rows start[k] .. end[k], inside the stratum of event k;
    last_set[i] is the number of the last event whose risk set holds row i."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    n = len(event_time)
    if event_time.shape != censoring_time.shape or event_time.ndim != 1:
        raise ValueError("event_time and censoring_time must be 1-d arrays of "
                         "the same length.")
    labels, codes = _stratum_codes(strata, n)
    if n == 0:
        raise ValueError("The Cox model needs at least one event.")
    if np.any(codes[:-1] > codes[1:]):
        raise ValueError(
            "The observations need to be sorted by stratum, the strata in the "
            "increasing order of their labels.")
    same = codes[:-1] == codes[1:]
    if np.any(same & (event_time[:-1] > event_time[1:])):
        raise ValueError(
            "The observations of each stratum need to be sorted so that the "
            "event times are in the increasing order, from the earliest to "
            "last events.")
    if np.any(same & (censoring_time[:-1] < censoring_time[1:])):
        raise ValueError(
            "The observations of each stratum need to be sorted so that the "
            "censoring times are in the decreasing order, from uncensored, "
            "last censored, to the earliest censored.")
    n_strata = len(labels)
    stratum_ptr = np.zeros(n_strata + 1, dtype=np.int64)
    np.cumsum(np.bincount(codes, minlength=n_strata), out=stratum_ptr[1:])
    is_event = np.isfinite(event_time)
    stratum_n_event = np.bincount(codes[is_event], minlength=n_strata)
    if np.any(stratum_n_event == 0):
        raise ValueError(
            "Some strata have no event. They have to be removed before using "
            "the CoxModel class.")
    event_ptr = np.zeros(n_strata + 1, dtype=np.int64)
    np.cumsum(stratum_n_event, out=event_ptr[1:])
    rows = np.flatnonzero(is_event)              # the row of every event
    ev_time, ev_code = event_time[rows], codes[rows]
    # start: the first event of the same stratum tied with event k
    head = np.ones(len(rows), dtype=bool)
    head[1:] = (ev_code[1:] != ev_code[:-1]) | (ev_time[1:] != ev_time[:-1])
    start = np.maximum.accumulate(np.where(head, rows, 0))
    # end: the stratum's last row minus its rows censored before t_k (a tied
    # censoring time is in the risk set): merge events and censored rows by
    # (stratum, time, events first) and count the censored rows ahead
    cens_rows = np.flatnonzero(~is_event)
    m_time = np.concatenate((ev_time, censoring_time[cens_rows]))
    m_code = np.concatenate((ev_code, codes[cens_rows]))
    m_cens = np.concatenate((np.zeros(len(rows), dtype=np.int64),
                             np.ones(len(cens_rows), dtype=np.int64)))
    order = np.lexsort((m_cens, m_time, m_code))
    ahead = np.empty(len(order), dtype=np.int64)
    ahead[order] = np.cumsum(m_cens[order])
    cens_ptr = stratum_ptr - event_ptr           # censored rows before stratum s
    end = (stratum_ptr[ev_code + 1] - 1
           - (ahead[:len(rows)] - cens_ptr[ev_code]))
    diff = np.zeros(n + 1, dtype=np.int64)
    np.add.at(diff, start, 1)
    np.add.at(diff, end + 1, -1)
    n_app = np.cumsum(diff[:n])
    if not np.all(n_app >= 1):
        raise ValueError(
            "Some individuals never appear in the risk set. They have to be "
            "removed before using the CoxModel class.")
    # the risk sets that hold row i are the first n_app[i] of its stratum
    last_set = event_ptr[codes] + n_app - 1
    return stratum_ptr, stratum_n_event, start, end, last_set


def _check_ties(ties, strata=None, entry_time=None):
    if ties not in ('breslow', 'efron'):
        raise ValueError("ties must be 'breslow' or 'efron', not %r." % (ties,))
    if ties == 'efron' and strata is not None and entry_time is None:
        raise ValueError(
            "ties='efron' together with strata is not supported: Efron's "
            "approximation in the stratified model is not built.")
    if ties == 'efron' and entry_time is not None and strata is None:
        raise ValueError(
            "ties='efron' together with entry_time is not supported: Efron's "
            "approximation in the counting-process model is not built.")


def _check_weights(weights, n, strata=None, entry_time=None, ties='breslow'):
    """The case weights of n rows as a float64 vector (None stays None)."""
    if weights is None:
        return None
    if strata is not None:
        raise ValueError(
            "weights together with strata is not supported: case weights in "
            "the stratified model are not built.")
    if entry_time is not None:
        raise ValueError(
            "weights together with entry_time is not supported: case weights "
            "in the counting-process model are not built.")
    if ties == 'efron':
        raise ValueError(
            "weights together with ties='efron' is not supported: case "
            "weights with Efron's approximation are not built.")
    weights = np.array(weights, dtype=np.float64)
    if weights.shape != (n,):
        raise ValueError(
            "weights must be a 1-d array with one weight for each "
            "observation: shape %s, %d observations." % (weights.shape, n))
    if not np.all(np.isfinite(weights)) or np.any(weights <= 0):
        raise ValueError(
            "Every weight must be strictly positive and finite (drop the "
            "rows of weight 0 instead).")
    return weights


def _check_competing(competing_time, strata=None, entry_time=None,
                     ties='breslow', weights=None):
    if competing_time is None:
        return
    if strata is not None:
        raise ValueError(
            "competing_time together with strata is not supported: the "
            "stratified Fine-Gray model is not built.")
    if entry_time is not None:
        raise ValueError(
            "competing_time together with entry_time is not supported: the "
            "Fine-Gray model with delayed entry is not built.")
    if ties == 'efron':
        raise ValueError(
            "competing_time together with ties='efron' is not supported: "
            "Efron's approximation in the Fine-Gray model is not built.")
    if weights is not None:
        raise ValueError(
            "competing_time together with weights is not supported: case "
            "weights in the Fine-Gray model are not built.")


def _cox_event_times(model):
    """The event times of a CoxModel as the handle numbers them: a list with
    one (number of the first event, event times ascending) per stratum (one
    entry without strata)."""
    t = model.event_time
    if getattr(model, 'strata', None) is not None:
        out, first = [], 0
        for s, ne in enumerate(model.stratum_n_event):
            r0 = int(model.stratum_ptr[s])
            out.append((first, t[r0:r0 + int(ne)]))
            first += int(ne)
        return out
    if hasattr(model, 'event_row'):       # counting-process and Fine-Gray rows
        return [(0, t[model.event_row])]
    return [(0, t[:model.n_event])]


def cox_hazard_grid(model, times=None):
    """The time grid of a baseline hazard and, for every grid point, the
    number of the last event at or before it (-1: none), as the handle numbers
    its events: (times, grid_event), grid_event int32 of shape (T,), or
    (n_strata, T) for a stratified model (every stratum indexed on its own,
    in global event numbers).  A grid point on an event time takes the last
    event tied there.  times=None: the model's distinct event times; a
    stratified model needs a grid.  Pure NumPy: no device call."""
    events = _cox_event_times(model)
    stratified = getattr(model, 'strata', None) is not None
    if times is None:
        if stratified:
            raise ValueError(
                "A stratified model has one set of event times per stratum: "
                "a grid of times is required.")
        times = np.unique(events[0][1])
    else:
        times = np.array(times, dtype=np.float64)
        if times.ndim != 1 or len(times) == 0:
            raise ValueError("times must be a non-empty 1-d array.")
        if not np.all(np.isfinite(times)):
            raise ValueError("Every grid time must be finite.")
        if np.any(times[:-1] > times[1:]):
            raise ValueError("The grid times must be in the ascending order.")
    grid = np.empty((len(events), len(times)), dtype=np.int32)
    for s, (first, t) in enumerate(events):
        k = np.searchsorted(t, times, side='right') - 1
        grid[s] = np.where(k >= 0, first + k, -1)
    return times, (grid if stratified else grid[0])


class CoxModel(_DeviceHamiltonian, _Model):
    """cox_model.py:7-303 on a HIP design whose rows are already in the
    model's order (RegressionModel(..., family='cox') sorts them).  The
    likelihood, its gradient and the Hessian-vector products run on the device
    through one bbx_cox handle.  With `strata` (one label per row, the rows in
    cox_preprocess_stratified's order) the likelihood is the stratified
    partial likelihood: one risk-set structure and one baseline hazard per
    stratum, shared coefficients.  With `entry_time` (one per row, -inf where
    a row is at risk from the start; the rows in cox_preprocess_interval's
    order) the likelihood is the counting-process form, through one bbx_coxcp
    handle (csrc/cox_interval.hip): row i is in the risk set of an event at t
    iff entry_time[i] < t <= its event or censoring time, which covers delayed
    entry and subjects written as several (start, stop] rows.  With
    ties='efron' (without strata and without entry_time) tied event times are
    handled by Efron's approximation instead of Breslow's rule, on the plain
    model's rows through one bbx_coxef handle (csrc/cox_efron.hip);
    `tie_group_size` then holds, for every event, the number of events that
    share its time.  With `weights` (one strictly positive weight per row, in
    row order; without strata, entry_time and ties='efron') the likelihood is
    the weighted partial likelihood, through one bbx_coxw handle
    (csrc/cox_weighted.hip): with integer weights it is the plain likelihood
    of the rows written that many times.  With `competing_time` (one per row,
    inf where the row had no competing event; exactly one of the three times
    of a row is finite; the rows in cox_preprocess_finegray's order; without
    strata, entry_time, ties='efron' and weights) the likelihood is the
    Fine-Gray subdistribution-hazard likelihood, through one bbx_coxfg handle
    (csrc/cox_finegray.hip): a row with a competing event stays in the later
    risk sets with weight G(t-) / G(T_i-), G the left-continuous Kaplan-Meier
    estimate of the censoring survivor function on the rows given."""

    _handle_attr = '_cox'

    def __init__(self, event_time, censoring_time, design, strata=None,
                 entry_time=None, ties='breslow', weights=None,
                 competing_time=None):
        _check_competing(competing_time, strata, entry_time, ties, weights)
        _check_ties(ties, strata, entry_time)
        weights = _check_weights(weights, len(event_time), strata, entry_time,
                                 ties)
        self.ties = ties
        self.weights = weights
        self.competing_time = None
        if competing_time is not None:
            self._init_finegray(event_time, censoring_time, competing_time,
                                design)
            return
        if entry_time is not None:
            if strata is not None:
                raise ValueError(
                    "entry_time together with strata is not supported: the "
                    "stratified counting-process model is not implemented.")
            self._init_interval(entry_time, event_time, censoring_time, design)
            return
        self.strata = None
        self.entry_time = None
        if strata is None:
            n_event, start, end, n_app = cox_risk_sets(event_time,
                                                       censoring_time)
        else:
            sptr, sne, start, end, last_set = cox_stratified_risk_sets(
                event_time, censoring_time, strata)
            n_event = int(np.sum(sne))
        if len(event_time) != design.shape[0]:
            raise ValueError(
                "Incompatible sizes of the outcome and design matrix.")
        if n_event == 0:
            raise ValueError("The Cox model needs at least one event.")
        if strata is None:
            self.n_appearance_in_risk_set = n_app
        else:
            self.strata = np.asarray(strata)
            self.stratum_ptr = sptr
            self.stratum_n_event = sne
            self.last_risk_set_index = last_set
        self.n_event = n_event
        self.event_time = np.asarray(event_time, dtype=np.float64)
        self.censoring_time = np.asarray(censoring_time, dtype=np.float64)
        self.risk_set_start_index = start
        self.risk_set_end_index = end
        self.design = design
        self.name = 'cox'
        self._ham_prefix = 'bbx_cox_'
        if ties == 'efron':
            # the plain model's rows and arrays on the bbx_coxef handle
            # (csrc/cox_efron.hip)
            self.tie_group_size = cox_tie_groups(event_time)[1]
            self._ham_prefix = 'bbx_coxef_'
        if weights is not None:
            # the plain model's rows and arrays on the bbx_coxw handle
            # (csrc/cox_weighted.hip)
            self._ham_prefix = 'bbx_coxw_'
        self._cox = c_void_p()
        self._location_serial = 0
        if strata is None:
            i32 = [np.ascontiguousarray(a, dtype=np.int32)
                   for a in (start, end, n_app)]
            # bbx_coxw_create takes the weights after the index arrays
            more = () if weights is None else (_ptr(weights),)
            _lib.check(self._ham_fn('create')(
                design.handle, n_event, _ptr(i32[0]), _ptr(i32[1]),
                _ptr(i32[2]), *more, byref(self._cox)))
        else:
            sptr = np.ascontiguousarray(sptr, dtype=np.int64)
            i32 = [np.ascontiguousarray(a, dtype=np.int32)
                   for a in (sne, start, end, last_set)]
            _lib.check(self._ham_fn('create_stratified')(
                design.handle, len(sne), _ptr(sptr), *[_ptr(a) for a in i32],
                byref(self._cox)))

    def _init_interval(self, entry_time, event_time, censoring_time, design):
        n_event, evrow, a, b, p, q, entry_perm = cox_interval_risk_sets(
            entry_time, event_time, censoring_time)
        if len(event_time) != design.shape[0]:
            raise ValueError(
                "Incompatible sizes of the outcome and design matrix.")
        if n_event == 0:
            raise ValueError("The Cox model needs at least one event.")
        self.strata = None
        self.n_event = n_event
        self.entry_time = np.asarray(entry_time, dtype=np.float64)
        self.event_time = np.asarray(event_time, dtype=np.float64)
        self.censoring_time = np.asarray(censoring_time, dtype=np.float64)
        self.event_row = evrow
        self.risk_set_start_index = a
        self.risk_set_entry_index = b
        self.n_event_by_exit = p
        self.n_event_by_entry = q
        self.entry_order = entry_perm
        self.design = design
        self.name = 'cox'
        self._ham_prefix = 'bbx_coxcp_'
        self._cox = c_void_p()
        self._location_serial = 0
        i32 = [np.ascontiguousarray(v, dtype=np.int32)
               for v in (evrow, a, b, p, q, entry_perm)]
        _lib.check(self._ham_fn('create')(
            design.handle, n_event, *[_ptr(v) for v in i32],
            byref(self._cox)))

    @classmethod
    def _finegray(cls, event_time, censoring_time, competing_time, design,
                  event_g, comp_rinv):
        """The Fine-Gray model with G from the caller: RegressionModel's,
        which computes it before it drops rows."""
        self = cls.__new__(cls)
        self.ties, self.weights = 'breslow', None
        self._init_finegray(event_time, censoring_time, competing_time, design,
                            event_g, comp_rinv)
        return self

    def _init_finegray(self, event_time, censoring_time, competing_time,
                       design, event_g=None, comp_rinv=None):
        n_event, evrow, a, b, p, comp_row = cox_finegray_risk_sets(
            event_time, censoring_time, competing_time)
        if len(event_time) != design.shape[0]:
            raise ValueError(
                "Incompatible sizes of the outcome and design matrix.")
        if n_event == 0:
            raise ValueError("The Cox model needs at least one event.")
        if event_g is None:
            # no row of these is dropped: they are all the data
            G = cox_finegray_censoring_survivor(event_time, censoring_time,
                                                competing_time)
            event_g, comp_rinv = G[evrow], 1. / G[comp_row]
        self.strata = None
        self.entry_time = None
        self.n_event = n_event
        self.event_time = np.asarray(event_time, dtype=np.float64)
        self.censoring_time = np.asarray(censoring_time, dtype=np.float64)
        self.competing_time = np.asarray(competing_time, dtype=np.float64)
        self.event_row = evrow
        self.risk_set_start_index = a
        self.n_competing_before = b
        self.n_event_by_exit = p
        self.competing_row = comp_row
        self.event_censoring_survivor = np.ascontiguousarray(
            event_g, dtype=np.float64)
        self.competing_inverse_survivor = np.ascontiguousarray(
            comp_rinv, dtype=np.float64)
        self.design = design
        self.name = 'cox'
        self._ham_prefix = 'bbx_coxfg_'
        self._cox = c_void_p()
        self._location_serial = 0
        i32 = [np.ascontiguousarray(v, dtype=np.int32)
               for v in (evrow, a, b, p, comp_row)]
        _lib.check(self._ham_fn('create')(
            design.handle, n_event, *[_ptr(v) for v in i32[:4]],
            len(comp_row), _ptr(i32[4]),
            _ptr(self.event_censoring_survivor),
            _ptr(self.competing_inverse_survivor), byref(self._cox)))

    @property
    def handle(self):
        return self._cox

    def compute_loglik_and_gradient(self, beta, loglik_only=False):
        """cox_model.py:180-204: (-inf, None) when a risk-set sum is 0."""
        return self._device_loglik_and_gradient(beta, loglik_only)

    def compute_hessian(self, beta):
        raise NotImplementedError()

    def get_hessian_matvec_operator(self, beta):
        """cox_model.py:251-273.  The handle holds one location: an operator
        stops working once a later call has moved it."""
        return self._hessian_operator(beta)

    # the trajectory's f(q0) (hmc.py:95-97) is the model's own likelihood
    hamiltonian_loglik_and_gradient = compute_loglik_and_gradient

    # ------------------------------------------------------ prediction
    def _coef_draws(self, coef):
        """coef (P,) or (P, S) as (the draws (S, P) C-contiguous, whether a
        draw axis was given)."""
        return _coef_draws(coef, self.n_pred)

    def _log_baseline_hazard(self, draws, grid_event):
        """bbx_<family>_baseline_hazard: (n_draw, grid_event.size)."""
        grid = np.ascontiguousarray(grid_event, dtype=np.int32).ravel()
        out = np.empty((len(draws), len(grid)))
        st = self._ham_fn('baseline_hazard')(
            self.handle, _ptr(draws), len(draws), len(grid), _ptr(grid),
            _ptr(out))
        if st == _lib.ERR_NUMERIC:
            raise ValueError(
                "The baseline hazard cannot be computed: %s."
                % _lib.last_error())
        _lib.check(st)
        return out

    def cumulative_baseline_hazard(self, coef, times=None, log=False):
        """Breslow's cumulative baseline hazard Lambda0 at `times` (None: the
        distinct event times) for coef of shape (P,) or (P, S) -- what
        samples['coef'] is: (times, value), value of shape (T,) or (T, S);
        for a stratified model (n_strata, T[, S]), the strata in np.unique
        order of their labels.  It is the hazard of a subject at the column
        means of the training rows (the design's centred columns); with
        ties='efron' the jump at a tied time is the sum of the group's
        1/phi_l, with weights a_k / H_k, with entry times H_k is the interval
        risk set's sum, and with competing_time Lambda0 is the cumulative
        baseline subdistribution hazard.  log=True returns log Lambda0 (-inf
        before the first event), which stays finite where Lambda0 itself
        under- or overflows.  One device call for all the draws.  ValueError
        if a draw has an empty risk-set sum."""
        draws, many = self._coef_draws(coef)
        times, grid = cox_hazard_grid(self, times)
        value = self._log_baseline_hazard(draws, grid)
        value = np.moveaxis(value.reshape((len(draws),) + grid.shape), 0, -1)
        if not many:
            value = value[..., 0]
        value = np.ascontiguousarray(value)
        return times, (value if log else np.exp(value))

    def martingale_residuals(self, coef):
        """delta_i - exp(eta_i) Lambda_i of every row at coef (P,), in the
        model's row order: the w of the gradient's row pass, Lambda_i the
        baseline hazard accumulated over the risk sets that hold row i.  With
        case weights it is a_i times that.  ValueError if a risk-set sum is
        empty."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.shape != (self.n_pred,):
            raise ValueError("coef must have length %d" % self.n_pred)
        out = np.empty(self.n_obs)
        st = self._ham_fn('residuals')(self.handle, _ptr(coef), _ptr(out))
        if st == _lib.ERR_NUMERIC:
            raise ValueError(
                "The residuals cannot be computed: %s." % _lib.last_error())
        _lib.check(st)
        return out

    def _new_design(self, X_new):
        """X_new (raw columns) as a design centred with the TRAINING design's
        column offsets, by the constructors that keep constant columns."""
        return _new_design(self.design, X_new, add_intercept=False)

    def predict_survival(self, coef, X_new=None, times=None, strata_new=None,
                         linear_predictor=None, return_draws=False):
        """Posterior survival S(t | x) = exp(-Lambda0(t) exp(x~ . beta)) of new
        rows over the draws coef (P,) or (P, S): a dict with 'time' (T,),
        'mean' and 'sd' (n_new, T) -- the mean and the population standard
        deviation over the draws -- and, with return_draws, 'draws'
        (n_new, T, S).  For the Fine-Gray model S is 1 - CIF.  Exactly one of
        X_new (n_new rows of the model's n_pred raw columns, NumPy or SciPy;
        centred with the training design's column means, never its own) and
        linear_predictor ((n_new,) for one draw, else (n_new, S): x~ . beta
        on the centred columns) is given.  With strata, strata_new holds the
        training stratum of every new row and `times` is required."""
        draws, many = self._coef_draws(coef)
        n_draw = len(draws)
        if (X_new is None) == (linear_predictor is None):
            raise ValueError(
                "Exactly one of X_new and linear_predictor must be given.")
        if X_new is not None:
            if not sparse.issparse(X_new):
                X_new = np.asarray(X_new, dtype=np.float64)
            if X_new.ndim != 2 or X_new.shape[1] != self.n_pred \
                    or X_new.shape[0] == 0:
                raise ValueError(
                    "X_new must have at least one row and the model's %d "
                    "columns: shape %s." % (self.n_pred, X_new.shape))
            n_new = X_new.shape[0]
            train = self.design
            if train.centered and train.column_offset is None:
                raise TypeError(
                    "The training design was adopted from device pointers "
                    "and keeps no host copy of its column offsets: pass "
                    "linear_predictor instead of X_new.")
        else:
            lp = np.asarray(linear_predictor, dtype=np.float64)
            if lp.ndim == 1 and not many:
                lp = lp[:, None]
            if lp.ndim != 2 or lp.shape[1] != n_draw or lp.shape[0] == 0:
                raise ValueError(
                    "linear_predictor must have shape (n_new,) for one draw "
                    "or (n_new, %d): %s."
                    % (n_draw, np.shape(linear_predictor)))
            n_new = lp.shape[0]
        group, n_group = None, 1
        if self.strata is not None:
            if strata_new is None:
                raise ValueError(
                    "The model is stratified: strata_new (the stratum of "
                    "every new row) is required.")
            strata_new = np.asarray(strata_new)
            if strata_new.shape != (n_new,):
                raise ValueError(
                    "strata_new must be a 1-d array with one label for each "
                    "new row.")
            labels = np.unique(self.strata)
            code = np.searchsorted(labels, strata_new)
            code[code == len(labels)] = 0
            if not np.all(labels[code] == strata_new):
                raise ValueError(
                    "Every label of strata_new must be a stratum of the "
                    "training rows.")
            group = np.ascontiguousarray(code, dtype=np.int32)
            n_group = len(labels)
        elif strata_new is not None:
            raise ValueError("strata_new is an argument of a stratified "
                             "model only.")
        times, grid = cox_hazard_grid(self, times)
        # every check is done: the device from here on
        if X_new is not None:
            new_design = self._new_design(X_new)
            eta = np.stack([new_design.dot(b) for b in draws])
        else:
            eta = np.ascontiguousarray(lp.T)
        log_hazard = self._log_baseline_hazard(draws, grid)
        n_time = len(times)
        mean, sd = np.empty((n_new, n_time)), np.empty((n_new, n_time))
        out = np.empty((n_new, n_time, n_draw)) if return_draws else None
        _lib.check(_lib.load().bbx_cox_survival_summary(
            self.design.device, n_new, n_time, n_draw, n_group, _ptr(eta),
            _ptr(log_hazard), _ptr(group), _ptr(mean), _ptr(sd), _ptr(out)))
        res = {'time': times, 'mean': mean, 'sd': sd}
        if return_draws:
            res['draws'] = out
        return res

    @staticmethod
    def simulate_outcome(X, beta, censoring_frac=.9, seed=None):
        """cox_model.py:275-298: exponential event times under a constant
        baseline hazard, exponential censoring."""
        if seed is not None:
            np.random.seed(seed)
        log_hazard_rate = X.dot(beta)
        log_hazard_rate = log_hazard_rate - np.max(log_hazard_rate)
        hazard_rate = np.exp(log_hazard_rate)
        event_time = np.random.exponential(scale=hazard_rate ** -1)
        t = np.quantile(event_time, 1 - censoring_frac)
        scale = - t / np.log(1 - (1 - censoring_frac))
        censoring_time = np.random.exponential(
            scale=scale * np.ones(len(hazard_rate)))
        censoring_time[event_time < censoring_time] = float("inf")
        event_time[event_time >= censoring_time] = float('inf')
        return event_time, censoring_time


def RegressionModel(outcome, X, family='linear', add_intercept=None,
                    center_predictor=True, device=0, storage='auto',
                    dense_storage_dtype='float64', entry_time=None,
                    ties='breslow', weights=None, dispersion=None,
                    dispersion_prior=None, cutpoints=None,
                    cutpoint_prior=None, df=None, quantile=None,
                    weibull_shape=None, weibull_shape_prior=None,
                    competing_time=None):
    """model/factory.py:10-68 with the design placed on an MI355X.  `X` may be
    a SciPy sparse matrix, a NumPy array, or an already built HipDesignMatrix.
    For family='cox', outcome = (event_time, censoring_time) or, for the
    stratified model, (event_time, censoring_time, strata): the rows are
    sorted into the model's order (and uninformative ones dropped) before the
    design goes to the GPU; a prebuilt HipDesignMatrix must already be in that
    order.  With `entry_time` (family='cox' without strata) the model is the
    counting-process form: a row is at risk from its entry time on, and the
    rows are sorted by cox_preprocess_interval.  With ties='efron'
    (family='cox' without strata and without entry_time) tied event times are
    handled by Efron's approximation instead of Breslow's rule; the row order
    is the same.  With `weights` (family='cox' without strata, entry_time and
    ties='efron'; one strictly positive case weight per row of X as given) the
    likelihood is the weighted partial likelihood; the weights are sorted and
    pruned with their rows.  With `competing_time` (family='cox' without
    strata, entry_time, ties='efron' and weights; inf where a row had no
    competing event, and exactly one of the three times of a row finite) the
    model is the Fine-Gray competing-risks model: the censoring survivor
    function is estimated on the rows as given, then the rows are sorted and
    pruned by cox_preprocess_finegray.  For family='poisson', outcome = y or
    (y, exposure) or, for the conditional Poisson model,
    (y, exposure, strata) (exposure may be None):
    the rows are sorted stratum-major and uninformative strata dropped
    (cpoisson_preprocess) before the design goes to the GPU; a prebuilt
    HipDesignMatrix must already be in that order.  For family='negbin',
    outcome = y or (y, exposure); `dispersion` (None: sampled, with the prior
    `dispersion_prior` = {'shape': .., 'rate': ..}, None: Gamma(2, 0.1); a
    number: held fixed) is the negative-binomial size.  Strata are refused:
    the conditional model has no negative-binomial form here.  For
    family='ordinal', outcome = y or (y, offset) with y in 0 ... K - 1, every
    category present; `cutpoints` (None: sampled, with the prior
    `cutpoint_prior` = {'sd': ..}, None: 10; K - 1 increasing numbers: held
    fixed) are the model's intercepts, so no intercept column is added
    (asking for one warns and drops it, as for Cox).  For family='weibull',
    outcome = (event_time, censoring_time) as for Cox -- exactly one of a
    row's two times finite -- but the rows stay in their order and an
    intercept is added; `weibull_shape` (None: sampled, with the prior
    `weibull_shape_prior` = {'shape': .., 'rate': ..}, None: Gamma(2, 1); a
    number: held fixed) is the Weibull shape k.  Strata are refused.  For
    family='probit', outcome = y in {0, 1}; a tuple with n_trial is refused
    (the binomial outcome is the logit model's).  For family='student_t',
    outcome = y, finite, and `df` > 0 (None: 4) is the fixed degrees of
    freedom of the errors.  For family='quantile', outcome = y, finite, and
    `quantile` in (0, 1) (None: 1/2, the median) is the fixed level whose
    conditional quantile is modelled.  For family='tobit', outcome = (y, status) with
    status 0 (observed), 1 (right-censored: the truth lies above y) or 2
    (left-censored: at or below y); for family='lognormal', outcome =
    (event_time, censoring_time) as for the Weibull model, fitted as the
    log-normal accelerated-failure-time model (coefficients are log time
    ratios).  (The
    eight keywords stand before `competing_time`, which stays the last one:
    pass them by name.)"""
    if entry_time is not None and family != 'cox':
        raise ValueError("entry_time is an argument of family='cox' only.")
    if ties != 'breslow' and family != 'cox':
        raise ValueError("ties is an argument of family='cox' only.")
    if weights is not None and family != 'cox':
        raise ValueError("weights is an argument of family='cox' only.")
    if competing_time is not None and family != 'cox':
        raise ValueError("competing_time is an argument of family='cox' only.")
    if dispersion is not None and family != 'negbin':
        raise ValueError("dispersion is an argument of family='negbin' only.")
    if dispersion_prior is not None and family != 'negbin':
        raise ValueError(
            "dispersion_prior is an argument of family='negbin' only.")
    if cutpoints is not None and family != 'ordinal':
        raise ValueError("cutpoints is an argument of family='ordinal' only.")
    if cutpoint_prior is not None and family != 'ordinal':
        raise ValueError(
            "cutpoint_prior is an argument of family='ordinal' only.")
    if weibull_shape is not None and family != 'weibull':
        raise ValueError(
            "weibull_shape is an argument of family='weibull' only.")
    if weibull_shape_prior is not None and family != 'weibull':
        raise ValueError(
            "weibull_shape_prior is an argument of family='weibull' only.")
    if family == 'weibull' and not (isinstance(outcome, tuple)
                                    and len(outcome) == 2):
        raise ValueError(
            "The Weibull model takes outcome = (event_time, censoring_time): "
            "strata are not supported.")
    if family == 'ordinal' and isinstance(outcome, tuple) \
            and len(outcome) != 2:
        raise ValueError(
            "The ordinal model takes outcome = y or (y, offset): strata are "
            "not supported.")
    if family == 'negbin' and isinstance(outcome, tuple) \
            and len(outcome) != 2:
        raise ValueError(
            "The negative-binomial model takes outcome = y or (y, exposure): "
            "strata are not supported, the conditional model has no "
            "negative-binomial form here.")
    if df is not None and family != 'student_t':
        raise ValueError("df is an argument of family='student_t' only.")
    if quantile is not None and family != 'quantile':
        raise ValueError(
            "quantile is an argument of family='quantile' only.")
    if family == 'quantile':
        outcome = _finite_outcome(outcome, X.shape[0], 'quantile')
        quantile = _checked_quantile(.5 if quantile is None else quantile)
    if family == 'probit':
        # (before the design goes to the GPU)
        outcome = _binary_outcome(outcome, X.shape[0])
    if family == 'student_t':
        outcome = _finite_outcome(outcome, X.shape[0])
        df = _checked_df(4. if df is None else df)
    if family in ('tobit', 'lognormal'):
        if not (isinstance(outcome, tuple) and len(outcome) == 2):
            raise ValueError(
                "The %s model takes outcome = %s." % (
                    family, "(y, status)" if family == 'tobit'
                    else "(event_time, censoring_time): strata are not "
                    "supported"))
        # (before the design goes to the GPU)
        if family == 'tobit':
            outcome = _censored_outcome(outcome[0], outcome[1], X.shape[0])
        else:
            _survival_outcome(outcome[0], outcome[1], X.shape[0])
    stratified_poisson = (family == 'poisson' and isinstance(outcome, tuple)
                          and len(outcome) == 3)
    if add_intercept is None:
        add_intercept = family not in ('cox', 'ordinal') \
            and not stratified_poisson
    if family == 'ordinal':
        if add_intercept:
            add_intercept = False
            warn("Intercept is not identifiable in the ordinal model (the "
                 "cutpoints are its intercepts) and won't be added.")
        if isinstance(X, HipDesignMatrix) and X.intercept_added:
            raise ValueError("The ordinal model takes a design without an "
                             "intercept column.")
    if stratified_poisson:
        if add_intercept:
            add_intercept = False
            warn("Intercept is not identifiable in the conditional Poisson "
                 "model and won't be added.")
        y, exposure, strata = outcome
        if isinstance(X, HipDesignMatrix):
            with catch_warnings():
                simplefilter('ignore')
                keep = cpoisson_preprocess(y, exposure, strata)[4]
            if not np.array_equal(keep, np.arange(len(np.asarray(y)))):
                raise ValueError(
                    "A prebuilt HipDesignMatrix must have its rows in the "
                    "conditional Poisson model's order (stratum by stratum "
                    "in the sorted order of the labels, every stratum with "
                    "a positive count and more than one row); pass X as a "
                    "NumPy or SciPy matrix to have it sorted.")
            if X.intercept_added:
                raise ValueError("The conditional Poisson model takes a "
                                 "design without an intercept column.")
        else:
            y, exposure, strata, X, _ = cpoisson_preprocess(
                y, exposure, strata, X)
    if family == 'cox':
        if add_intercept:
            add_intercept = False
            warn("Intercept is not identifiable in Cox model and won't be "
                 "added.")
        strata = None
        if len(outcome) == 3:
            event_time, censoring_time, strata = outcome
        else:
            event_time, censoring_time = outcome
        _check_competing(competing_time, strata, entry_time, ties, weights)
        if entry_time is not None and strata is not None:
            raise ValueError(
                "entry_time together with strata is not supported: the "
                "stratified counting-process model is not implemented.")
        _check_ties(ties, strata, entry_time)
        weights = _check_weights(weights, len(np.asarray(event_time)), strata,
                                 entry_time, ties)
        if competing_time is not None:
            with catch_warnings():
                if isinstance(X, HipDesignMatrix):
                    simplefilter('ignore')
                event_time, censoring_time, competing_time, sorted_X, keep, \
                    event_g, comp_rinv = cox_preprocess_finegray(
                        event_time, censoring_time, competing_time,
                        None if isinstance(X, HipDesignMatrix) else X)
            if isinstance(X, HipDesignMatrix):
                if not np.array_equal(keep, np.arange(X.shape[0])):
                    raise ValueError(
                        "A prebuilt HipDesignMatrix must have its rows in the "
                        "Fine-Gray model's order (by increasing event, "
                        "competing or censoring time, at the same time "
                        "events before competing events before censored "
                        "rows, none censored before the first event); pass "
                        "X as a NumPy or SciPy matrix to have it sorted.")
                if X.intercept_added:
                    raise ValueError("The Cox model takes a design without "
                                     "an intercept column.")
            else:
                X = sorted_X
        elif entry_time is not None:
            if isinstance(X, HipDesignMatrix):
                with catch_warnings():
                    simplefilter('ignore')
                    keep = cox_preprocess_interval(
                        entry_time, event_time, censoring_time)[4]
                if not np.array_equal(keep, np.arange(X.shape[0])):
                    raise ValueError(
                        "A prebuilt HipDesignMatrix must have its rows in the "
                        "counting-process Cox model's order (by increasing "
                        "event or censoring time, events before the rows "
                        "censored at the same time, every row in some risk "
                        "set); pass X as a NumPy or SciPy matrix to have it "
                        "sorted.")
                if X.intercept_added:
                    raise ValueError("The Cox model takes a design without "
                                     "an intercept column.")
            else:
                entry_time, event_time, censoring_time, X, _ = \
                    cox_preprocess_interval(entry_time, event_time,
                                            censoring_time, X)
        elif isinstance(X, HipDesignMatrix):
            et = np.asarray(event_time, dtype=np.float64)
            ct = np.asarray(censoring_time, dtype=np.float64)
            if strata is None:
                in_order = cox_sort_permutation(et, ct) is None \
                    and not np.any(ct < np.min(et))
            else:
                with catch_warnings():
                    simplefilter('ignore')
                    keep = cox_preprocess_stratified(et, ct, strata)[4]
                in_order = np.array_equal(keep, np.arange(len(et)))
            if not in_order:
                raise ValueError(
                    "A prebuilt HipDesignMatrix must have its rows in the Cox "
                    "model's order (events by increasing time, then censored "
                    "rows by decreasing censoring time, none censored before "
                    "the first event; with strata, stratum by stratum in the "
                    "sorted order of the labels, each stratum in that order "
                    "and with an event); pass X as a NumPy or SciPy matrix "
                    "to have it sorted.")
            if X.intercept_added:
                raise ValueError("The Cox model takes a design without an "
                                 "intercept column.")
        elif strata is None:
            event_time, censoring_time, X, keep = cox_preprocess(
                event_time, censoring_time, X)
            if weights is not None:
                weights = weights[keep]
        else:
            event_time, censoring_time, strata, X, _ = \
                cox_preprocess_stratified(event_time, censoring_time, strata,
                                          X)
    if isinstance(X, HipDesignMatrix):
        design = X
    elif sparse.issparse(X):
        design = HipSparseDesignMatrix(
            X, add_intercept=add_intercept, center_predictor=center_predictor,
            device=device, storage=storage)
    else:
        design = HipDenseDesignMatrix(
            X, add_intercept=add_intercept, center_predictor=center_predictor,
            device=device, storage_dtype=dense_storage_dtype)
    if family == 'linear':
        return LinearModel(outcome, design)
    if family == 'logit':
        if isinstance(outcome, tuple):
            n_success, n_trial = outcome
        else:
            n_success, n_trial = outcome, None
        return LogisticModel(n_success, n_trial, design)
    if family == 'probit':
        return ProbitModel(outcome, design)
    if family == 'student_t':
        return StudentTModel(outcome, design, df)
    if family == 'quantile':
        return QuantileModel(outcome, design, quantile)
    if family == 'tobit':
        return CensoredNormalModel(outcome[0], outcome[1], design)
    if family == 'lognormal':
        return LogNormalAFTModel(outcome[0], outcome[1], design)
    if family == 'cox':
        if competing_time is not None:
            return CoxModel._finegray(event_time, censoring_time,
                                      competing_time, design, event_g,
                                      comp_rinv)
        return CoxModel(event_time, censoring_time, design, strata,
                        entry_time, ties, weights)
    if family == 'poisson':
        if stratified_poisson:
            return PoissonModel(y, exposure, design, strata)
        if isinstance(outcome, tuple):
            y, exposure = outcome
        else:
            y, exposure = outcome, None
        return PoissonModel(y, exposure, design)
    if family == 'negbin':
        if isinstance(outcome, tuple):
            y, exposure = outcome
        else:
            y, exposure = outcome, None
        return NegBinModel(y, exposure, design, dispersion, dispersion_prior)
    if family == 'weibull':
        event_time, censoring_time = outcome
        return WeibullModel(event_time, censoring_time, design, weibull_shape,
                            weibull_shape_prior)
    if family == 'ordinal':
        if isinstance(outcome, tuple):
            y, offset = outcome
        else:
            y, offset = outcome, None
        return OrdinalModel(y, design, offset, cutpoints, cutpoint_prior)
    raise NotImplementedError()
