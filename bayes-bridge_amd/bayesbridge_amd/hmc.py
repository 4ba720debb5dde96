"""HMC draw of the regression coefficients, the reference's only sampler for
the Cox model and one it also accepts for the logit model: `sample_by_hmc` and its stability-limit estimate
(reg_coef_sampler.py:105-240), the trajectory and accept step (hmc.py:88-174),
the step-size adapter (stepsize_adapter.py:6-131), the stability-estimate
stabilizer (reg_coef_sampler.py:394-429) and the Hessian principal-component
summary (reg_coef_posterior_summarizer.py:22-67).

The trajectory runs on the device in one call (bbx_cox_hmc_trajectory /
bbx_logit_hmc_trajectory: one host synchronisation per trajectory).  The largest Hessian eigenvalue comes
from SciPy's ARPACK on the host, as in the reference, with the device Hessian
matvec behind it.  Every random number (the first eigenvector guess, dt, the
integration time, the momentum, the accept uniform) comes from the global
NumPy stream in the reference's order.  method='nuts' replaces the trajectory
and the accept step by the No-U-Turn draw of nuts.py."""
import math
from math import copysign, exp, log, log10
from warnings import warn

import numpy as np
import scipy.sparse.linalg
import scipy.stats

from . import nuts
from .reg_coef_sampler import (HipRegressionCoefficientSampler,
                               RegressionCoeffficientPosteriorSummarizer,
                               compute_prior_shrunk_scale)


class DirectionSummarizer():
    """Running average of a direction up to sign
    (reg_coef_posterior_summarizer.py:43-67, method 'average')."""

    def __init__(self, summary_method='average'):
        self.method = summary_method
        self.n_averaged = 0
        self.v = None

    def update(self, v):
        if self.n_averaged == 0 or self.method == 'previous':
            self.v = v
        else:
            v *= np.sign(np.inner(self.v, v))
            weight = 1 / (1 + self.n_averaged)
            self.v = weight * v + (1 - weight) * self.v
        self.n_averaged += 1

    def get_mean(self):
        return self.v


class HMCPosteriorSummarizer(RegressionCoeffficientPosteriorSummarizer):
    """The coefficient summary plus the Hessian principal component
    (reg_coef_posterior_summarizer.py:22-35)."""

    def __init__(self, n_coef, n_unshrunk, regularizing_slab_size):
        super().__init__(n_coef, n_unshrunk, regularizing_slab_size)
        self.pc_summarizer = DirectionSummarizer('average')

    def update_precond_hessian_pc(self, pc):
        self.pc_summarizer.update(pc)

    def estimate_precond_hessian_pc(self):
        return self.pc_summarizer.get_mean()


class RobbinsMonroStepsizer():
    """stepsize_adapter.py:182-209."""

    def __init__(self, init=1., decay_exponent=1., reference_iteration=None,
                 size_at_reference=None):
        self.init = init
        self.exponent = decay_exponent
        if reference_iteration is not None and size_at_reference is not None:
            self.scale = reference_iteration / (
                (init / size_at_reference) ** (1 / decay_exponent) - 1)
        else:
            self.scale = 1.

    def calculate_stepsize(self, n_iter):
        return self.init / (1 + n_iter / self.scale) ** self.exponent


class HamiltonianBasedStepsizeAdapter():
    """stepsize_adapter.py:6-131 (the 'piecewise' transform)."""

    def __init__(self, init_stepsize, target_accept_prob=.9,
                 init_adaptsize=1., adapt_decay_exponent=1.,
                 reference_iteration=500, adaptsize_at_reference=.05):
        if init_stepsize <= 0:
            raise ValueError("The initial stepsize must be positive.")
        self.log_stepsize = log(init_stepsize)
        self.log_stepsize_averaged = self.log_stepsize
        self.n_averaged = 0
        self.target_accept_prob = target_accept_prob
        if target_accept_prob <= 0 or target_accept_prob >= 1:
            raise ValueError("Target probability must be within (0, 1).")
        delta = 4 * scipy.stats.norm.ppf(target_accept_prob / 2) ** 2
        self.target_log10_hamiltonian_error = \
            .5 * log10(delta + delta ** 2 / 4)
        self.rm_stepsizer = RobbinsMonroStepsizer(
            init=init_adaptsize, decay_exponent=adapt_decay_exponent,
            reference_iteration=reference_iteration,
            size_at_reference=adaptsize_at_reference)

    def get_current_stepsize(self, averaged=False):
        return exp(self.log_stepsize_averaged if averaged
                   else self.log_stepsize)

    def adapt_stepsize(self, hamiltonian_error):
        rm_stepsize = self.rm_stepsizer.calculate_stepsize(self.n_averaged)
        self.n_averaged += 1
        self.log_stepsize += rm_stepsize * self.transform_to_adaptsize(
            hamiltonian_error)
        weight = 1 / self.n_averaged
        self.log_stepsize_averaged = (
            weight * self.log_stepsize
            + (1 - weight) * self.log_stepsize_averaged)
        return exp(self.log_stepsize)

    def transform_to_adaptsize(self, error, upper_bound=1.):
        log10_error = -float('inf') if error == 0. else log10(abs(error))
        target = self.target_log10_hamiltonian_error
        if log10_error > target:
            adapt_size = (target - log10_error) / .301
        else:
            adapt_size = (target - log10_error) / 3
        if abs(adapt_size) > upper_bound:
            adapt_size = copysign(1., adapt_size)
        return adapt_size


class StabilityEstimateStabilizer():
    """Detects and adjusts unusually large stability-limit estimates
    (reg_coef_sampler.py:394-429)."""

    def __init__(self, n_warmup=100):
        self.stability_estimate = []
        self.n_update = 0
        self.n_warmup = n_warmup

    def update(self, estimate):
        self.stability_estimate.append(estimate)
        self.n_update += 1

    def stabilize(self, estimate):
        if self.n_update < self.n_warmup:
            return estimate
        gaussian_cdf_at_onestd = .8414
        est = np.array(self.stability_estimate[:self.n_update])
        cdf_at_estimate = np.mean(est < estimate)
        if cdf_at_estimate <= gaussian_cdf_at_onestd:
            return estimate
        median = np.median(est)
        at_cdf = np.quantile(est, gaussian_cdf_at_onestd)
        one_std_dist = at_cdf - median
        above = min(2., scipy.stats.norm.ppf(cdf_at_estimate) - 1.)
        return at_cdf + one_std_dist * above


def generate_next_state(model, dt, n_step, q0, logp0, grad0, precond_scale,
                        precond_prior_prec, hamiltonian_tol=100.):
    """hmc.py:88-134 with the trajectory (hmc.py:137-174) on the device.
    logp0, grad0: f at q0 (one gradient evaluation, counted here)."""
    n_grad_evals = 1
    P = len(q0)
    p0 = np.random.randn(P)                                   # dynamics.py
    if n_step == 0:
        warn("The number of integration steps was set to be 0.")
    traj = model.hmc_trajectory(dt, n_step, precond_scale,
                                precond_prior_prec, q0, p0, logp0, grad0,
                                hamiltonian_tol)
    q, ham = traj['q'], traj['hamiltonian']
    n_grad_evals += traj['n_steps']
    instability_detected = traj['instability']
    if instability_detected:
        warn("Numerical integration became unstable while simulating the HMC "
             "trajectory.")
        acceptprob = 0.
        hamiltonian_error = -float('inf')
    else:
        hamiltonian_error = (-ham[1]) - (-ham[0])
        acceptprob = min(1, np.exp(hamiltonian_error))
    accepted = acceptprob > np.random.rand()
    if not accepted:
        q = q0
    info = {'accepted': accepted, 'accept_prob': acceptprob,
            'hamiltonian_error': hamiltonian_error,
            'instability_detected': instability_detected,
            'n_grad_evals': n_grad_evals, 'momentum': p0}
    return q, info


class HipHMCCoefficientSampler():
    """The 'hmc' branch of SparseRegressionCoefficientSampler
    (reg_coef_sampler.py:20-58,105-279) on a device Cox or logit model."""

    _sampling_info_attributes = ('regcoef_summarizer',
                                 'stability_adjustment_adapter',
                                 'stability_est_stabilizer')

    def __init__(self, n_coef, prior_sd_for_unshrunk,
                 stability_estimate_stabilized=False,
                 regularizing_slab_size=float('inf')):
        self.prior_sd_for_unshrunk = np.asarray(prior_sd_for_unshrunk,
                                                dtype=np.float64)
        self.n_unshrunk = len(self.prior_sd_for_unshrunk)
        self.regularizing_slab_size = regularizing_slab_size
        self.regcoef_summarizer = HMCPosteriorSummarizer(
            n_coef, self.n_unshrunk, regularizing_slab_size)
        self.stability_adjustment_adapter = HamiltonianBasedStepsizeAdapter(
            init_stepsize=.3, target_accept_prob=.95)
        self.stability_est_stabilizer = StabilityEstimateStabilizer()
        self.stability_est_stabilized = stability_estimate_stabilized

    # the L-BFGS-B mode search of the chain's initialisation
    search_mode = HipRegressionCoefficientSampler.search_mode

    def get_internal_state(self):
        return {k: getattr(self, k) for k in self._sampling_info_attributes}

    def set_internal_state(self, state):
        for k in self._sampling_info_attributes:
            setattr(self, k, state[k])

    def compute_preconditioning_scale(self, gscale, lscale,
                                      regcoef_precond_post_sd):
        n_coef = len(regcoef_precond_post_sd)
        nu = n_coef - len(lscale)
        precond_scale = np.ones(n_coef)
        precond_scale[nu:] = compute_prior_shrunk_scale(
            gscale, lscale, self.regularizing_slab_size)
        if nu > 0:
            precond_scale[:nu] = regcoef_precond_post_sd[:nu]
        precond_prior_prec = np.concatenate((
            (self.prior_sd_for_unshrunk / precond_scale[:nu]) ** -2,
            np.ones(len(lscale))))
        return precond_scale, precond_prior_prec

    def compute_stability_limit(self, gscale, lscale, model, precond_scale,
                                precond_prior_prec):
        """2 / sqrt(largest eigenvalue of the preconditioned negative
        Hessian) at the extrapolated conditional mean
        (reg_coef_sampler.py:203-240): ARPACK k=1, ncv=2, tol=.1."""
        location = self.regcoef_summarizer.extrapolate_coef_condmean(
            gscale, lscale)
        pc_estimate = self.regcoef_summarizer.estimate_precond_hessian_pc()
        loglik_hessian_matvec = model.get_hessian_matvec_operator(location)
        counter = [0]

        def matvec(v):
            counter[0] += 1
            v = np.ravel(v)
            return precond_prior_prec * v \
                - precond_scale * loglik_hessian_matvec(precond_scale * v)

        P = len(location)
        op = scipy.sparse.linalg.LinearOperator((P, P), matvec)
        if pc_estimate is None:
            pc_estimate = np.random.randn(P)
        eigval, eigvec = scipy.sparse.linalg.eigsh(
            op, k=1, tol=.1, v0=pc_estimate, ncv=2)
        max_curvature = eigval[0]
        if max_curvature <= 0:
            raise ArithmeticError(
                "Numerical instability occured during the Lancoz iteration "
                "and a negative curvature value returned for a log-concave "
                "distribution. Likely caused by divergence of regression "
                "coefficients to infinity. Check the input data and / or "
                "place an informative prior.")
        self.regcoef_summarizer.update_precond_hessian_pc(np.squeeze(eigvec))
        return 2 / np.sqrt(max_curvature), counter[0]

    def sample_by_hmc(self, coef, gscale, lscale, model, method='hmc',
                      max_step=512):
        """reg_coef_sampler.py:105-172, methods 'hmc' and 'nuts'."""
        if method not in ('hmc', 'nuts'):
            raise NotImplementedError()
        post_sd = self.regcoef_summarizer.estimate_coef_precond_scale_sd()
        precond_scale, precond_prior_prec = \
            self.compute_preconditioning_scale(gscale, lscale, post_sd)
        stability_limit, n_hessian_matvec = self.compute_stability_limit(
            gscale, lscale, model, precond_scale, precond_prior_prec)
        if self.stability_est_stabilized:
            pre = stability_limit
            stability_limit = self.stability_est_stabilizer.stabilize(
                stability_limit)
            self.stability_est_stabilizer.update(pre)
        adjustment_factor = \
            self.stability_adjustment_adapter.get_current_stepsize()
        dt = np.random.uniform(.5, 1) * (adjustment_factor * stability_limit)
        coef_precond = coef / precond_scale
        if method == 'nuts':
            return self._finish_nuts(
                coef_precond, dt, model, precond_scale, precond_prior_prec,
                int(math.log2(max_step)), gscale, lscale, n_hessian_matvec,
                stability_limit, adjustment_factor)
        integration_time = np.pi / 2 * np.random.uniform(.8, 1.)
        n_step = min(int(np.ceil(integration_time / dt)), max_step)
        # f(q0) (hmc.py:95-97): the log-density and gradient in the
        # preconditioned coordinates (reg_coef_sampler.py:259-279)
        loglik, grad = model.hamiltonian_loglik_and_gradient(
            coef_precond * precond_scale)
        logp0 = loglik + np.sum(-precond_prior_prec * coef_precond ** 2) / 2
        if math.isfinite(logp0):
            grad0 = precond_scale * grad
            grad0 += -precond_prior_prec * coef_precond
        else:
            grad0 = np.zeros_like(coef_precond)
        coef_precond, hmc_info = generate_next_state(
            model, dt, n_step, coef_precond, logp0, grad0, precond_scale,
            precond_prior_prec)
        info = {key: hmc_info[key] for key in (
            'accepted', 'accept_prob', 'n_grad_evals', 'instability_detected')}
        info['n_integrator_step'] = n_step
        coef = coef_precond * precond_scale
        self.regcoef_summarizer.update(coef, gscale, lscale)
        self.stability_adjustment_adapter.adapt_stepsize(
            hmc_info['hamiltonian_error'])
        info['n_hessian_matvec'] = n_hessian_matvec
        info['stepsize'] = dt
        info['stability_limit_est'] = stability_limit
        info['stability_adjustment_factor'] = adjustment_factor
        info['momentum'] = hmc_info['momentum']
        info['hamiltonian_error'] = hmc_info['hamiltonian_error']
        return coef, info

    def _finish_nuts(self, coef_precond, dt, model, precond_scale,
                     precond_prior_prec, max_height, gscale, lscale,
                     n_hessian_matvec, stability_limit, adjustment_factor):
        """reg_coef_sampler.py:149-172."""
        coef_precond, nuts_info = nuts.generate_next_state(
            model, dt, coef_precond, precond_scale, precond_prior_prec,
            max_height=max_height)
        info = {key: nuts_info[key] for key in (
            'ave_accept_prob', 'n_grad_evals', 'tree_height',
            'instability_detected')}
        coef = coef_precond * precond_scale
        self.regcoef_summarizer.update(coef, gscale, lscale)
        self.stability_adjustment_adapter.adapt_stepsize(
            nuts_info['ave_hamiltonian_error'])
        info['n_hessian_matvec'] = n_hessian_matvec
        info['stepsize'] = dt
        info['stability_limit_est'] = stability_limit
        info['stability_adjustment_factor'] = adjustment_factor
        info['momentum'] = nuts_info['momentum']
        info['hamiltonian_error'] = nuts_info['ave_hamiltonian_error']
        return coef, info
