"""The No-U-Turn draw of the regression coefficients:
NoUTurnSampler.generate_next_state (hamiltonian_monte_carlo/nuts.py:108-188)
with the trajectory tree on the device (csrc/hamiltonian.hpp; bbx_cox_nuts_*,
bbx_logit_nuts_*).

One doubling is one device call and one host wait.  Every random number comes
from the global NumPy stream in the reference's order: the momentum, the
exponential of the slice variable, the max_height directions, then one
uniform per tree merge that happens, in post-order.  A half-tree of height h
needs at most 2^h of them (2^h - 1 merges inside it and the merge into the
main tree) and fewer when it ends early, so the candidates are drawn from a
copy of the generator's state, handed to the device, and the stream is then
advanced by the number the device consumed."""
import math
from warnings import warn

import numpy as np

MAX_HEIGHT = 10          # NUTS_MAXH of csrc/hamiltonian.hpp


def draw_ahead(n):
    """n numbers of np.random.uniform() and the generator state before them;
    `advance` then leaves the stream as if only the first k had been drawn."""
    state = np.random.get_state()
    return np.random.rand(n), state


def advance(state, k):
    np.random.set_state(state)
    if k > 0:
        np.random.rand(k)


def generate_next_state(model, dt, q, precond_scale, precond_prior_prec,
                        logp=None, grad=None, p=None, max_height=10,
                        hamiltonian_error_tol=100., warning_requested=True):
    """nuts.py:108-151 on f(q) = loglik(precond_scale q) - 1/2
    sum(precond_prior_prec q^2) of a device Cox or logit model.  Returns (q, info);
    info has the reference's keys plus 'directions', 'n_uniform' (uniforms
    consumed by the merges) and 'momentum'."""
    if not 1 <= max_height <= MAX_HEIGHT:
        raise ValueError("max_height must be in [1, %d]" % MAX_HEIGHT)
    q = np.ascontiguousarray(q, dtype=np.float64)
    n_grad_evals = 0
    if logp is None or grad is None:
        loglik, g = model.hamiltonian_loglik_and_gradient(q * precond_scale)
        logp = loglik + np.sum(-precond_prior_prec * q ** 2) / 2
        if math.isfinite(logp):
            grad = precond_scale * g
            grad += -precond_prior_prec * q
        else:
            grad = np.zeros_like(q)
        n_grad_evals += 1
    if p is None:
        p = np.random.randn(len(q))
    logp_joint = -(-logp + 0.5 * np.dot(p, p))
    logp_joint_threshold = logp_joint - np.random.exponential()
    directions = 2 * (np.random.rand(max_height) < 0.5) - 1
    model.nuts_begin(precond_scale, precond_prior_prec, q, p, logp, grad,
                     logp_joint, logp_joint_threshold, hamiltonian_error_tol)
    height, n_uniform, n_step = 0, 0, 0
    while True:
        uniforms, state = draw_ahead(2 ** height)
        out = model.nuts_doubling(dt, int(directions[height]), height,
                                  uniforms)
        advance(state, out['n_uniform'])
        n_uniform += out['n_uniform']
        n_step += out['n_steps']
        height += 1
        if out['u_turn_detected'] or out['instability_detected'] \
                or height >= max_height:
            break
    maxed_before_u_turn = height >= max_height \
        and not out['u_turn_detected']
    q, logp, grad = model.nuts_sample()
    n_grad_evals += n_step
    if warning_requested:
        if out['instability_detected']:
            warn("Numerical integration became unstable while simulating a "
                 "NUTS trajectory.")
        if maxed_before_u_turn:
            warn('The trajectory tree reached the max height of {:d} before '
                 'meeting the U-turn condition.'.format(max_height))
    info = {
        'logp': logp,
        'grad': grad,
        'ave_accept_prob': out['ave_accept_prob'],
        'ave_hamiltonian_error': out['ave_hamiltonian_error'],
        'n_grad_evals': n_grad_evals,
        'tree_height': height,
        'u_turn_detected': out['u_turn_detected'],
        'instability_detected': out['instability_detected'],
        'last_doubling_rejected': out['doubling_rejected'],
        'directions': directions,
        'n_uniform': n_uniform,
        'momentum': p,
    }
    return q, info
