"""NumPy oracle of the Cox likelihood (cox_model.py:180-273) in two forms:

  * a linear-time restatement with the device's structure (csrc/cox.hip): the
    risk-set sums as a suffix sum over the events plus a prefix sum over the
    censored rows -- never a difference of two large prefix sums;
  * a brute-force form through the explicit n_event x n matrix of
    multinomial probabilities, defined directly from the risk-set ranges.

The second is the definition the first is checked against where the
reference itself fails (a tied latest event time).  Also a host velocity-Verlet
loop (dynamics.py, hmc.py:137-174) driven by the oracle, to check the device
trajectory against."""
import math

import numpy as np


def risk_sums(arr, n_event, start, end):
    """sum(arr[start_k : end_k + 1]) for every k < n_event."""
    suffix = np.cumsum(arr[:n_event][::-1])[::-1]
    prefix = np.cumsum(arr[n_event:])
    total = suffix[start].copy()
    late = end >= n_event
    total[late] += prefix[end[late] - n_event]
    return total


def loglik_grad(X, beta, n_event, start, end, n_app):
    eta = X @ beta
    eta = eta - np.max(eta)
    h = np.exp(eta)
    H = risk_sums(h, n_event, start, end)
    if np.any(H == 0.):
        return -math.inf, None
    loglik = np.sum(eta[:n_event] - np.log(H))
    c = np.cumsum(1. / H)
    w = -c[n_app - 1] * h
    w[:n_event] += 1.
    return loglik, X.T @ w


def hessian_matvec(X, beta, v, n_event, start, end, n_app,
                   dtype=np.float64):
    """dtype=np.longdouble: everything after X beta and X v in extended
    precision (dense X only).  r = rowsum .* u - W^T W u cancels; where eta
    spreads widely the float64 form itself is off by ~3e-9 of the result."""
    eta = (X @ beta).astype(dtype)
    h = np.exp(eta - np.max(eta))
    H = risk_sums(h, n_event, start, end)
    u = (X @ v).astype(dtype)
    Wu = risk_sums(h * u, n_event, start, end) / H
    WtWu = h * np.cumsum(Wu / H)[n_app - 1]
    rowsum = np.cumsum(1. / H)[n_app - 1] * h
    Xt = X.T if dtype is np.float64 else X.T.astype(dtype)
    return (-(Xt @ (rowsum * u - WtWu))).astype(np.float64)


def explicit_matrix(X, beta, n_event, start, end):
    """W[k, i] = h_i / H_k for i in [start_k, end_k], 0 elsewhere."""
    eta = X @ beta
    h = np.exp(eta - np.max(eta))
    n = len(h)
    mask = np.zeros((n_event, n))
    for k in range(n_event):
        mask[k, start[k]:end[k] + 1] = 1.
    H = mask @ h
    return eta - np.max(eta), h, mask, H


def brute_loglik_grad(X, beta, n_event, start, end):
    eta, h, mask, H = explicit_matrix(X, beta, n_event, start, end)
    if np.any(H == 0.):
        return -math.inf, None
    W = mask * h[None, :] / H[:, None]
    ind = np.zeros(len(h))
    ind[:n_event] = 1.
    return np.sum(eta[:n_event] - np.log(H)), X.T @ (ind - W.sum(axis=0))


def brute_hessian_matvec(X, beta, v, n_event, start, end):
    eta, h, mask, H = explicit_matrix(X, beta, n_event, start, end)
    W = mask * h[None, :] / H[:, None]
    u = X @ v
    return -X.T @ (W.sum(axis=0) * u - W.T @ (W @ u))


def risk_sets_by_loops(event_time, censoring_time):
    """cox_model.py:150-178 as the reference writes it (O(n n_event))."""
    n = len(event_time)
    n_event = n - int(np.sum(np.isinf(event_time)))
    ev = event_time[:n_event]
    cens = np.flip(censoring_time[n_event:])
    start = np.zeros(n_event, dtype=np.int64)
    for i in range(1, n_event):
        start[i] = start[i - 1] if ev[i - 1] == ev[i] else i
    n_cens = np.array([np.searchsorted(cens, t) for t in ev], dtype=np.int64)
    end = n - 1 - n_cens
    n_app = np.zeros(n, dtype=np.int64)
    for k in range(n_event):
        n_app[start[k]:end[k] + 1] += 1
    return n_event, start, end, n_app


def precond_f(X, scale, prior_prec, risk):
    """f(q) of reg_coef_sampler.py:259-279 on the oracle likelihood."""
    def f(q):
        ll, g = loglik_grad(X, q * scale, *risk)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def trajectory(f, dt, n_step, q0, p0, logp0, grad0, tol=100.):
    """simulate_dynamics (hmc.py:137-174) with velocity_verlet: returns q, p,
    logp, n_grad_evals, instability and the first / last Hamiltonian."""
    def ham(logp, p):
        return -logp + 0.5 * np.dot(p, p)
    q, p, logp, grad = q0, p0, logp0, grad0
    h0 = ham(logp0, p0)
    hmin = hmax = h0
    n_grad, instab, hcur = 0, False, h0
    for _ in range(n_step):
        p = p + 0.5 * dt * grad
        q = q + dt * p
        logp, grad = f(q)
        if math.isfinite(logp):
            p = p + 0.5 * dt * grad
        hcur = ham(logp, p)
        hmin, hmax = min(hmin, hcur), max(hmax, hcur)
        n_grad += 1
        instab = math.isinf(logp) or (hmax - hmin) > tol
        if instab:
            break
    return q, p, logp, n_grad, instab, h0, hcur


# -- extended-precision reference with a componentwise error bound -----------
#
# loglik_grad_ext / hessian_matvec_ext evaluate from the float64 inputs X,
# beta, v in np.longdouble (64-bit significand: 2^-11 of a float64 ulp), so
# their own rounding is negligible next to a float64 evaluation's.  Each also
# returns a bound: EPS times first-order sums over absolute values of what a
# float64 evaluation rounds, in the linear-time form above,
#   eta_i : a_i = (|X| |beta|)_i                (the product X~ beta)
#   h_i   : relative r_i = a_i + |eta_i - m| + 2 (the shift, exp)
#   H_k   : relative rho_k = risk(h r)_k / H_k + 1
#   c_k   : cumsum_l (rho_l + 1) / H_l + c_k
#   w_i   : cb h + c h (r + 1) + |w|,  grad: |X|^T (wb + |w|)
# and the same for the Hessian matvec.  Every sum is counted once; a test's
# tolerance is a stated multiple of the bound that covers the summation depth
# of the device's blocked sums.

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _ld(X):
    return X if X.dtype == LD else X.astype(LD)


def _abs(X):
    return abs(X)


def _location_ext(X, beta, n_event, start, end, drop=None, strict_end=False):
    """h, H and their error terms at beta.  drop: a row left out of every
    risk set (its hazard kept elsewhere); strict_end: a censored prefix is
    added only for end_k > n_event (a mutant of the device's end_k >= ne)."""
    Xl = _ld(X)
    beta = np.asarray(beta, dtype=np.float64).astype(LD)
    a = _abs(Xl) @ abs(beta)
    eta = Xl @ beta
    d = eta - np.max(eta)
    h = np.exp(d)
    r = a + abs(d) + 2
    hr = h.copy()
    if drop is not None:
        hr[drop] = 0.
    end_used = end
    if strict_end:
        end_used = np.where(end == n_event, n_event - 1, end)
    H = risk_sums(hr, n_event, start, end_used)
    HR = risk_sums(hr * r, n_event, start, end_used)
    return Xl, a, d, h, r, H, HR


def loglik_grad_ext(X, beta, n_event, start, end, n_app, drop=None,
                    strict_end=False, loglik_only=False):
    """(loglik, grad, loglik bound, grad bound); (-inf, None, 0, None) where
    some H_k == 0."""
    Xl, a, d, h, r, H, HR = _location_ext(X, beta, n_event, start, end, drop,
                                          strict_end)
    if np.any(H == 0.):
        return -math.inf, None, 0., None
    rho = HR / H + 1
    logH = np.log(H)
    terms = d[:n_event] - logH
    ll = np.sum(terms)
    llb = np.sum(a[:n_event] + abs(d[:n_event]) + rho + abs(logH)
                 + abs(terms))
    if loglik_only:
        return float(ll), None, float(EPS * llb), None
    inv = 1. / H
    c = np.cumsum(inv)
    cb = np.cumsum(inv * (rho + 1)) + c
    k = n_app - 1
    ch = c[k] * h
    w = -ch
    w[:n_event] += 1.
    wb = cb[k] * h + ch * (r + 1) + abs(w)
    grad = Xl.T @ w
    gb = _abs(Xl).T @ (wb + abs(w))
    return (float(ll), np.asarray(grad, dtype=np.float64), float(EPS * llb),
            np.asarray(EPS * gb, dtype=np.float64))


def hessian_matvec_ext(X, beta, v, n_event, start, end, n_app):
    """(Hessian matvec at beta applied to v, its componentwise bound)."""
    Xl, a, d, h, r, H, HR = _location_ext(X, beta, n_event, start, end)
    if np.any(H == 0.):
        raise ValueError("a risk-set sum is 0")
    rho = HR / H + 1
    inv = 1. / H
    c = np.cumsum(inv)
    cb = np.cumsum(inv * (rho + 1)) + c
    v = np.asarray(v, dtype=np.float64).astype(LD)
    u = Xl @ v
    ub = _abs(Xl) @ abs(v)
    au = abs(u)
    S = risk_sums(h * u, n_event, start, end)
    Sa = risk_sums(h * au, n_event, start, end)
    Sb = risk_sums(h * (au * (r + 1) + ub), n_event, start, end) + Sa
    z = inv * (inv * S)
    za = inv * inv * Sa
    zb = inv * inv * (Sb + abs(S) * (2 * rho + 3))
    cz = np.cumsum(z)
    cza = np.cumsum(za)
    czb = np.cumsum(zb) + cza
    k = n_app - 1
    ch = c[k] * h
    rr = ch * u - h * cz[k]
    rb = (cb[k] * h * au + ch * (r + 2) * au + ch * ub + czb[k] * h
          + h * cza[k] * (r + 1) + abs(rr))
    out = -(Xl.T @ rr)
    ob = _abs(Xl).T @ (rb + abs(rr))
    return (np.asarray(out, dtype=np.float64),
            np.asarray(EPS * ob, dtype=np.float64))


# The tests' tolerance in units of the bounds above: the sums are counted once
# in the bound; this covers the depth of the blocked sums (a chain of <= ~64
# roundings on any path).  The sequential float64 oracle stays within 4 x.
EDGE_TOL = 64.


def distance_in_tolerances(got, want):
    """max over loglik and the gradient of |got - want| / (EDGE_TOL x want's
    bound): got = (loglik, grad, ...), want = loglik_grad_ext's result.  A
    -inf loglik on one side only is infinitely far."""
    ll, grad = got[0], got[1]
    wl, wg, lb, gb = want
    if math.isinf(ll) or math.isinf(wl):
        return 0. if ll == wl else math.inf
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.abs(np.asarray(grad) - wg) / (EDGE_TOL * gb)
        r[(gb == 0) & (np.asarray(grad) == wg)] = 0.
        r[(gb == 0) & (np.asarray(grad) != wg)] = math.inf
        rl = abs(ll - wl) / (EDGE_TOL * lb) if lb > 0 else \
            (0. if ll == wl else math.inf)
    return float(max(rl, np.max(r)))
