"""Brute-force oracle of the Cox family's prediction, in
np.longdouble, from the definitions: explicit risk-set membership of every row
for every distinct event time, no scans, no shift (long double holds
exp(+-11000)), nothing imported from the package.

Rows are described by what was observed, not by the handle's index arrays:
  T        the event, censoring or competing time of the row
  status   1 event of interest, 0 censored, 2 competing event
  entry    the entry time (None: at risk from the start)
  weights  case weights (None: 1)
  strata   one label per row (None: one stratum)
  ties     'breslow' or 'efron'
Row i is in the risk set of an event at t of its stratum iff
entry_i < t <= T_i; with competing rows (Fine-Gray) a competing row with
T_i < t stays in it with weight G(t-) / G(T_i-), G the left-continuous
Kaplan-Meier estimate of the censoring survivor function on all rows.

For every distinct event time t of a stratum with d tied events:
  Breslow   H = sum_{i at risk} a_i m_i(t) exp(eta_i); every tied event k adds
            q_k = a_k / H
  Efron     R = the sum over the rows at risk that are not among the d events,
            G = the sum over the d events; event l = 0 .. d-1 adds
            q_l = 1 / (R + (1 - l/d) G)
Lambda0(t) = sum of q_k over the events with t_k <= t (of the stratum), and the
martingale residual of row i is
  a_i (delta_i - exp(eta_i) sum_k m_i(t_k) f_ik q_k),
f_ik = 1 - l/d for an event row i inside its own Efron tie group, else 1."""
import collections

import numpy as np

LD = np.longdouble

Rows = collections.namedtuple('Rows', 'T status entry weights strata ties')


def rows(event_time, censoring_time, competing_time=None, entry=None,
         weights=None, strata=None, ties='breslow'):
    """Rows from the package's (event, censoring[, competing]) time vectors
    (inf where the row had no such time)."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    T = np.minimum(event_time, censoring_time)
    status = np.where(np.isfinite(event_time), 1, 0)
    if competing_time is not None:
        competing_time = np.asarray(competing_time, dtype=np.float64)
        status = np.where(np.isfinite(competing_time), 2, status)
        T = np.minimum(T, competing_time)
    return Rows(T, status, None if entry is None else np.asarray(entry),
                None if weights is None else np.asarray(weights),
                None if strata is None else np.asarray(strata), ties)


def censoring_survivor_left(T, status):
    """s -> G(s-) = prod over the distinct censoring times c < s of
    (1 - m_c / Y(c)), m_c rows censored at c, Y(c) = #{i : T_i >= c}."""
    cs = np.unique(T[status == 0])
    factor = np.array([LD(1) - LD(np.sum((T == c) & (status == 0)))
                       / LD(np.sum(T >= c)) for c in cs], dtype=LD)

    def G(s):
        out = LD(1)
        for c, f in zip(cs, factor):
            if c < s:
                out = out * f
        return out
    return G


def _terms(eta, r, global_shift=False):
    """[(stratum code, t, [q of the d tied events], per-row membership weight
    (n,), the d event rows)] for every distinct event time of every stratum,
    and the per-row hazards exp(eta).  global_shift: the float64 mutant that
    forms exp(eta - max eta) with ONE max over all strata."""
    n = len(r.T)
    if global_shift:
        eta = np.asarray(eta, dtype=np.float64)
        e = np.exp(eta - np.max(eta))
        one = np.float64(1)
    else:
        e = np.exp(np.asarray(eta, dtype=LD))
        one = LD(1)
    a = np.ones(n, dtype=e.dtype) if r.weights is None \
        else np.asarray(r.weights, dtype=e.dtype)
    code = np.zeros(n, dtype=np.int64) if r.strata is None \
        else np.unique(r.strata, return_inverse=True)[1].ravel()
    entry = np.full(n, -np.inf) if r.entry is None else r.entry
    competing = np.any(r.status == 2)
    G = censoring_survivor_left(r.T, r.status) if competing else None
    out = []
    for s in np.unique(code):
        here = code == s
        for t in np.unique(r.T[here & (r.status == 1)]):
            member = np.where(here & (entry < t) & (r.T >= t), one, 0 * one)
            if competing:
                gt = G(t)
                for i in np.flatnonzero(here & (r.status == 2) & (r.T < t)):
                    member[i] = gt / G(r.T[i])
            ev = np.flatnonzero(here & (r.status == 1) & (r.T == t))
            d = len(ev)
            if r.ties == 'efron':
                in_group = np.zeros(n, dtype=bool)
                in_group[ev] = True
                R = np.sum((member * a * e)[~in_group])
                Gs = np.sum((member * a * e)[in_group])
                with np.errstate(divide='ignore'):
                    q = [one / (R + (one - one * l / d) * Gs)
                         for l in range(d)]
            else:
                H = np.sum(member * a * e)
                with np.errstate(divide='ignore'):
                    q = [a[k] / H for k in ev]
            out.append((s, t, q, member, ev))
    return out, e, a, code


def log_baseline_hazard(times, eta, r, global_shift=False):
    """log Lambda0 at `times`: (T,), or (n_strata, T) with strata (np.unique
    order of the labels); -inf before the first event."""
    times = np.asarray(times, dtype=np.float64)
    terms, e, a, code = _terms(eta, r, global_shift)
    strata = np.unique(code)
    out = np.empty((len(strata), len(times)), dtype=e.dtype)
    jumps = []                      # (stratum, t, the sum of the d values)
    for (s, t, q, _, _) in terms:
        tot = 0 * e[0]
        for x in q:
            tot = tot + x
        jumps.append((s, t, tot))
    for si, s in enumerate(strata):
        for j, tj in enumerate(times):
            tot = 0 * e[0]
            for (s2, t, jump) in jumps:
                if s2 == s and t <= tj:
                    tot = tot + jump
            with np.errstate(divide='ignore', invalid='ignore'):
                out[si, j] = np.log(tot)
    if global_shift:
        with np.errstate(invalid='ignore'):
            out = out - np.max(np.asarray(eta, dtype=np.float64))
    return out if r.strata is not None else out[0]


def residuals(eta, r):
    """The martingale residual of every row (a_i times it with weights)."""
    terms, e, a, code = _terms(eta, r)
    n = len(r.T)
    lam = np.zeros(n, dtype=LD)
    for (s, t, q, member, ev) in terms:
        d = len(ev)
        full = LD(0)
        for x in q:
            full = full + x
        add = member * full
        if r.ties == 'efron':
            own = LD(0)
            for l, x in enumerate(q):
                own = own + (LD(1) - LD(l) / d) * x
            add[ev] = member[ev] * own
        lam = lam + add
    delta = (r.status == 1).astype(LD)
    return a * (delta - e * lam)


def survival(eta, log_hazard, group=None):
    """(S (n_row, n_time, n_draw), mean, sd (n_row, n_time)) from eta
    (n_draw, n_row) and log_hazard (n_draw, n_group, n_time): S =
    exp(-exp(log_hazard + eta)), the population standard deviation."""
    eta = np.asarray(eta, dtype=LD)
    lh = np.asarray(log_hazard, dtype=LD)
    n_draw, n_row = eta.shape
    g = np.zeros(n_row, dtype=np.int64) if group is None else np.asarray(group)
    with np.errstate(over='ignore', invalid='ignore'):
        x = lh[:, g, :] + eta[:, :, None]          # (n_draw, n_row, n_time)
        S = np.moveaxis(np.exp(-np.exp(x)), 0, -1)
        mean = np.sum(S, axis=-1) / n_draw
        sd = np.sqrt(np.sum((S - mean[..., None]) ** 2, axis=-1) / n_draw)
    return S, mean, sd


def nelson_aalen(times, r):
    """sum over the distinct event times t <= each grid time of d / Y(t)
    (Efron: sum_l 1 / (Y - l)); with weights sum a_k / sum_{at risk} a_i.
    The independent formula of coef = 0: no hazards, no membership weights."""
    times = np.asarray(times, dtype=np.float64)
    a = np.ones(len(r.T), dtype=LD) if r.weights is None \
        else np.asarray(r.weights, dtype=LD)
    out = np.zeros(len(times), dtype=LD)
    for t in np.unique(r.T[r.status == 1]):
        Y = np.sum(a[r.T >= t])
        ev = np.flatnonzero((r.status == 1) & (r.T == t))
        if r.ties == 'efron':
            jump = sum(LD(1) / (Y - LD(l)) for l in range(len(ev)))
        else:
            jump = np.sum(a[ev]) / Y
        out[times >= t] += jump
    return out
