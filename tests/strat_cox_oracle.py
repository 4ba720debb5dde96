"""NumPy oracle of the stratified Cox partial likelihood: every quantity is
the sum, over the strata, of tests/cox_oracle.py's unstratified one on that
stratum's rows alone (with that stratum's own shift max eta).  Also a
brute-force definition straight from the risk sets (an explicit n_event x n
membership matrix over all rows), a loop form of the preprocessing, and the
f(q) that drives cox_oracle.trajectory / nuts_oracle for a stratified model.

`strata` below is the list of per-stratum pieces made by `split`:
(row slice, n_event, start, end, n_app), the indices local to the stratum."""
import math

import numpy as np

import cox_oracle as co


def split(event_time, censoring_time, labels):
    """Rows in the stratified order -> the per-stratum pieces, each stratum's
    risk sets from the model's own unstratified cox_risk_sets."""
    from bayesbridge_amd.model import cox_risk_sets
    labels = np.asarray(labels)
    change = np.flatnonzero(labels[1:] != labels[:-1]) + 1
    bounds = np.concatenate(([0], change, [len(labels)]))
    pieces = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        ne, start, end, n_app = cox_risk_sets(event_time[a:b],
                                              censoring_time[a:b])
        pieces.append((slice(a, b), ne, start, end, n_app))
    return pieces


def global_risk_sets(pieces):
    """(stratum_ptr, stratum_n_event, start, end, last_set) in global
    indices, from the per-stratum pieces."""
    ptr, sne, start, end, last = [0], [], [], [], []
    e0 = 0
    for sl, ne, s, e, n_app in pieces:
        ptr.append(sl.stop)
        sne.append(ne)
        start.append(s + sl.start)
        end.append(e + sl.start)
        last.append(e0 + n_app - 1)
        e0 += ne
    return (np.array(ptr), np.array(sne), np.concatenate(start),
            np.concatenate(end), np.concatenate(last))


def loglik_grad(X, beta, pieces):
    ll, grad = 0., np.zeros(X.shape[1])
    for sl, *risk in pieces:
        l, g = co.loglik_grad(X[sl], beta, *risk)
        if g is None:
            return -math.inf, None
        ll += l
        grad += g
    return ll, grad


def hessian_matvec(X, beta, v, pieces, dtype=np.float64):
    out = np.zeros(X.shape[1])
    for sl, *risk in pieces:
        out += co.hessian_matvec(X[sl], beta, v, *risk, dtype=dtype)
    return out


def loglik_grad_ext(X, beta, pieces):
    """Sum over strata of cox_oracle.loglik_grad_ext and of its bounds (each
    rounding of a float64 evaluation lies in exactly one stratum's bound)."""
    ll, lb = 0., 0.
    grad, gb = np.zeros(X.shape[1], dtype=co.LD), np.zeros(X.shape[1])
    for sl, *risk in pieces:
        l, g, b, c = co.loglik_grad_ext(X[sl], beta, *risk)
        if g is None:
            return -math.inf, None, 0., None
        ll += co.LD(l)
        lb += b
        grad += g
        gb += c
    return float(ll), np.asarray(grad, dtype=np.float64), lb, gb


def hessian_matvec_ext(X, beta, v, pieces):
    out, ob = np.zeros(X.shape[1], dtype=co.LD), np.zeros(X.shape[1])
    for sl, *risk in pieces:
        o, b = co.hessian_matvec_ext(X[sl], beta, v, *risk)
        out += o
        ob += b
    return np.asarray(out, dtype=np.float64), ob


def loglik_grad_global_max(X, beta, pieces):
    """The mutant with ONE shift, max eta over all rows: what a stratified
    likelihood written against a global max computes."""
    eta = X @ beta
    m = np.max(eta)
    ll, grad = 0., np.zeros(X.shape[1])
    for sl, ne, start, end, n_app in pieces:
        d = eta[sl] - m
        h = np.exp(d)
        H = co.risk_sums(h, ne, start, end)
        if np.any(H == 0.):
            return -math.inf, None
        ll += np.sum(d[:ne] - np.log(H))
        w = -np.cumsum(1. / H)[n_app - 1] * h
        w[:ne] += 1.
        grad += X[sl].T @ w
    return ll, grad


def brute(X, beta, v, sptr, sne, start, end):
    """(loglik, grad, Hessian matvec) from the definition: risk set k is rows
    start[k] .. end[k]; event k is row sptr[s] + j of its stratum.  One
    membership matrix over all rows; the shift is the stratum's own max."""
    n = X.shape[0]
    ev_rows = np.concatenate([np.arange(sptr[s], sptr[s] + sne[s])
                              for s in range(len(sne))])
    eta = X @ beta
    shift = np.empty(n)
    for s in range(len(sne)):
        shift[sptr[s]:sptr[s + 1]] = np.max(eta[sptr[s]:sptr[s + 1]])
    d = eta - shift
    h = np.exp(d)
    mask = np.zeros((len(ev_rows), n))
    for k in range(len(ev_rows)):
        mask[k, start[k]:end[k] + 1] = 1.
    H = mask @ h
    if np.any(H == 0.):
        return -math.inf, None, None
    W = mask * h[None, :] / H[:, None]
    ind = np.zeros(n)
    ind[ev_rows] = 1.
    u = X @ v
    return (np.sum(d[ev_rows] - np.log(H)), X.T @ (ind - W.sum(axis=0)),
            -X.T @ (W.sum(axis=0) * u - W.T @ (W @ u)))


def precond_f(X, scale, prior_prec, pieces):
    """f(q) of reg_coef_sampler.py:259-279 on the stratified oracle."""
    def f(q):
        ll, g = loglik_grad(X, q * scale, pieces)
        logp = ll + np.sum(-prior_prec * q ** 2) / 2
        grad = None
        if math.isfinite(logp):
            grad = scale * g
            grad += -prior_prec * q
        return logp, grad
    return f


def preprocess_by_loops(event_time, censoring_time, labels):
    """The kept original indices in the stratified order, one stratum at a
    time: stable sorts, rows censored before the stratum's first event and
    strata without an event left out."""
    event_time = np.asarray(event_time, dtype=np.float64)
    censoring_time = np.asarray(censoring_time, dtype=np.float64)
    labels = np.asarray(labels)
    keep = []
    for lab in sorted(set(labels.tolist())):
        idx = [i for i in range(len(labels)) if labels[i] == lab]
        ev = [i for i in idx if event_time[i] < math.inf]
        if not ev:
            continue
        ev.sort(key=lambda i: event_time[i])                 # stable
        first = event_time[ev[0]]
        ce = [i for i in idx if not event_time[i] < math.inf
              and not censoring_time[i] < first]
        ce.sort(key=lambda i: -censoring_time[i])            # stable
        keep += ev + ce
    return np.array(keep, dtype=np.int64)


def make_strata(sizes, p, seed=0, only_events=(), all_tied=(), cens_frac=.5,
                shuffle=True):
    """Rows in the stratified order for strata of the given sizes (labels 0,
    1, ... in that order; `shuffle` permutes which size gets which label).
    Stratum index in `only_events`: no censored row; in `all_tied`: all its
    events at one time.  Times are rounded so that ties occur within and
    across strata; every censored row is censored at or after its stratum's
    first event.  Returns (event_time, censoring_time, labels, X, order):
    stratum `label` has sizes[order[label]] rows."""
    rs = np.random.RandomState(seed)
    sizes = np.asarray(sizes)
    special = {int(s): 'events' for s in only_events}
    special.update({int(s): 'tied' for s in all_tied})
    order = rs.permutation(len(sizes)) if shuffle else np.arange(len(sizes))
    et, ct, lab = [], [], []
    for label, s in enumerate(order):
        m = int(sizes[s])
        kind = special.get(int(s))
        n_cens = 0 if kind == 'events' else int(rs.binomial(m - 1, cens_frac))
        ne = m - n_cens
        t = np.sort(np.round(rs.exponential(1., ne) + .1, 1))
        if kind == 'tied':
            t[:] = t[0]
        c = np.sort(np.round(t[0] + rs.exponential(1., n_cens), 1))[::-1]
        et.append(np.concatenate((t, np.full(n_cens, np.inf))))
        ct.append(np.concatenate((np.full(ne, np.inf), c)))
        lab.append(np.full(m, label))
    et, ct, lab = (np.concatenate(a) for a in (et, ct, lab))
    return et, ct, lab, rs.randn(len(et), p), order
