"""Sorted Cox test cases from explicit arguments (plain NumPy / SciPy).

cox_case(ne, n_cens, ...) returns rows already in the Cox model's order
(events by increasing time, then censored rows by decreasing censoring time)
with:
  * tied event times: a run of tied events across every chunk and tile
    boundary of the event segment's scans (csrc/cox.hip cuts each segment into
    SCAN_G chunks of ceil(len / SCAN_G) elements and scans a chunk in tiles of
    SCAN_TILE), read forward (the cumsums of 1/H) and reversed (the suffix sum
    of the hazards);
  * censoring times, some equal to event times; the largest equals the latest
    event time and, where the event times allow it, the next one is below it,
    so that some risk sets end exactly at the first censored row (end_k == ne);
  * optional "hot" rows at chosen indices: rows whose eta = x . beta is at the
    maximum, so that a risk set that loses one moves."""
import collections

import numpy as np
import scipy.sparse as sparse

SCAN_G = 256
SCAN_TILE = 2048

Case = collections.namedtuple(
    'Case', 'event_time censoring_time X beta hot n_event')


def chunk_len(length):
    return -(-length // SCAN_G)


def scan_starts(length):
    """Positions 0 < t < length where a chunk or a tile of a scan over
    `length` elements begins."""
    L = chunk_len(length)
    out = []
    for t0 in range(0, length, max(L, 1)):
        out.extend(t for t in range(t0, min(t0 + L, length), SCAN_TILE)
                   if t > 0)
    return np.array(out, dtype=np.int64)


def event_boundaries(ne):
    """Row indices i (0 < i < ne) where a chunk or tile of the event segment
    begins, in forward order (t = i) or in the reversed suffix scan
    (t = ne - i): a run across i covers rows i - 1 and i."""
    t = scan_starts(ne)
    return np.union1d(t, ne - t).astype(np.int64)


def tie_runs(ne, tie_width=2):
    """Row ranges [a, b) of tied events, one across each event boundary
    (rows b - tie_width .. b + tie_width - 1), overlapping runs merged.  Where
    chunks are short (ceil(ne / SCAN_G) <= 4 tie_width) merging would tie
    almost every event: there a boundary whose run would touch the previous
    run is left out, so that distinct event times remain between the runs."""
    merge = chunk_len(ne) > 4 * tie_width
    runs = []
    for b in event_boundaries(ne):
        a, e = max(b - tie_width, 0), min(b + tie_width, ne)
        if runs and a <= runs[-1][1]:
            if merge:
                runs[-1][1] = e
            continue
        runs.append([a, e])
    return runs


def _event_times(ne, rs, tie_width, n_random_runs):
    t = np.arange(1., ne + 1.)
    runs = [tuple(r) for r in tie_runs(ne, tie_width)]
    for _ in range(n_random_runs if ne > 1 else 0):
        a = rs.randint(0, ne - 1)
        runs.append((a, a + rs.randint(2, 7)))
    for a, b in sorted(runs):           # in order: every run stays sorted
        a, b = max(a, 0), min(b, ne)
        t[a:b] = t[a]
    return t


def _censoring_times(t, n_cens, rs, cens_ties):
    if n_cens == 0:
        return np.empty(0)
    below = t[t < t[-1]]                # below the latest tied run
    pool = below if len(below) else t
    c = pool[rs.randint(0, len(pool), n_cens)]
    if not cens_ties:
        c = c + .5
    else:                               # half tied to an event time
        jitter = rs.rand(n_cens) < .5
        c[jitter] += .5
    c[0] = t[-1]
    return np.sort(c)[::-1]


def _design(n, p, values, rs, density):
    if values == 'normal':
        return rs.randn(n, p)
    mask = sparse.random(n, p, density=density, format='csr', random_state=rs)
    if values == 'binary':
        mask.data[:] = 1.
    elif values == 'valued':
        mask.data[:] = rs.randn(mask.nnz)
    elif values == 'mixed':             # binary, the last tenth valued
        mask.data[:] = 1.
        n_val = max(1, p // 10)
        col = mask.indices >= p - n_val
        mask.data[col] = rs.randn(int(col.sum()))
    else:
        raise ValueError(values)
    return mask


def cox_case(ne, n_cens, p=6, values='normal', hot=(), tie_width=2,
             n_random_runs=4, cens_ties=True, beta_scale=.5, density=.2,
             seed=0):
    """`values`: 'normal' (dense ndarray), 'binary', 'valued' or 'mixed'
    (CSR).  `hot`: row indices set to the maximum eta (negative indices
    count from the end)."""
    if ne < 1 or n_cens < 0:
        raise ValueError("ne >= 1 and n_cens >= 0")
    rs = np.random.RandomState(seed)
    n = ne + n_cens
    t = _event_times(ne, rs, tie_width, n_random_runs)
    c = _censoring_times(t, n_cens, rs, cens_ties)
    event_time = np.concatenate((t, np.full(n_cens, np.inf)))
    censoring_time = np.concatenate((np.full(ne, np.inf), c))
    X = _design(n, p, values, rs, density)
    beta = rs.randn(p) * beta_scale
    hot = np.unique(np.asarray(hot, dtype=np.int64) % n) if len(hot) else \
        np.empty(0, dtype=np.int64)
    if len(hot):
        if values == 'normal':
            rest = np.setdiff1d(np.arange(n), hot)
            top = np.max(X[rest] @ beta) + 1. if len(rest) else 1.
            X[hot] = beta * (top / np.dot(beta, beta))
        else:
            X = X.tolil()
            for i in hot:
                X[i, :] = (beta > 0).astype(np.float64)
                if not np.any(beta > 0):
                    X[i, np.argmax(beta)] = 1.
            X = X.tocsr()
    return Case(event_time, censoring_time, X, beta, hot, ne)


def steep_case(ne, n_cens=1, ramp=70., bursts=4, burst_len=12, step=7.,
               seed=0):
    """Dense, two columns, beta = (1, .3), no ties: event eta falls by `ramp`
    over the events and, in `bursts` runs of `burst_len` rows placed across
    tile and chunk boundaries, by `step` from one row to the next.  1/H then
    spans more than e^ramp across the tiles of the cumsum of 1/H, and grows by
    far more than 2^53 within eight rows of each burst (one thread's elements
    of a scan tile).  Censored rows sit below every event."""
    rs = np.random.RandomState(seed)
    drop = np.full(ne, ramp / max(ne - 1, 1))
    L = chunk_len(ne)
    starts = [min(b * L + SCAN_TILE, ne - 1) for b in (3, SCAN_G // 2)]
    starts += [L * (SCAN_G // 3), ne - SCAN_TILE]
    for s in starts[:bursts]:
        a = max(1, s - burst_len // 2)
        drop[a:a + burst_len] = step
    drop[0] = 0.
    eta = -np.cumsum(drop)
    n = ne + n_cens
    X = np.column_stack((np.concatenate((eta, eta[-1] - 10. - rs.rand(n_cens))),
                         rs.randn(n)))
    event_time = np.concatenate((np.arange(1., ne + 1.),
                                 np.full(n_cens, np.inf)))
    censoring_time = np.concatenate((np.full(ne, np.inf),
                                     ne + 1. + np.sort(rs.rand(n_cens))[::-1]))
    return Case(event_time, censoring_time, X, np.array([1., .3]),
                np.empty(0, dtype=np.int64), ne)
