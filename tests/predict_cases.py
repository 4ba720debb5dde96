"""The inputs of the prediction tests (tests/test_hip_predict.py), shared with
the CPU measurement of their tolerances (tests/test_predict_host_logic.py):
every case is a dict with the raw matrix, the oracle's X~, the draws and the
outcome arguments of one family."""
import numpy as np
import scipy.sparse as sparse

import predict_oracle as po

KINDS = ('tiled_binary', 'csr_valued', 'dense64', 'dense32')
ROW_EDGES = (1, 255, 256, 257, 65537)
DRAW_EDGES = (1, 2, 15, 16, 17, 33)
DRAW_BLOCKS = (1, 3, 17, 22)


def raw_matrix(kind, n, p, seed):
    """Columns with non-zero means: centring with the wrong means shows."""
    rs = np.random.RandomState(seed)
    if kind in ('tiled_binary', 'csr_valued'):
        if kind == 'tiled_binary':
            X = (rs.rand(n, p) < .2).astype(np.float64)
        else:
            X = (rs.rand(n, p) < .3) * (1. + .5 * rs.randn(n, p))
        if not X.any():
            X[0, 0] = 1.      # (a single row: keep one stored entry)
        return X
    X = .5 + rs.randn(n, p)
    if kind == 'dense32':
        X = X.astype(np.float32).astype(np.float64)
    return X


def oracle_matrix(kind, X, center, intercept):
    """X~ as the design of `kind` holds it: float32 storage keeps the
    CENTRED entries rounded to float32."""
    Xt = po.design_matrix(X, center, False)
    if kind == 'dense32':
        Xt = Xt.astype(np.float32).astype(np.float64)
    return po.design_matrix(Xt, None, intercept)


def problem(family, kind, n, p, S, seed, shifted=True, X=None):
    """One case: raw X (n, p), with `shifted` an intercept and centred
    columns.  The draws scatter around a coefficient vector that gives
    moderate linear predictors; the outcome is simulated from it."""
    rs = np.random.RandomState(seed + 7919)
    if X is None:
        X = raw_matrix(kind, n, p, seed)
    center = None
    if shifted:      # the column means as the design's constructor forms them
        center = X.mean(axis=0) if kind in ('dense64', 'dense32') \
            else np.asarray(csr(X).mean(axis=0)).ravel()
    Xt = oracle_matrix(kind, X, center, shifted)
    P = Xt.shape[1]
    beta = .4 * rs.randn(P) / np.sqrt(max(p, 1) / 4.)
    coef = beta[:, None] + .05 * rs.randn(P, S)
    eta = Xt @ beta
    case = {'family': family, 'kind': kind, 'X': X, 'center': center,
            'shifted': shifted, 'Xt': Xt, 'coef': coef, 'obs_prec': None,
            'n_trial': None, 'exposure': None, 'offset': None}
    if family == 'linear':
        case['y'] = eta + .7 * rs.randn(n)
        case['obs_prec'] = 1.5 + rs.rand(S)        # another one per draw
    elif family == 'logit':
        m = rs.randint(1, 4, n).astype(np.float64)
        case['n_trial'] = m
        case['y'] = rs.binomial(m.astype(int),
                                1 / (1 + np.exp(-eta))).astype(np.float64)
    else:
        case['exposure'] = .5 + 1.5 * rs.rand(n)
        case['offset'] = np.log(case['exposure'])
        case['y'] = rs.poisson(case['exposure']
                               * np.exp(np.clip(eta, -5, 3))
                               ).astype(np.float64)
    case['const'] = po.ll_const(family, case['y'], case['n_trial'])
    return case


def oracle(case, form, outcome=True, Xt=None, eta=None):
    """`form` (po.explicit or po.recurrence) on a case."""
    kw = {'obs_prec': case['obs_prec'], 'offset': case['offset']}
    if outcome:
        kw.update(y=case['y'], n_trial=case['n_trial'], const=case['const'])
    if eta is not None:
        kw['eta'] = eta
    return form(case['family'], case['Xt'] if Xt is None else Xt,
                case['coef'], **kw)


def subset(case, rows):
    """The rows of a case as new rows: X~ keeps the TRAINING means."""
    sub = dict(case)
    for key in ('X', 'Xt', 'y', 'n_trial', 'exposure', 'offset', 'const'):
        if case[key] is not None:
            sub[key] = case[key][rows]
    return sub


# ---- the cases of tests 1, 2, 3, 6 and 7 (what the tolerances are measured on)

def oracle_cases():
    """Test 1: every family on every kind of design, n = 2049, P = 40,
    S = 33, with intercept and centring and without."""
    for f, family in enumerate(po.FAMILIES):
        for k, kind in enumerate(KINDS):
            for shifted in (True, False):
                yield problem(family, kind, 2049, 40 - int(shifted), 33,
                              100 + 10 * f + k, shifted)


def row_edge_cases():
    """Test 2: n around the workgroup and one past 256 x 256; P = 3, S = 5."""
    for n in ROW_EDGES:
        yield problem('logit', 'csr_valued', n, 3, 5, 200 + n % 97, False)
    yield problem('logit', 'tiled_binary', 65537, 3, 5, 299, False)


def draw_edge_cases():
    """Test 3: S around the default block of 16 draws."""
    for S in DRAW_EDGES:
        yield problem('logit', 'dense64', 300, 4, S, 300 + S)


def draw_block_cases():
    """Test 3: S = 17 for the forced block sizes, every family."""
    for f, family in enumerate(po.FAMILIES):
        yield problem(family, 'dense64', 300, 4, 17, 350 + f)


def new_row_cases():
    """Test 6: (the training case, the rows that come back as X_new)."""
    for kind, seed in (('dense64', 400), ('csr_valued', 401)):
        rows = np.random.RandomState(seed).choice(2000, 300, replace=False)
        yield problem('logit', kind, 2000, 10, 20, seed), np.sort(rows)


def waic_cases():
    """Test 7: the training rows, n = 3000, S = 64."""
    yield problem('logit', 'tiled_binary', 3000, 20, 64, 500)
    yield problem('linear', 'dense64', 3000, 20, 64, 501)
    yield problem('poisson', 'csr_valued', 3000, 20, 64, 502)


def measured_cases():
    """Every (case, with an outcome) the tolerances are measured on."""
    for case in oracle_cases():
        yield case, True
    for case in row_edge_cases():
        yield case, True
    for case in draw_edge_cases():
        yield case, case['coef'].shape[1] > 1
    for case in draw_block_cases():
        yield case, True
    for case, rows in new_row_cases():
        yield subset(case, rows), True
    for case in waic_cases():
        yield case, True


def csr(X):
    X = sparse.csr_matrix(X)
    X.sort_indices()
    return X
