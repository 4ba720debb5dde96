"""Writes tests/golden/seg_scan_parent_bits.npz: what the handles whose
likelihoods run a blocked two-pass scan -- the conditional Poisson model
(csrc/cpoisson.hip), the stratified Cox model (csrc/cox_strat.hpp) and the five
handles that launch cox_scan_out_kernel (plain, Efron, interval, weighted,
Fine-Gray) -- computed on an MI355X in the build of the commit BEFORE their
three copies of the block scan were folded onto csrc/seg_scan.hpp: the
log-likelihood and gradient at a seeded beta, one Hessian-vector product after
set_location there, and the end state of a 3-step device trajectory, on a
seeded dense float64 design with 5 columns and no intercept.
tests/test_hip_seg_scan_bits.py imports `compute` and compares bit for bit.

    python tests/golden/make_seg_scan_bits.py OUT.npz     (needs a GPU)

To write the fixture again, run this file from this tree with the package of
the parent commit's build first on PYTHONPATH.

The stratum layouts are those of tests/test_hip_cpoisson.py and
tests/test_hip_strat_cox.py, imported.  Every value is kept as its uint64 bit
pattern; they are scalars and 5-vectors."""
import os
import sys
import warnings

import numpy as np

TESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

P = 5                                  # columns of the design
COX_KINDS = ('plain', 'efron', 'interval', 'weighted', 'finegray')
COX_ROWS = (5, 257, 70144)             # 70 144 = 256 x 274
TWO_TILES = 600064                     # 256 x 2344: chunks of two tiles
CPOISSON = ('small', 'pairs', 'seams', 'tiles', 'two_three', 'shift800')
STRAT = ('seams', 'tiles', 'tiny')


def cases():
    """Every case as (family, name or row count).  At TWO_TILES rows: the
    plain handle, and the Fine-Gray one, whose second scan is the rev == 2
    mirror (cox_finegray.hip's half_rev)."""
    return ([('cpoisson', name) for name in CPOISSON]
            + [('strat', name) for name in STRAT]
            + [(kind, n) for kind in COX_KINDS for n in COX_ROWS]
            + [('plain', TWO_TILES), ('finegray', TWO_TILES)])


def bits(a):
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    return a.view(np.uint64).copy()


def _cpoisson_model(name):
    """(model, {scale name: beta}).  Coefficients at scales 0.3 and 2; in
    'shift800' one stratum's linear predictor lies 800 below another's."""
    import test_hip_cpoisson as tcp
    from bayesbridge_amd import RegressionModel
    seed = CPOISSON.index(name)
    rs = np.random.RandomState(seed)
    if name == 'shift800':
        sizes = [300, 500, 200]
        lab = np.repeat(np.arange(3), sizes)
        n = len(lab)
        X = np.column_stack((rs.randn(n, P - 1), (lab == 1) * 1.))
        dsn = tcp._device_design('dense64', X, False)[0]
        sptr = tcp.cpo.stratum_ptr_of(sizes)
        y = tcp._counts(rs, sptr, np.full(n, 1.5))
        model = RegressionModel((y, rs.uniform(.5, 2., n), lab), dsn,
                                'poisson')
        beta = np.append(rs.randn(P - 1) * .3, 800.)
        eta = X.dot(beta)
        assert eta[lab == 1].min() - eta[lab == 0].max() > 780
        return model, {'shift': beta}
    sizes = [2, 3] if name == 'two_three' else tcp.LAYOUTS[name]()
    model = tcp._data('dense64', sizes, P, seed=seed)[0]
    return model, {'s0.3': rs.randn(P) * .3, 's2': rs.randn(P) * 2.}


def _strat_model(name):
    import strat_cox_oracle as so
    import test_hip_strat_cox as tsc
    seed = STRAT.index(name)
    if name == 'tiny':
        # fewer than 256 rows and fewer than 64 events: one chunk per element
        et, ct, lab = so.make_strata([7, 40, 90, 3, 60], 1, seed=7,
                                     cens_frac=.8, shuffle=False)[:3]
        assert len(et) < 256 and np.sum(np.isfinite(et)) < 64
    else:
        et, ct, lab = tsc._case(name)
    model = tsc._model('dense64', et, ct, lab, P, seed=seed)[0]
    return model, {'s0.3': np.random.RandomState(seed).randn(P) * .3}


def _cox_data(kind, n):
    """n rows that the model's preprocessing sorts but does not drop: the
    earliest time is an event.  Times on a grid of 0.01, so that they tie.
    Returns (event_time, censoring_time, X, the model's keywords, beta)."""
    from bayesbridge_amd.model import _n_risk_sets
    rs = np.random.RandomState([COX_KINDS.index(kind), n])
    X = rs.randn(n, P)
    t = 1. + np.round(rs.exponential(np.exp(-.3 * X[:, 0])), 2)
    status = rs.choice(3, n, p=[.5, .3, .2])   # event, censored, competing
    t[0], status[0] = .5, 0
    if kind != 'finegray':
        status[status == 2] = 0
    inf = np.inf
    et, ct = np.where(status == 0, t, inf), np.where(status == 1, t, inf)
    kw = {}
    if kind == 'efron':
        kw['ties'] = 'efron'
    elif kind == 'weighted':
        kw['weights'] = np.exp(rs.randn(n) * .5)
    elif kind == 'finegray':
        kw['competing_time'] = np.where(status == 2, t, inf)
    elif kind == 'interval':
        # delayed entry for half of the rows, unless no event falls inside
        entry = np.where(rs.rand(n) < .5, rs.rand(n) * t, -inf)
        p, q = _n_risk_sets(entry, t, et)
        kw['entry_time'] = np.where(p > q, entry, -inf)
    return et, ct, X, kw, rs.randn(P) * .3


def _cox_model(kind, n):
    from bayesbridge_amd import RegressionModel
    et, ct, X, kw, beta = _cox_data(kind, n)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = RegressionModel((et, ct), X, 'cox', **kw)
    assert model.n_obs == n and model.n_pred == P, (kind, n, model.n_obs)
    return model, {'s0.3': beta}


def compute(case):
    """{name: uint64 array} of one of cases()."""
    family, which = case
    if family == 'cpoisson':
        model, betas = _cpoisson_model(which)
    elif family == 'strat':
        model, betas = _strat_model(which)
    else:
        model, betas = _cox_model(family, which)
    n = model.n_obs
    rs = np.random.RandomState(5)
    out = {}
    for tag, beta in betas.items():
        ll, grad = model.compute_loglik_and_gradient(beta)
        assert np.isfinite(ll), (case, tag, ll)
        out[tag + '_loglik'], out[tag + '_grad'] = bits(ll), bits(grad)
        out[tag + '_hessian_matvec'] = bits(
            model.get_hessian_matvec_operator(beta)(rs.randn(P)))
        scale, pp = np.exp(rs.randn(P) * .3) * .3, np.ones(P)
        q0, p0 = beta / scale, rs.randn(P)
        logp0 = ll - .5 * np.sum(pp * q0 ** 2)
        grad0 = scale * grad - pp * q0
        # (the curvature grows with n: a step well inside the stability limit)
        tr = model.hmc_trajectory(.02 / np.sqrt(n), 3, scale, pp, q0, p0,
                                  logp0, grad0, hamiltonian_tol=1e300)
        assert tr['n_steps'] == 3 and tr['grad'] is not None, (case, tag, tr)
        out.update({tag + '_traj_q': bits(tr['q']),
                    tag + '_traj_p': bits(tr['p']),
                    tag + '_traj_logp': bits(tr['logp']),
                    tag + '_traj_grad': bits(tr['grad'])})
    return out


def key(case, name):
    return '%s_%s_%s' % (case[0], case[1], name)


if __name__ == "__main__":
    # the package first on PYTHONPATH, before the tests' conftest puts this
    # tree's in front of it
    import bayesbridge_amd
    print('package', os.path.dirname(bayesbridge_amd.__file__))
    out = {}
    for case in cases():
        for name, val in compute(case).items():
            out[key(case, name)] = val
        print(case, 'done', flush=True)
    np.savez(sys.argv[1], **out)
    print('wrote', sys.argv[1], len(out), 'arrays',
          sum(v.size for v in out.values()), 'doubles')
