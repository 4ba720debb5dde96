"""Writes tests/golden/latent_rows_parent_bits.npz: what the chains of the
latent families (probit, student_t, censored) held on an MI355X in the build
of the commit BEFORE their three row kernels were folded onto
csrc/latent_rows.hpp -- latent, zbase, coef, the scalar obs_prec where the
model has one, loglik and logp, after create (the reserved stream index), after
set_state with a seeded coefficient (the refresh path), after init_obs_prec,
after each of three 'cholesky' iterations and, at the two smallest and the
largest row count, after each of three 'cg' iterations of a second chain; for
Student-t also after set_df(7.) -- on a seeded dense float64 design with 5
columns, at the row counts where the row kernel changes path.
tests/test_hip_latent_rows_bits.py imports `compute` and compares bit for bit.

    python tests/golden/make_latent_rows_bits.py OUT.npz     (needs a GPU)

To write the fixture again, run this file from this tree with the package of
the parent commit's build first on PYTHONPATH: the row counts come from this
tree's headers (the parent had the same WAVE and ROW_GRID).

Every value is kept as its uint64 bit pattern.  A committed file stays under
1 MiB and the latents of the largest case are 4 MB per state, so a vector of
more than LONG entries is kept as its first and last EDGE entries and the four
words of the SHA-256 of all its bytes: equal digests are equal bits."""
import hashlib
import os
import re
import sys

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..',
                    'bayes-bridge_amd', 'csrc')
FAMILIES = ('probit', 'student_t', 'censored')
P = 5                    # columns of the design: the intercept and 4 more
LONG, EDGE = 4096, 256


def _constant(name, src):
    text = open(os.path.join(CSRC, src)).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))


def rows():
    """The row counts, from the headers: one lane per row on at most ROW_GRID
    blocks of 256 (four waves), a block total per block and a fold of the
    blocks' sums; from ROW_GRID x 256 rows on a lane takes a second row."""
    wave = _constant('WAVE', 'common.hpp')
    row_grid = _constant('ROW_GRID', 'chain.hpp')
    return (1, wave - 1, wave + 1, 255, 257, row_grid * 256 + 3)


def cg_rows():
    """... of which the 'cg' iterations run at the two smallest and the
    largest."""
    return rows()[:2] + rows()[-1:]


def bits(a):
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    if a.size <= LONG:
        return a.view(np.uint64).copy()
    digest = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint64)
    return np.concatenate([a[:EDGE].view(np.uint64), a[-EDGE:].view(np.uint64),
                           digest])


def _chain(family, n, seed):
    """A chain of `family` on n seeded rows (the same rows for every seed)."""
    from bayesbridge_amd import (HipDenseDesignMatrix, HipGibbsChain,
                                 design_matrix)
    rng = np.random.default_rng([FAMILIES.index(family), n])
    X = rng.normal(size=(n, P - 1))
    # (the design classes drop columns that are constant over the rows, and
    # every column of a single row is: the one-row case keeps its 5 columns, as
    # in make_glm_rows_bits.py)
    keep = design_matrix.remove_intercept_indicator
    if n == 1:
        design_matrix.remove_intercept_indicator = lambda X: X
    try:
        dsn = HipDenseDesignMatrix(X, add_intercept=True,
                                   center_predictor=True,
                                   storage_dtype='float64')
    finally:
        design_matrix.remove_intercept_indicator = keep
    assert dsn.shape == (n, P)
    eta = .2 + X.dot(rng.normal(size=P - 1) * .5)
    more = {}
    if family == 'probit':
        y = (eta + rng.normal(size=n) > 0.).astype(np.float64)
    elif family == 'student_t':
        y = eta + .7 * rng.standard_t(4., size=n)
    else:
        # all three statuses from three rows on; a single row is censored, so
        # that it draws
        y = eta + .7 * rng.normal(size=n)
        more['status'] = ((np.arange(n) + 1) % 3).astype(np.uint8)
    chain = HipGibbsChain(dsn, family, y, sd_unshrunk=[2.], slab_size=2.,
                          seed=seed, **more)
    coef = rng.normal(size=P) * .3
    return chain, coef


def _state(chain, out, tag):
    coef, obs_prec, _, _ = chain.get_state()
    loglik, logp = chain.logp()
    out[tag + '_latent'] = bits(chain.get_latent())
    out[tag + '_zbase'] = bits(chain.get_zbase())
    out[tag + '_coef'] = bits(coef)
    if obs_prec is not None:
        out[tag + '_obs_prec'] = bits(obs_prec)
    out[tag + '_loglik'] = bits(loglik)
    out[tag + '_logp'] = bits(logp)


def compute(family, n):
    """{name: uint64 array} of family's chains on n rows."""
    out = {}
    samplers = ('cholesky', 'cg') if n in cg_rows() else ('cholesky',)
    for sampler in samplers:
        chain, coef = _chain(family, n, seed=11)
        first = sampler == 'cholesky'
        if first:
            _state(chain, out, 'create')
        chain.set_state(coef=coef, global_scale=.5)
        if first:
            _state(chain, out, 'set_state')
        chain.init_obs_prec()
        if first:
            _state(chain, out, 'init')
        chain.set_coef_sampler(sampler)
        for k in range(3):
            chain.run(1)
            _state(chain, out, '%s%d' % (sampler, k))
        if first and family == 'student_t':
            chain.set_df(7.)
            _state(chain, out, 'df7')
        chain.close()
    return out


if __name__ == "__main__":
    out = {}
    for family in FAMILIES:
        for n in rows():
            for key, val in compute(family, n).items():
                if key.endswith(('_loglik', '_logp')):
                    assert np.isfinite(val.view(np.float64)).all(), (family, n,
                                                                     key)
                out['%s_%d_%s' % (family, n, key)] = val
    np.savez(sys.argv[1], **out)
    print('wrote', sys.argv[1], len(out), 'arrays',
          sum(v.size for v in out.values()), 'words')
