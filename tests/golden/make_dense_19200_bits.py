"""Writes tests/golden/dense_19200_parent_bits.npz: dot, Tdot and gram_matvec
of a seeded 48 x 19 200 dense design (the widest the single-pass X~ v kernel
takes), f32 and f64 storage, as the build of the commit BEFORE wide designs
were added computed them on an MI355X.  tests/test_hip_wide_dense.py imports
`compute` and compares bit for bit.

    python tests/golden/make_dense_19200_bits.py OUT.npz     (needs a GPU)"""
import sys

import numpy as np


def compute(storage):
    from bayesbridge_amd import HipDenseDesignMatrix
    rng = np.random.default_rng(19200)
    n, p = 48, 19199
    X = rng.normal(size=(n, p)).astype(np.float32)
    d = HipDenseDesignMatrix(X, center_predictor=True, add_intercept=True,
                             storage_dtype=storage)
    assert d.shape == (n, 19200)
    v, w = rng.normal(size=p + 1), rng.normal(size=n)
    omega = rng.gamma(2., .15, n)
    return {'dot': d.dot(v), 'tdot': d.Tdot(w),
            'gram_matvec': d.gram_matvec(omega, v)}


if __name__ == "__main__":
    out = {}
    for storage in ('float32', 'float64'):
        for key, val in compute(storage).items():
            out['%s_%s' % (storage, key)] = val
    np.savez(sys.argv[1], **out)
