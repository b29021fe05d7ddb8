#!/usr/bin/env python3
"""
Generate tests/golden/simpls_da_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the reference
is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_da_golden.py

The reference has no discriminant analysis, so the fixture is built from the pieces it does have: for each split and
each c = 1 .. k it fits ``simpls(X_tr, onehot_tr, c, seed=...)`` on the training rows, predicts the indicators of the test
rows with ``[1, X_te] @ out['beta']`` (the intercept row is part of beta, regression.py:149-151) and takes the class
from their argmax.  Stored: X, y, the masks (True = training row), k, the resulting confusion counts
(G, G, k, n) and the smallest gap between the two largest predicted indicators -- data only.  All designs have G <= 11,
where the reference's rank-1 randomized SVD is exact.  Before a fixture is written the same
counts are computed with the CPU oracle (tests/discriminant_expect.py); a fixture whose two versions differ in ANY cell,
or whose margin (either version's) is below 1e-6, is refused: choose another seed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden  # noqa: E402,F401  (puts the h5py stub and the reference on sys.path)
from pyls.types.regression import simpls, get_mask            # noqa: E402

from discriminant_expect import da_expected, one_hot, MARGIN  # noqa: E402


def design(S, B, sizes, seed, shift=0.45, nan_x=()):
    """Class means shifted on about a tenth of the features, so that accuracy is neither 1 nor chance; rows in random
    order (the labels are NOT sorted)."""
    rs = np.random.RandomState(seed)
    assert sum(sizes) == S
    y = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    X = rs.randn(S, B)
    nf = max(2, B // 10)
    means = shift * rs.randn(len(sizes), nf)
    X[:, :nf] += means[y]
    for i in nan_x:
        X[i] = np.nan
    return X, y, rs


def splits(rs, y, n, test_size=0.25):
    """Per class, round(n_g test_size) test rows chosen at random."""
    out = np.ones((len(y), n), dtype=bool)
    for s in range(n):
        for g in np.unique(y):
            rows = np.flatnonzero(y == g)
            out[rs.choice(rows, size=int(round(len(rows) * test_size)), replace=False), s] = False
    return out


def reference_da(X, y, masks, k):
    G = int(y.max()) + 1
    Y = one_hot(y, G)
    ok = get_mask(X, Y)
    n = masks.shape[1]
    conf = np.zeros((G, G, k, n), dtype=np.int64)
    margin = np.inf
    for s in range(n):
        tr, te = masks[:, s] & ok, ~masks[:, s] & ok
        ones = np.ones((te.sum(), 1))
        for c in range(1, k + 1):
            out = simpls(X[tr], Y[tr], c, seed=1234)
            pred = np.column_stack([ones, X[te]]) @ out['beta']
            np.add.at(conf[:, :, c - 1, s], (y[te], np.argmax(pred, axis=1)), 1)
            top = np.sort(pred, axis=1)[:, -2:]
            margin = min(margin, float(np.min(top[:, 1] - top[:, 0])))
    return dict(confusion=conf, margin=margin)


def main():
    cases = [('a', dict(S=90, B=400, sizes=(30, 30, 30), seed=11), 6, 8),
             ('b', dict(S=60, B=150, sizes=(33, 27), seed=22), 8, 8),
             ('nan', dict(S=70, B=130, sizes=(30, 20, 12, 8), seed=33, nan_x=(6, 29, 51)), 5, 8)]
    for tag, kw, k, n in cases:
        X, y, rs = design(**kw)
        masks = splits(rs, y, n)
        got = reference_da(X, y, masks, k)
        want = da_expected(X, y, masks, k)
        differ = int(np.sum(got['confusion'] != want['confusion']))
        acc = np.einsum('ggcs->c', got['confusion']) / got['confusion'].sum(axis=(0, 1, 3))
        print('simpls_da_{}: cells differing from the oracle {}; margin reference {:.3e} oracle {:.3e}; pooled accuracy '
              'per c {}'.format(tag, differ, got['margin'], want['margin'], np.round(acc, 3).tolist()))
        if differ or min(got['margin'], want['margin']) < MARGIN:
            raise SystemExit('simpls_da_{}: reference and oracle differ, or the margin is below {:g}: not written'
                             .format(tag, MARGIN))
        np.savez_compressed(os.path.join(HERE, 'simpls_da_{}.npz'.format(tag)), X=X, y=y, cvsamples=masks,
                            n_components=np.asarray(k), ref_confusion=got['confusion'], ref_margin=np.asarray(got['margin']))


if __name__ == '__main__':
    main()
