#!/usr/bin/env python3
"""
Generate tests/golden/simpls_cv_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the
reference is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_cv_golden.py

The reference has no cross-validation for PLSRegression (pyls/types/regression.py:237-238), so the fixture is built
from the pieces it does have: for each split and each c = 1 .. k it fits ``simpls(X_tr, Y_tr, c, seed=...)`` on the
training rows and predicts the test rows with ``[1, X_te] @ out['beta']`` (the intercept row is part of beta,
regression.py:149-151).  Stored: X, Y, the masks (True = training row), k and the resulting Pearson r, R^2 and
squared-error sums -- data only.  All designs have T <= 11, where the reference's rank-1 randomized SVD is exact
(SURVEY.md section 0.3).  Before a fixture is written the same quantities are computed with the CPU oracle
(tests/regression_cv_expect.py); a fixture whose two versions differ by more than 1e-10 is refused.
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
from pyls.compute import efficient_corr                        # noqa: E402

from regression_cv_expect import cv_expected, abs_err, rel_err  # noqa: E402

AGREE = 1e-10


def design(S, B, T, seed, nan_x=(), nan_y=()):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]          # separated leading eigenpairs, as the existing goldens
    for i in nan_x:
        X[i] = np.nan
    for i in nan_y:
        Y[i] = np.nan
    return X, Y, rs


def splits(rs, S, n, test_size=0.25):
    out = np.ones((S, n), dtype=bool)
    for s in range(n):
        out[rs.choice(S, size=int(round(S * test_size)), replace=False), s] = False
    return out


def reference_cv(X, Y, masks, k):
    ok = get_mask(X, Y)
    T, n = Y.shape[1], masks.shape[1]
    r, r2, sse = np.zeros((T, k, n)), np.zeros((T, k, n)), np.zeros((T, k + 1, n))
    for s in range(n):
        tr, te = masks[:, s] & ok, ~masks[:, s] & ok
        ones = np.ones((te.sum(), 1))
        sse[:, 0, s] = np.sum((Y[te] - Y[tr].mean(axis=0)) ** 2, axis=0)
        for c in range(1, k + 1):
            out = simpls(X[tr], Y[tr], c, seed=1234)
            pred = np.column_stack([ones, X[te]]) @ out['beta']
            r[:, c - 1, s] = efficient_corr(Y[te], pred)
            res = np.sum((Y[te] - pred) ** 2, axis=0)
            r2[:, c - 1, s] = 1.0 - res / np.sum((Y[te] - Y[te].mean(axis=0)) ** 2, axis=0)
            sse[:, c, s] = res
    n_test = (~masks & ok[:, None]).sum(axis=0)
    return dict(r=r, r2=r2, sse=sse, mse=sse.sum(axis=0) / n_test[None, :])


def main():
    cases = [('a', dict(S=90, B=400, T=7, seed=101), 6, 8),
             ('b', dict(S=60, B=150, T=3, seed=202), 8, 8),
             ('nan', dict(S=80, B=200, T=5, seed=303, nan_x=(4, 31, 62), nan_y=(17,)), 5, 8)]
    for tag, kw, k, n in cases:
        X, Y, rs = design(**kw)
        masks = splits(rs, kw['S'], n)
        got = reference_cv(X, Y, masks, k)
        want = cv_expected(X, Y, masks, k)
        errs = dict(r=abs_err(got['r'], want['r']), r2=rel_err(got['r2'], want['r2']),
                    sse=rel_err(got['sse'], want['sse']), mse=rel_err(got['mse'], want['mse']))
        print('simpls_cv_{}: reference vs oracle {}'.format(tag, errs))
        if max(errs.values()) > AGREE:
            raise SystemExit('simpls_cv_{}: reference and oracle differ by more than {:g}: not written'.format(tag, AGREE))
        np.savez_compressed(os.path.join(HERE, 'simpls_cv_{}.npz'.format(tag)), X=X, Y=Y, cvsamples=masks,
                            n_components=np.asarray(k), ref_r=got['r'], ref_r2=got['r2'], ref_sse=got['sse'],
                            ref_mse=got['mse'])


if __name__ == '__main__':
    main()
