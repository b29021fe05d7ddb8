#!/usr/bin/env python3
"""
Generate tests/golden/simpls_coef_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the reference
is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_coef_golden.py

The reference's ``simpls`` computes the model coefficients as ``beta`` (pyls/types/regression.py:149-151: row 0 the
intercept, rows 1 .. B the coefficients) and its PLSResults drop them.  The fixture holds ``simpls(...)['beta']`` of the
c-component fit on the original rows (raw X, Y: simpls centres them itself, so row 0 is the intercept of the raw data)
and, per bootstrap sample, of the c-component fit on what PLSRegression._single_boot fits (regression.py:279-327: the
centred X, the centred Y -- for 3-D Y the original Y aggregated over the resampled third axis --, all-NaN rows
dropped), summed: sum of beta and of beta^2.  Data only.  All designs have T <= 11, where the reference's rank-1
randomized SVD is exact.  Before a fixture is written the same quantities are computed with
the CPU oracle (tests/regression_coef_expect.py, from a k-component fit: the models are nested); a fixture whose two
versions differ by more than 1e-10 is refused.
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

from regression_coef_expect import coef_expected, max_rel      # noqa: E402

AGREE = 1e-10
_AGG = dict(mean=np.mean, median=np.median, sum=np.sum)


def design(S, B, T, seed, C=0, nan_x=(), nan_y=()):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]          # separated leading eigenpairs, as the existing goldens
    if C:
        Y = Y[..., None] + 0.3 * rs.randn(S, T, C)
    for i in nan_x:
        X[i] = np.nan
    for i in nan_y:
        Y[i] = np.nan
    return X, Y, rs


def reference_coefs(X, Y, subj, third, c, aggfunc):
    agg = _AGG[aggfunc]
    Y_agg = agg(Y, axis=-1) if Y.ndim == 3 else Y
    ok = get_mask(X, Y_agg)
    beta = simpls(X[ok], Y_agg[ok], c, seed=1234)['beta']
    Xc = X - np.nanmean(X, axis=0, keepdims=True)
    Yc = Y_agg - np.nanmean(Y_agg, axis=0, keepdims=True)
    bsum, bsq = np.zeros_like(beta[1:]), np.zeros_like(beta[1:])
    for i in range(subj.shape[1]):
        inds = subj[:, i]
        Xi = Xc[inds]
        Yi = agg(Y[..., third[:, i]], axis=-1)[inds] if Y.ndim == 3 else Yc[inds]
        m = get_mask(Xi, Yi)
        b = simpls(Xi[m], Yi[m], c, seed=1234)['beta'][1:]
        bsum += b
        bsq += b ** 2
    return dict(coefs=beta[1:], intercept=beta[0], bsum=bsum, bsq=bsq)


def main():
    cases = [('a', dict(S=60, B=150, T=4, seed=11), 6, 3, 40, 'mean'),
             ('nan', dict(S=70, B=120, T=3, seed=22, nan_x=(5, 40), nan_y=(17, 63)), 5, 5, 32, 'mean'),
             ('y3d', dict(S=50, B=100, T=3, seed=33, C=5), 4, 2, 32, 'median')]
    for tag, kw, k, c, n, aggfunc in cases:
        X, Y, rs = design(**kw)
        S = kw['S']
        subj = rs.randint(0, S, size=(S, n))
        third = rs.randint(0, Y.shape[-1], size=(Y.shape[-1], n)) if Y.ndim == 3 else None
        got = reference_coefs(X, Y, subj, third, c, aggfunc)
        want = coef_expected(X, Y, subj, k, c, aggfunc=aggfunc, third=third)
        errs = {key: max_rel(got[key], want[key]) for key in ('coefs', 'intercept', 'bsum', 'bsq')}
        print('simpls_coef_{}: reference vs oracle {}  (oracle max |coefs_normed| {:.2f})'.format(
            tag, {key: '{:.1e}'.format(v) for key, v in errs.items()}, np.max(np.abs(want['normed']))))
        if max(errs.values()) > AGREE:
            raise SystemExit('simpls_coef_{}: reference and oracle differ by more than {:g}: not written'.format(tag, AGREE))
        extra = dict(third=third) if third is not None else {}
        np.savez_compressed(os.path.join(HERE, 'simpls_coef_{}.npz'.format(tag)), X=X, Y=Y, bootsamples=subj,
                            n_components=np.asarray(k), coef_components=np.asarray(c), aggfunc=np.asarray(aggfunc),
                            ref_coefs=got['coefs'], ref_intercept=got['intercept'], ref_bsum=got['bsum'],
                            ref_bsq=got['bsq'], **extra)


if __name__ == '__main__':
    main()
