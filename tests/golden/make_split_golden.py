#!/usr/bin/env python3
"""
Generate tests/golden/simpls_split_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` and ``compute.efficient_corr``
(build container only; the reference is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_split_golden.py

The reference has no split-half for PLSRegression (pyls/types/regression.py:237-238), so the fixture is built from the
pieces it does have, arranged as BasePLS.split_half arranges them (pyls/base.py:366-397): ``simpls`` on all usable
rows of (X, Y[perm]) gives the x_weights W and y_loadings Q that stand in for U and V; per split the two halves'
cross-covariances are projected, D_h^T Q and D_h W, and ``efficient_corr`` compares the halves.  Stored: X, Y, the
masks of the observed data (S, n) and of P given permutations (P, S, n), the permutations (S, P), k, the per-split
correlations, their means over the splits and the resulting p-values -- data only.  All designs have T <= 11, where
the reference's rank-1 randomized SVD is exact.

A fixture is refused when the reference's values and the CPU oracle's (tests/regression_split_expect.py) differ by
more than 1e-10, or when any permuted mean lies within 1e-6 of the observed one: the pinned p-values are exact counts
that no implementation within the device tolerance of the means can move.
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

from regression_split_expect import split_expected, split_null, pvals_of, corr_err  # noqa: E402

AGREE = 1e-10
GAP = 1e-6


def halves(rs, S, n):
    out = np.zeros((S, n), dtype=bool)
    for s in range(n):
        out[rs.choice(S, size=(S + s % 2) // 2, replace=False), s] = True
    return out


def design(S, B, T, seed, nan_x=(), nan_y=(), C=0):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]          # separated leading eigenpairs, as the existing goldens
    if C:
        Y = Y[:, :, None] + 0.3 * rs.randn(S, T, C)
    for i in nan_x:
        X[i] = np.nan
    for i in nan_y:
        Y[i] = np.nan
    return X, Y, rs


def main():
    impl = dict(simpls=lambda x, y, c: simpls(x, y, c, seed=1234), efficient_corr=efficient_corr, get_mask=get_mask)
    cases = [('a', dict(S=90, B=400, T=7, seed=111), 6, 5, 8),
             ('nan', dict(S=80, B=200, T=5, seed=313, nan_x=(4, 31, 62), nan_y=(17, 40)), 5, 5, 7),
             ('y3d', dict(S=60, B=150, T=4, seed=515, C=3), 4, 5, 6)]
    for tag, kw, k, n, P in cases:
        X, Y, rs = design(**kw)
        S = kw['S']
        Y2 = Y if Y.ndim == 2 else np.mean(Y, axis=-1)
        masks = halves(rs, S, n)
        perms = np.stack([rs.permutation(S) for _ in range(P)], axis=1)
        perm_masks = np.stack([halves(rs, S, n) for _ in range(P)])
        got = split_expected(X, Y2, masks, k, **impl) + split_null(X, Y2, perm_masks, perms, k, **impl)
        want = split_expected(X, Y2, masks, k) + split_null(X, Y2, perm_masks, perms, k)
        errs = [corr_err(g, w) for g, w in zip(got, want)]
        print('simpls_split_{}: reference vs oracle {}'.format(tag, errs))
        if max(errs) > AGREE:
            raise SystemExit('simpls_split_{}: reference and oracle differ by more than {:g}: not written'.format(tag, AGREE))
        uc, vc, puc, pvc = got
        obs_u, obs_v = uc.mean(axis=-1), vc.mean(axis=-1)
        null_u, null_v = puc.mean(axis=-1).T, pvc.mean(axis=-1).T            # (k, P)
        gap = min(np.abs(null_u - obs_u[:, None]).min(), np.abs(null_v - obs_v[:, None]).min())
        print('simpls_split_{}: smallest |permuted mean - observed mean| {:.3g}'.format(tag, gap))
        if not gap > GAP:
            raise SystemExit('simpls_split_{}: a permuted mean within {:g} of the observed one: not written'.format(tag, GAP))
        np.savez_compressed(os.path.join(HERE, 'simpls_split_{}.npz'.format(tag)), X=X, Y=Y, splitsamples=masks,
                            permsamples=perms, perm_splitsamples=perm_masks, n_components=np.asarray(k),
                            ref_ucorr=uc, ref_vcorr=vc, ref_perm_ucorr=puc, ref_perm_vcorr=pvc,
                            ref_ucorr_mean=obs_u, ref_vcorr_mean=obs_v, ref_perm_ucorr_mean=null_u,
                            ref_perm_vcorr_mean=null_v, ref_ucorr_pvals=pvals_of(obs_u, null_u),
                            ref_vcorr_pvals=pvals_of(obs_v, null_v))


if __name__ == '__main__':
    main()
