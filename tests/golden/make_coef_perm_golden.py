#!/usr/bin/env python3
"""
Generate tests/golden/simpls_coef_perm_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the
reference is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_coef_perm_golden.py

Inputs are those of the existing simpls_coef_<tag>.npz (X, Y, n_components, coef_components, aggfunc:
tests/golden/make_coef_golden.py); nothing of them is stored again.  What is new is ``permsamples`` (S, N_PERM), one
permutation of the rows of Y per column, drawn here from a fixed seed and stored.  Per permutation the reference's
``simpls`` fits c components on ``(Xc[m], Yc[perm][m])``, m = get_mask(Xc, Yc[perm]) (the centred X, the centred --
3-D: aggregated -- Y with its rows permuted, rows that are NaN throughout dropped); the coefficients are ``beta[1:]``
(regression.py:149-151).  The fixture holds the integer exceedance counts ``ref_count`` (B, T) =
#{p : |beta_p| >= |beta|} against the reference's own fit of the unpermuted pair, ``ref_max`` (T, N_PERM) =
max_f s_f |beta_p[f, t]| with s_f the standard deviation of feature f over the usable rows of X, and the two p-value
arrays built from them.  Data only.  All designs have T <= 11, where the reference's rank-1 randomized SVD is exact
(SURVEY.md section 0.3).  A fixture is refused unless
  * the CPU oracle (tests/regression_coef_perm_expect.py, from a k-component fit: the models are nested) gives the same
    counts and maxima within 1e-10;
  * the smallest relative gap | |beta_p| - |beta| | / |beta| over all (f, t, p) with beta != 0 exceeds 1e-8, in the
    reference and in the oracle: no count is decided by rounding, so every test compares the counts for equality.
The permutation seed is the first of SEEDS under which both hold.
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

from regression_coef_expect import max_rel                     # noqa: E402
from regression_coef_perm_expect import (centred, feature_scale, coef_perm_expected, pvals_of,   # noqa: E402
                                         min_rel_gap)

AGREE = 1e-10
MIN_GAP = 1e-8
N_PERM = 40
SEEDS = range(4321, 4341)


def reference_perms(Xc, Yc, perms, c):
    m = get_mask(Xc, Yc)
    obs = simpls(Xc[m], Yc[m], c, seed=1234)['beta'][1:]
    out = []
    for i in range(perms.shape[1]):
        Yp = Yc[perms[:, i]]
        m = get_mask(Xc, Yp)
        out.append(simpls(Xc[m], Yp[m], c, seed=1234)['beta'][1:])
    return obs, np.stack(out)


def main():
    for tag in ('a', 'nan', 'y3d'):
        g = dict(np.load(os.path.join(HERE, 'simpls_coef_{}.npz'.format(tag)), allow_pickle=False))
        k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
        Xc, Yc = centred(g['X'], g['Y'], aggfunc)
        S = len(Xc)
        for seed in SEEDS:
            rs = np.random.RandomState(seed)
            perms = np.stack([rs.permutation(S) for _ in range(N_PERM)], axis=1).astype(np.int32)
            obs, series = reference_perms(Xc, Yc, perms, c)
            got = pvals_of(obs, series, feature_scale(Xc))
            want = coef_perm_expected(g['X'], g['Y'], perms, k, c, aggfunc=aggfunc)
            gap = min(min_rel_gap(obs, series), min_rel_gap(want['coefs'], want['perms']))
            if gap > MIN_GAP:
                break
            print('simpls_coef_perm_{}: seed {} leaves a relative gap of {:.1e}: next seed'.format(tag, seed, gap))
        else:
            raise SystemExit('simpls_coef_perm_{}: no seed keeps the counts {:g} away from a tie'.format(tag, MIN_GAP))
        err = max_rel(got['coefs_max'], want['coefs_max'])
        same = np.array_equal(got['count'], want['count'])
        print('simpls_coef_perm_{}: seed {}, reference vs oracle: coefs_max {:.1e}, counts equal {}, smallest gap {:.1e} '
              '(n = {}, counts {} .. {})'.format(tag, seed, err, same, gap, N_PERM, got['count'].min(), got['count'].max()))
        if err > AGREE or not same:
            raise SystemExit('simpls_coef_perm_{}: reference and oracle differ: not written'.format(tag))
        np.savez_compressed(os.path.join(HERE, 'simpls_coef_perm_{}.npz'.format(tag)), permsamples=perms,
                            ref_count=got['count'].astype(np.int32), ref_max=got['coefs_max'],
                            ref_pvals=got['coefs_pvals'], ref_pvals_fwe=got['coefs_pvals_fwe'],
                            min_gap=np.float64(gap))


if __name__ == '__main__':
    main()
