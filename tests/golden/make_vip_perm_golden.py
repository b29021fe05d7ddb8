#!/usr/bin/env python3
"""
Generate tests/golden/simpls_vip_perm_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the
reference is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_vip_perm_golden.py

Inputs are those of the existing simpls_coef_<tag>.npz (X, Y, n_components, coef_components -- taken as the component
count c of the VIP scores --, aggfunc: tests/golden/make_coef_golden.py) and the permutations are the stored
``permsamples`` (S, 40) of simpls_coef_perm_<tag>.npz (tests/golden/make_coef_perm_golden.py); nothing of them is stored
again.  Per permutation the reference's ``simpls`` fits c components on ``(Xc[m], Yc[perm][m])``, m = get_mask(Xc,
Yc[perm]) (the centred X, the centred -- 3-D: aggregated -- Y with its rows permuted, rows that are NaN throughout
dropped); the VIP scores are the formula of MATLAB's ``plsregress`` documentation applied to its ``x_weights`` and
``y_loadings`` (tests/golden/make_vip_golden.py).  The fixture holds the integer exceedance counts ``ref_count`` (B,) =
#{p : vip_p >= vip} against the reference's own fit of the unpermuted pair, ``ref_max`` (n,) = max_f vip_p[f] and the
two p-value arrays built from them, and ``min_gap``.  Data only.  All designs have T <= 11, where the reference's rank-1
randomized SVD is exact.  A fixture is refused unless
  * the CPU oracle (tests/regression_vip_perm_expect.py, from a k-component fit: the models are nested) gives the same
    counts and, within 1e-10, the same maxima;
  * the smallest relative gap |vip_p - vip| / vip over all (f, p), and the same of the maxima against vip, exceeds 1e-8
    in the reference and in the oracle: no count is decided by rounding, so every test compares the counts for
    equality;
  * no permuted fit divides 0 by 0.
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
from regression_coef_perm_expect import centred                # noqa: E402
from regression_vip_expect import vip_of                       # noqa: E402
from regression_vip_perm_expect import vip_perms, vip_perm_expected, pvals_of, min_rel_gap   # noqa: E402

AGREE = 1e-10
MIN_GAP = 1e-8


def main():
    for tag in ('a', 'nan', 'y3d'):
        g = dict(np.load(os.path.join(HERE, 'simpls_coef_{}.npz'.format(tag)), allow_pickle=False))
        perms = np.load(os.path.join(HERE, 'simpls_coef_perm_{}.npz'.format(tag)), allow_pickle=False)['permsamples']
        k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
        Xc, Yc = centred(g['X'], g['Y'], aggfunc)
        m = get_mask(Xc, Yc)

        def fit(X, Y, n):
            return simpls(X, Y, n, seed=1234)
        obs = vip_of(fit(Xc[m], Yc[m], c), c)
        series = vip_perms(Xc, Yc, perms, c, c, simpls=fit, get_mask=get_mask)
        if not np.isfinite(series).all():
            raise SystemExit('simpls_vip_perm_{}: a permuted fit divides 0 by 0: not written'.format(tag))
        got = pvals_of(obs, series)
        want = vip_perm_expected(g['X'], g['Y'], perms, k, c, aggfunc=aggfunc)
        gaps = min_rel_gap(obs, series) + min_rel_gap(want['vip'], want['perms'])
        err = max(max_rel(got['vip_max'], want['vip_max']), max_rel(obs, want['vip']))
        same = np.array_equal(got['count'], want['count']) and np.array_equal(got['fwe_count'], want['fwe_count'])
        print('simpls_vip_perm_{}: reference vs oracle {:.1e}, counts equal {}; per-feature gap {:.1e} / {:.1e}, gap vs '
              'maxima {:.1e} / {:.1e}; counts {} .. {}, fwe counts {} .. {}, NaN rows {}  (S x B = {} x {}, c = {})'.format(
                  tag, err, same, gaps[0], gaps[2], gaps[1], gaps[3], got['count'].min(), got['count'].max(),
                  got['fwe_count'].min(), got['fwe_count'].max(), int((~m).sum()), Xc.shape[0], Xc.shape[1], c))
        if min(gaps) <= MIN_GAP:
            raise SystemExit('simpls_vip_perm_{}: a count is within {:g} of a tie: not written'.format(tag, MIN_GAP))
        if err > AGREE or not same:
            raise SystemExit('simpls_vip_perm_{}: reference and oracle differ: not written'.format(tag))
        np.savez_compressed(os.path.join(HERE, 'simpls_vip_perm_{}.npz'.format(tag)),
                            ref_count=got['count'].astype(np.int32), ref_max=got['vip_max'],
                            ref_pvals=got['vip_pvals'], ref_pvals_fwe=got['vip_pvals_fwe'],
                            min_gap=np.float64(min(gaps)))


if __name__ == '__main__':
    main()
