#!/usr/bin/env python3
"""
Generate tests/golden/simpls_cv_perm_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the
reference is imported the way make_golden.py imports it):

    python tests/golden/make_cv_perm_golden.py

The designs, masks and component counts are those of make_cv_golden.py (S = 90 / 60 / 80, T <= 11, 8 splits, NaN rows
in the third); 12 permutations of the rows are drawn from the same RandomState after the masks, with the project's own
generator (pypyls_amd.resampling.gen_permsamp).  For each permutation
that script's ``reference_cv`` runs on ``(X, Y[perm])`` under the same masks and the split-means are stored; the
p-values are the CPU oracle's (tests/regression_cv_perm_expect.py).  Data only.  A fixture is refused when reference
and oracle differ by more than 1e-10, when a value is not finite, or when an observed split-mean lies within 1e-4 of
a null value (absolute on r, relative to max(1, |v|) on R^2 and mse): a device error of 1e-5 cannot flip a p-value.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_cv_golden import design, splits, reference_cv                     # noqa: E402
from pypyls_amd.resampling import gen_permsamp                              # noqa: E402
from regression_cv_perm_expect import (cv_perm_expected, split_means, null_of, gaps, abs_err, rel_err)  # noqa: E402

AGREE, GAP, N_PERM = 1e-10, 1e-4, 12


def main():
    cases = [('a', dict(S=90, B=400, T=7, seed=101), 6, 8),
             ('b', dict(S=60, B=150, T=3, seed=202), 8, 8),
             ('nan', dict(S=80, B=200, T=5, seed=303, nan_x=(4, 31, 62), nan_y=(17,)), 5, 8)]
    for tag, kw, k, n in cases:
        X, Y, rs = design(**kw)
        masks = splits(rs, kw['S'], n)
        perms = gen_permsamp([kw['S']], 1, N_PERM, seed=rs, verbose=False)
        ref_obs = split_means(reference_cv(X, Y, masks, k))
        ref_null = null_of(reference_cv, X, Y, masks, perms, k)
        want = cv_perm_expected(X, Y, masks, perms, k)
        errs = {}
        for part, got, exp in (('obs', ref_obs, want['obs']), ('null', ref_null, want['null'])):
            errs[part] = max(abs_err(got['r'], exp['r']), rel_err(got['r2'], exp['r2']), rel_err(got['mse'], exp['mse']))
        gap = gaps(want['obs'], want['null'])
        finite = all(np.isfinite(v).all() for d in (ref_obs, ref_null) for v in d.values())
        print('simpls_cv_perm_{}: reference vs oracle {}  finite {}  gaps {}  r p-values {:.4f} .. {:.4f}'
              .format(tag, errs, finite, gap, want['pvals']['r'].min(), want['pvals']['r'].max()))
        if max(errs.values()) > AGREE or not finite:
            raise SystemExit('simpls_cv_perm_{}: reference and oracle differ by more than {:g}: not written'.format(tag, AGREE))
        if min(gap.values()) <= GAP:
            raise SystemExit('simpls_cv_perm_{}: an observed value within {:g} of a null value: not written'.format(tag, GAP))
        np.savez_compressed(os.path.join(HERE, 'simpls_cv_perm_{}.npz'.format(tag)), cvpermsamples=perms,
                            ref_obs_r=ref_obs['r'], ref_obs_r2=ref_obs['r2'], ref_obs_mse=ref_obs['mse'],
                            ref_perm_r=ref_null['r'], ref_perm_r2=ref_null['r2'], ref_perm_mse=ref_null['mse'],
                            pvals_r=want['pvals']['r'], pvals_r2=want['pvals']['r2'], pvals_mse=want['pvals']['mse'])


if __name__ == '__main__':
    main()
