#!/usr/bin/env python3
"""
Generate tests/golden/simpls_coef_ci_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the
reference is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_coef_ci_golden.py

Inputs are those of the existing simpls_coef_<tag>.npz (X, Y, bootsamples, third, n_components, coef_components,
aggfunc: tests/golden/make_coef_golden.py); nothing of them is stored again.  Per bootstrap sample the reference's
``simpls`` fits c components on what PLSRegression._single_boot fits (regression.py:279-327: the centred X, the
centred Y -- for 3-D Y the original Y aggregated over the resampled third axis --, all-NaN rows dropped); the
coefficients are ``beta[1:]`` (regression.py:149-151).  The fixture holds ``np.percentile`` of them over the bootstraps
at the levels in ``ci``: ``ref_ci`` (len(ci), B, T, 2), [..., 0] lower, [..., 1] upper.  Data only.  All designs have
T <= 11, where the reference's rank-1 randomized SVD is exact.  Before a fixture is written
the same intervals are computed with the CPU oracle (tests/regression_coef_ci_expect.py, from a k-component fit: the
models are nested); a fixture whose two versions differ by more than 1e-10 is refused.
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
from regression_coef_ci_expect import coef_ci_expected, ci_of  # noqa: E402

AGREE = 1e-10
LEVELS = (95, 80)
_AGG = dict(mean=np.mean, median=np.median, sum=np.sum)


def reference_boot(X, Y, subj, third, c, aggfunc):
    agg = _AGG[aggfunc]
    Y_agg = agg(Y, axis=-1) if Y.ndim == 3 else Y
    Xc = X - np.nanmean(X, axis=0, keepdims=True)
    Yc = Y_agg - np.nanmean(Y_agg, axis=0, keepdims=True)
    out = []
    for i in range(subj.shape[1]):
        inds = subj[:, i]
        Xi = Xc[inds]
        Yi = agg(Y[..., third[:, i]], axis=-1)[inds] if Y.ndim == 3 else Yc[inds]
        m = get_mask(Xi, Yi)
        out.append(simpls(Xi[m], Yi[m], c, seed=1234)['beta'][1:])
    return np.stack(out)


def main():
    for tag in ('a', 'nan', 'y3d'):
        g = dict(np.load(os.path.join(HERE, 'simpls_coef_{}.npz'.format(tag)), allow_pickle=False))
        k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
        boot = reference_boot(g['X'], g['Y'], g['bootsamples'], g.get('third'), c, aggfunc)
        got = np.stack([ci_of(boot, ci=level) for level in LEVELS])
        want = np.stack([coef_ci_expected(g['X'], g['Y'], g['bootsamples'], k, c, ci=level, aggfunc=aggfunc,
                                          third=g.get('third')) for level in LEVELS])
        err = max(max_rel(got[i], want[i]) for i in range(len(LEVELS)))
        print('simpls_coef_ci_{}: reference vs oracle {:.1e}  (n = {}, shape {})'.format(
            tag, err, boot.shape[0], got.shape))
        if err > AGREE:
            raise SystemExit('simpls_coef_ci_{}: reference and oracle differ by more than {:g}: not written'
                             .format(tag, AGREE))
        np.savez_compressed(os.path.join(HERE, 'simpls_coef_ci_{}.npz'.format(tag)), ref_ci=got,
                            ci=np.asarray(LEVELS, dtype=float))


if __name__ == '__main__':
    main()
