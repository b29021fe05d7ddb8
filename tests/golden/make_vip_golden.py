#!/usr/bin/env python3
"""
Generate tests/golden/simpls_vip_<tag>.npz by RUNNING THE REFERENCE's ``simpls`` (build container only; the
reference is imported the way make_golden.py imports it, h5py stub included):

    python tests/golden/make_vip_golden.py

Inputs are those of the existing simpls_coef_<tag>.npz (X, Y, bootsamples, third, n_components, coef_components --
taken as the component count c of the VIP scores --, aggfunc: tests/golden/make_coef_golden.py); nothing of them is
stored again.  The reference's ``simpls`` fits c components on the original data and, per bootstrap sample, on what
PLSRegression._single_boot fits (regression.py:279-327: the centred X, the centred Y -- for 3-D Y the original Y
aggregated over the resampled third axis --, all-NaN rows dropped).  The VIP scores are the formula of MATLAB's
``plsregress`` documentation applied to its ``x_weights`` and ``y_loadings`` (the x_scores are unit-norm):

    VIP[f] = sqrt(B sum_a ssq_a x_weights[f, a]^2 / |x_weights[:, a]|^2 / sum_a ssq_a),  ssq_a = |y_loadings[:, a]|^2

The fixture holds ``ref_vip`` (B,) of the original fit, ``ref_stderr`` (B,) = np.std(ddof=1) over the bootstraps and
``ref_ci`` (len(ci), B, 2) = np.percentile at the levels in ``ci``.  Data only.  All designs have T <= 11, where the
reference's rank-1 randomized SVD is exact.  A fixture is refused when the same values from the
CPU oracle (tests/regression_vip_expect.py, from a k-component fit: the models are nested) differ by more than 1e-10,
when a fit divides 0 by 0 (no explained variance, a component of zero weight norm) or when sum_f VIP^2 differs from B
by more than 1e-12 relative.
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
from regression_vip_expect import _fits, degenerate, summary, vip_expected, vip_of   # noqa: E402

AGREE = 1e-10
INVARIANT = 1e-12
LEVELS = (95, 80)


def main():
    for tag in ('a', 'nan', 'y3d'):
        g = dict(np.load(os.path.join(HERE, 'simpls_coef_{}.npz'.format(tag)), allow_pickle=False))
        k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
        B = g['X'].shape[1]
        fits = list(_fits(g['X'], g['Y'], g['bootsamples'], c, aggfunc, g.get('third'),
                          lambda X, Y, n: simpls(X, Y, n, seed=1234), get_mask))
        if any(degenerate(f, c) for f in fits):
            raise SystemExit('simpls_vip_{}: a fit divides 0 by 0: not written'.format(tag))
        vips = np.stack([vip_of(f, c) for f in fits])
        inv = float(np.max(np.abs((vips ** 2).sum(axis=1) - B)) / B)
        if inv > INVARIANT:
            raise SystemExit('simpls_vip_{}: sum VIP^2 is off B by {:.1e} relative: not written'.format(tag, inv))
        vip, boot = vips[0], vips[1:]
        sd = summary(boot)[0]
        civ = np.stack([summary(boot, ci=level)[1] for level in LEVELS])
        want = [vip_expected(g['X'], g['Y'], g['bootsamples'], k, c, ci=level, aggfunc=aggfunc, third=g.get('third'))
                for level in LEVELS]
        err = max([max_rel(vip, want[0]['vip']), max_rel(sd, want[0]['stderr'])]
                  + [max_rel(civ[i], want[i]['ci']) for i in range(len(LEVELS))])
        print('simpls_vip_{}: reference vs oracle {:.1e}, invariant {:.1e}  (n = {}, c = {}, B = {})'.format(
            tag, err, inv, boot.shape[0], c, B))
        if err > AGREE:
            raise SystemExit('simpls_vip_{}: reference and oracle differ by more than {:g}: not written'
                             .format(tag, AGREE))
        np.savez_compressed(os.path.join(HERE, 'simpls_vip_{}.npz'.format(tag)), ref_vip=vip, ref_stderr=sd, ref_ci=civ,
                            ci=np.asarray(LEVELS, dtype=float))


if __name__ == '__main__':
    main()
