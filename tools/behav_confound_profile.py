"""Time behavioral_pls(confounds=Z) at the headline shape and write profiles/behav_confound_c4.json.

    python tools/behav_confound_profile.py [--reps 3] [--out profiles/behav_confound_c4.json] [--quick]

S = 500, B = 200 000, T = 50 (one cell), q = 5 confounds, 100 splits, P = 1000 permutations of the cross-validation,
n_perm = n_boot = 0, one GPU, a fixed-budget engine.  Four calls -- with and without ``confounds=Z``, each with and
without ``cv_perm=P`` -- one warm-up of each, then ``--reps`` timed rounds that alternate the four on the same build;
medians of the wall time of the public call (it ends in a device synchronise) and of the front-end's ``h2d_and_bind``,
``crossval`` and ``crossval_perm`` phases.  The calls without the keyword run the code of the parent commit: their
``crossval`` phase is the observed leg without confounds.

Then one timed call with the keyword for the kernel classes (plsx_kernel_timing; events on the launch stream, not used
for the wall times): k_cfb_fold_X moves (2 / g + 1) 8 S Bpad bytes per split (X_r read twice per launch of g <= 4 splits,
every copy written once), set against the 6.3 TB/s streaming rate the project measured.

``--quick``: B = 4000, 10 splits, P = 50 (a rehearsal)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAM_TBS = 6.3
LAUNCH_SPLITS = 4                                        # CFB_G of csrc/plsx_k_confound_behav.h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'behav_confound_c4.json'))
    ap.add_argument('--quick', action='store_true')
    args = ap.parse_args()
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, B, T, q, ns, P = (500, 4000, 50, 5, 10, 50) if args.quick else (500, 200000, 50, 5, 100, 1000)
    rs = np.random.RandomState(0)
    Z = rs.randn(S, q)
    X = rs.randn(S, B) + Z @ rs.randn(q, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T) + Z @ rs.randn(q, T)
    eng = Engine(scratch_gb=48.0)

    def call(cf, p, timing=False):
        phases = {}
        kw = dict(n_perm=0, n_boot=0, test_split=ns, test_size=0.25, seed=1, verbose=False, _engine=eng, _phases=phases)
        if p:
            kw['cv_perm'] = p
        if cf:
            kw['confounds'] = Z
        torch.cuda.synchronize()
        eng.set_timing(timing)
        t0 = time.perf_counter()
        res = pls.behavioral_pls(X, Y, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kt = eng.kernel_timing() if timing else {}
        eng.set_timing(False)
        return dict(wall_s=wall, phases=phases, kt=kt, res=res, group=eng.crossval_confound_group() if cf else 0)

    kinds = [(False, 0), (True, 0), (False, P), (True, P)]
    for kind in kinds:
        call(*kind)
    runs = {kind: [] for kind in kinds}
    for _ in range(args.reps):
        for kind in kinds:
            r = call(*kind)
            r.pop('res')
            runs[kind].append(r)

    def med(kind, fn):
        return round(float(np.median([fn(r) for r in runs[kind]])), 4)

    def block(p):
        a, b = (False, p), (True, p)
        d = dict(wall_s_without=med(a, lambda r: r['wall_s']), wall_s_with=med(b, lambda r: r['wall_s']),
                 wall_s_all_without=[round(r['wall_s'], 4) for r in runs[a]],
                 wall_s_all_with=[round(r['wall_s'], 4) for r in runs[b]])
        for ph in ('h2d_and_bind', 'crossval') + (('crossval_perm',) if p else ()):
            d[ph + '_phase_ms_without'] = med(a, lambda r: r['phases'].get(ph, 0.0))
            d[ph + '_phase_ms_with'] = med(b, lambda r: r['phases'].get(ph, 0.0))
        d['with_over_without'] = round(d['wall_s_with'] / d['wall_s_without'], 4)
        return d

    out = dict(shape=dict(S=S, B=B, T=T, q=q, cells=1, splits=ns, cv_perm=P, n_perm=0, n_boot=0), reps=args.reps,
               call_without_cv_perm=block(0), call_with_cv_perm=block(P))
    obs = out['call_without_cv_perm']
    out['observed_leg'] = dict(
        crossval_phase_ms_without_confounds=obs['crossval_phase_ms_without'],
        crossval_phase_ms_with_confounds=obs['crossval_phase_ms_with'],
        per_split_ms_with_confounds=round(obs['crossval_phase_ms_with'] / ns, 4),
        note='with confounds every split runs the dual-space body of the permutation null on its own fold copy '
             '(tables, the scaled S x S matrix, the fit under the identity arrangement), a group of splits at a time; '
             'without them the leg is the batched feature-space pass of plsx_crossval_batch')

    # kernel classes: one timed call of the observed leg with the keyword, one of the null
    def classes(kt):
        return {k: [round(v[0], 3), v[1]] for k, v in kt.items()}

    t_obs = call(True, 0, timing=True)
    g = t_obs['group']
    ms, brackets = t_obs['kt'].get('k_cfb_fold_X', (0.0, 0))
    nbytes = 0.0
    for s0 in range(0, ns, max(g, 1)):
        grp = min(g, ns - s0)
        for a in range(0, grp, LAUNCH_SPLITS):
            nbytes += (2 + min(LAUNCH_SPLITS, grp - a)) * 8.0 * S * B
    tbs = nbytes / (ms * 1e-3) / 1e12 if ms > 0 else None
    out['k_cfb_fold_X'] = dict(
        splits_per_group=g, splits_per_launch=LAUNCH_SPLITS, ms=round(ms, 3), brackets=brackets,
        gbytes=round(nbytes / 1e9, 3), tb_per_s=None if tbs is None else round(tbs, 3),
        fraction_of_streaming_rate=None if tbs is None else round(tbs / STREAM_TBS, 3), streaming_rate_tb_per_s=STREAM_TBS,
        bytes_note='(2 + g) 8 S B per launch of g splits, B for Bpad')
    out['observed_classes'] = classes(t_obs['kt'])
    t_null = call(True, P, timing=True)
    out['null_classes'] = classes(t_null['kt'])
    cv = t_null['res'].cvres
    out['result_check'] = dict(pearson_r_mean=float(cv.pearson_r.mean()), perm_pearson_r_mean=float(cv.perm_pearson_r.mean()),
                               pvals_first3=[float(v) for v in cv.pearson_r_pvals[:3]],
                               finite=bool(np.isfinite(cv.pearson_r).all() and np.isfinite(cv.perm_pearson_r).all()))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
