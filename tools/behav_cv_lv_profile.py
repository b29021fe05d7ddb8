"""Time behavioral_pls(cv_lv=True) at the headline shape and write profiles/behav_cv_lv_c4.json.

    python tools/behav_cv_lv_profile.py [--reps 3] [--out profiles/behav_cv_lv_c4.json] [--quick]

S = 500, B = 200 000, T = 50 (one cell), 100 splits, P = 1000 permutations of the cross-validation, n_perm = n_boot = 0,
one GPU, a fixed-budget engine.  Four calls -- with and without ``cv_perm=P``, each with and without ``cv_lv=True`` --
one warm-up of each, then ``--reps`` timed rounds that alternate the four; medians of the wall time of the public call
(it ends in a device synchronise) and of the front-end's ``crossval`` / ``crossval_perm`` phases.

Then one timed call of each ``cv_lv`` kind for the kernel classes (plsx_kernel_timing; events on the launch stream, not
used for the wall times): the bar of the feature is that the added scoring stays below the scoring it follows --
k_cvp_lv below k_cvp_final (class k_sd_cv_score holds nothing else on this call) on the null, k_cv_lv below k_cv_final
on the observed leg.

``--quick``: B = 4000, 10 splits, P = 50 (a rehearsal)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'behav_cv_lv_c4.json'))
    ap.add_argument('--quick', action='store_true')
    args = ap.parse_args()
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, B, T, ns, P = (500, 4000, 50, 10, 50) if args.quick else (500, 200000, 50, 100, 1000)
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)

    def call(p, lv, timing=False):
        phases = {}
        kw = dict(n_perm=0, n_boot=0, test_split=ns, test_size=0.25, seed=1, verbose=False, _engine=eng, _phases=phases)
        if p:
            kw['cv_perm'] = p
        if lv:
            kw['cv_lv'] = True
        torch.cuda.synchronize()
        eng.set_timing(timing)
        t0 = time.perf_counter()
        res = pls.behavioral_pls(X, Y, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kt = eng.kernel_timing() if timing else {}
        eng.set_timing(False)
        return dict(wall_s=wall, phases=phases, kt=kt, res=res)

    kinds = [(0, False), (0, True), (P, False), (P, True)]
    for kind in kinds:
        call(*kind)
    runs = {kind: [] for kind in kinds}
    for _ in range(args.reps):
        for kind in kinds:
            runs[kind].append(call(*kind))

    def med(kind, fn):
        return round(float(np.median([fn(r) for r in runs[kind]])), 4)

    def block(p):
        a, b = (p, False), (p, True)
        d = dict(wall_s_without=med(a, lambda r: r['wall_s']), wall_s_with=med(b, lambda r: r['wall_s']),
                 wall_s_all_without=[round(r['wall_s'], 4) for r in runs[a]],
                 wall_s_all_with=[round(r['wall_s'], 4) for r in runs[b]],
                 crossval_phase_ms_without=med(a, lambda r: r['phases'].get('crossval', 0.0)),
                 crossval_phase_ms_with=med(b, lambda r: r['phases'].get('crossval', 0.0)))
        if p:
            d.update(crossval_perm_phase_ms_without=med(a, lambda r: r['phases'].get('crossval_perm', 0.0)),
                     crossval_perm_phase_ms_with=med(b, lambda r: r['phases'].get('crossval_perm', 0.0)))
        d['with_over_without'] = round(d['wall_s_with'] / d['wall_s_without'], 4)
        return d

    out = dict(shape=dict(S=S, B=B, T=T, cells=1, splits=ns, cv_perm=P, n_perm=0, n_boot=0), reps=args.reps,
               call_without_cv_perm=block(0), call_with_cv_perm=block(P))

    # kernel classes: one timed call per kind with cv_lv
    def classes(kt):
        return {k: [round(v[0], 3), v[1]] for k, v in kt.items()}

    def ms(kt, name):
        return kt.get(name, (0.0, 0))[0]

    t_obs = call(0, True, timing=True)
    t_null = call(P, True, timing=True)
    ko, kn = t_obs['kt'], t_null['kt']
    out['observed_leg'] = dict(
        k_cv_final_ms=round(ms(ko, 'k_cv_final'), 3), k_cv_lv_ms=round(ms(ko, 'k_cv_lv'), 3),
        k_cv_lv_over_k_cv_final=round(ms(ko, 'k_cv_lv') / ms(ko, 'k_cv_final'), 4) if ms(ko, 'k_cv_final') > 0 else None,
        classes=classes(ko))
    out['null'] = dict(
        k_cvp_final_ms=round(ms(kn, 'k_sd_cv_score'), 3), k_cvp_lv_ms=round(ms(kn, 'k_cvp_lv'), 3),
        k_cvp_lv_over_k_cvp_final=round(ms(kn, 'k_cvp_lv') / ms(kn, 'k_sd_cv_score'), 4) if ms(kn, 'k_sd_cv_score') > 0 else None,
        note='class k_sd_cv_score holds k_cvp_final alone on this call (the observed leg\'s k_cv_final has its own class)',
        classes=classes(kn))
    cv = t_null['res'].cvres
    live = np.isfinite(cv.lv_corr).all(axis=1)
    out['result_check'] = dict(lv_corr_shape=list(cv.lv_corr.shape), perm_lv_corr_shape=list(cv.perm_lv_corr.shape),
                               live_lvs=int(live.sum()), lv0_mean=float(cv.lv_corr[0].mean()),
                               null_lv0_mean=float(np.nanmean(cv.perm_lv_corr[0])),
                               lv_corr_pvals_first3=[float(v) for v in cv.lv_corr_pvals[:3]],
                               same_bits_as_without=bool(all(
                                   np.array_equal(cv[k], runs[(P, False)][0]['res'].cvres[k])
                                   for k in ('pearson_r', 'r_squared', 'perm_pearson_r', 'perm_r_squared'))))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
