"""Time behavioral_pls(cv_perm=P) at the headline shape and write profiles/behav_cv_perm_c4.json.

    python tools/behav_cv_perm_profile.py [--reps 3] [--out profiles/behav_cv_perm_c4.json] [--quick]

S = 500, B = 200 000, T = 50 (one cell), 100 splits, P = 1000 permutations of the cross-validation, n_perm = n_boot = 0,
one GPU, a fixed-budget engine.  One warm-up call of each kind, then ``--reps`` timed calls with and without
``cv_perm``, alternating; medians.

1. Wall time of the public call with and without the keyword, and the front-end's phases ``crossval`` (the observed
   leg on the same 100 splits, unchanged by this feature) and ``crossval_perm`` (both end in a device synchronise).
   The feature-route cost of the same null is an EXTRAPOLATION: P x the measured ``crossval`` phase -- that leg does
   not depend on the values of Y.
2. k_cvp_gram (with the sum of its partial tiles; 2 S^2 B flop per split, the full S x S product) next to k_nt_gemm<2>
   forming the plain K = X X^T of the dual permutation route at the same S and B in the same process (the symmetric
   form: upper blocks only, S^2 B flop issued -- plsx_last_timing's nt_flops counts what was issued), both against
   plsx_mfma_f64_peak.
3. The kernel classes of the null (plsx_kernel_timing): moment tables, scaled Gram, operand build, W', G, small solve,
   scoring, split reduction.

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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'behav_cv_perm_c4.json'))
    ap.add_argument('--quick', action='store_true')
    args = ap.parse_args()
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    from pypyls_amd import resampling
    S, B, T, ns, P = (500, 4000, 50, 10, 50) if args.quick else (500, 200000, 50, 100, 1000)
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)

    def call(p, timing=False):
        phases = {}
        kw = dict(n_perm=0, n_boot=0, test_split=ns, test_size=0.25, seed=1, verbose=False, _engine=eng, _phases=phases)
        if p:
            kw['cv_perm'] = p
        torch.cuda.synchronize()
        eng.set_timing(timing)
        t0 = time.perf_counter()
        res = pls.behavioral_pls(X, Y, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kt = eng.kernel_timing() if timing else {}
        eng.set_timing(False)
        return dict(wall_s=wall, phases=phases, kt=kt, res=res)

    call(0)
    call(P)
    runs = {0: [], P: []}
    for _ in range(args.reps):
        for flag in (0, P):
            runs[flag].append(call(flag))

    def med(flag, fn):
        return float(np.median([fn(r) for r in runs[flag]]))

    cv_ms = med(P, lambda r: r['phases'].get('crossval', 0.0))
    null_ms = med(P, lambda r: r['phases'].get('crossval_perm', 0.0))
    out = dict(shape=dict(S=S, B=B, T=T, cells=1, splits=ns, cv_perm=P, n_perm=0, n_boot=0), reps=args.reps)
    out['public_call'] = dict(
        wall_s_without=round(med(0, lambda r: r['wall_s']), 4), wall_s_with=round(med(P, lambda r: r['wall_s']), 4),
        wall_s_all_without=[round(r['wall_s'], 4) for r in runs[0]], wall_s_all_with=[round(r['wall_s'], 4) for r in runs[P]],
        crossval_phase_ms=round(cv_ms, 2), crossval_perm_phase_ms=round(null_ms, 2),
        feature_route_null_s_EXTRAPOLATED=round(P * cv_ms / 1e3, 2),
        extrapolation='P x the crossval phase of the same {} splits (measured here; the leg is the parent\'s, unchanged)'.format(ns),
        ratio_extrapolated_over_measured=round(P * cv_ms / null_ms, 1) if null_ms > 0 else None)
    # the kernel classes of the null: a timed call (events on the launch stream; not used for the wall times above)
    timed = call(P, timing=True)
    kt = timed['kt']

    def ms(name):
        return round(kt.get(name, (0.0, 0))[0], 3)
    gram_ms = kt.get('k_cvp_gram', (0.0, 0))[0]
    gram_flop = 2.0 * S * S * B * ns
    out['null_kernel_ms'] = dict(
        moment_tables=ms('k_cvp_moments'), scaled_gram=ms('k_cvp_gram'), operand_build=ms('k_build_A'), W=ms('k_cvp_w'),
        G=ms('k_cvp_g'), small_solve=ms('k_small'), scoring=ms('k_sd_cv_score'), split_reduction=ms('k_cvp_mean'),
        note='one timed call; k_build_A / k_small / k_sd_cv_score hold nothing else on this call except the observed '
             'leg\'s own small solve ({} splits)'.format(ns),
        launches={k: v[1] for k, v in kt.items() if v[1]})
    out['scaled_gram'] = dict(ms=round(gram_ms, 3), flop=gram_flop,
                              tflops=round(gram_flop / (gram_ms * 1e9), 2) if gram_ms > 0 else None)
    # the plain K = X X^T of the dual permutation route, same S and B, same process
    plain = None
    try:
        perms = resampling.gen_permsamp([S], 1, 1, seed=3, verbose=False)
        eng.set_perm_path(None)
        if eng.set_perm_path(True):
            eng.perm(perms)                                    # warm: forms K once
            eng.set_perm_path(None)
            eng.set_perm_path(True)
            eng.set_timing(True)
            eng.perm(perms)
            k2 = eng.kernel_timing()
            flops = eng.last_timing()['nt_flops']
            eng.set_timing(False)
            nt_ms = k2.get('k_nt_gemm', (0.0, 0))[0]
            plain = dict(ms=round(nt_ms, 3), flop_issued=flops, launches=k2.get('k_nt_gemm', (0.0, 0))[1],
                         tflops=round(flops / (nt_ms * 1e9), 2) if nt_ms > 0 else None,
                         note='k_nt_gemm<2>, symmetric K (upper blocks) + reduce, plus the W / G products of one permutation')
    except Exception as exc:                                   # recorded, not hidden
        plain = dict(error=repr(exc))
    out['plain_gram_k_nt_gemm'] = plain
    if plain and plain.get('tflops') and out['scaled_gram']['tflops']:
        out['scaled_over_plain_rate'] = round(out['scaled_gram']['tflops'] / plain['tflops'], 3)
    out['mfma_f64_peak_tflops'] = round(eng.mfma_f64_peak(), 1)
    cv = timed['res'].cvres
    out['result_check'] = dict(finite=bool(np.isfinite(cv.perm_pearson_r).all() and np.isfinite(cv.perm_r_squared).all()),
                               pearson_r_pvals_min_max=[float(cv.pearson_r_pvals.min()), float(cv.pearson_r_pvals.max())])
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
