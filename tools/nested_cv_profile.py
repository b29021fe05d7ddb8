"""Time the nested cross-validation of pls_regression (inner_split) at BASELINE config 5's solver shape and write
profiles/nested_cv_c5.json.

    python tools/nested_cv_profile.py [--reps 3] [--out profiles/nested_cv_c5.json] [--quick]
                                      [--without-only] [--parent-without FILE] [--root DIR]
                                      [--kernel-run] [--kernel-stats FILE]

S = 1000, B = 100 000, T = 20, k = 15, 100 outer x 10 inner splits, cv_perm = 1000 on one GPU, a fixed-budget engine:
1000 x 100 x 11 = 1.1 million SIMPLS fits in the nested null, against 100 000 in the plain one.

1. The public call with ``inner_split=10`` and the same call without it, ALTERNATED in one process (one warm-up of
   each, then ``--reps`` pairs, every call bracketed by device synchronisation; medians, every repeat kept), with the
   wall time of the phases (``crossval_perm``, ``crossval_nested``, ``crossval_nested_perm``).  The expectation to hold
   the result against: 11 x the fits of the plain null, so about 11 x its measured leg.
2. ``--without-only`` runs the call without the keyword alone and ``--root DIR`` imports the package from another
   checkout (the parent commit's), so the same program measures both sides; ``--parent-without FILE`` copies the parent's
   record into the output.
3. ``--kernel-run`` makes one nested null call at cv_perm = 100 (110 000 fits) and writes nothing: the program to put
   behind ``rocprofv3 --kernel-trace --stats --`` in a run of its own.  ``--kernel-stats FILE`` copies the rows of that
   run's kernel_stats.csv for the three new kernels, k_sd_cv_score and the solver into the output.

``--quick``: B = 2000, 10 outer x 3 inner splits, cv_perm = 50 (a rehearsal)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

KERNELS = ('k_sd_cvn_expand', 'k_sd_cvn_select', 'k_sd_cvn_reduce', 'k_sd_cv_score', 'k_sd_cvp_expand', 'k_sd_cvp_reduce',
           'k_sd_init', 'k_sd_step', 'k_sd_final', 'k_nt_')


def kernel_rows(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r['Name'].split('(')[0].replace('void ', '').strip()
            if any(key in name for key in KERNELS):
                rows[name[:60]] = dict(calls=int(r['Calls']), total_ms=round(float(r['TotalDurationNs']) / 1e6, 3),
                                       avg_ms=round(float(r['AverageNs']) / 1e6, 4))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--without-only', action='store_true')
    ap.add_argument('--parent-without', default=None)
    ap.add_argument('--kernel-run', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    out_path = args.out or os.path.join(root, 'profiles', 'nested_cv_c5.json')
    S, B, T, k, n, ni, P = (1000, 2000, 20, 15, 10, 3, 50) if args.quick else (1000, 100000, 20, 15, 100, 10, 1000)
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=n, seed=1, verbose=False, _engine=eng)

    def call(inner, phases=None, perms=P):
        extra = dict(inner_split=inner) if inner else {}
        t0 = time.perf_counter()
        res = pls.pls_regression(X, Y, cv_perm=perms, _phases=phases, **extra, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    if args.kernel_run:
        call(ni, perms=max(1, P // 10))
        eng.close()
        return
    out = dict(shape=dict(S=S, B=B, T=T, n_components=k, test_split=n, inner_split=ni, cv_perm=P), reps=args.reps,
               fits_plain_null=P * n, fits_nested_null=P * n * (1 + ni), fits_nested_observed=n * (1 + ni))
    call(0)                                                # warm-up at full size (allocations)
    if not args.without_only:
        call(ni)
    t_with, t_without, ph_with, ph_without = [], [], {}, {}
    res = None
    for _ in range(args.reps):
        t_without.append(call(0, ph_without)[0])
        if not args.without_only:
            t, res = call(ni, ph_with)
            t_with.append(t)
    eng.close()

    def leg(ts, phases):
        return dict(wall_s=round(float(np.median(ts)), 4), wall_s_all=[round(t, 4) for t in ts],
                    phase_ms={key: round(val / len(ts), 2) for key, val in phases.items() if key.startswith('crossval')})
    out['call_without_inner_split'] = leg(t_without, ph_without)
    print(json.dumps(dict(call_without_inner_split=out['call_without_inner_split'])), flush=True)
    if not args.without_only:
        out['call_with_inner_split'] = w = leg(t_with, ph_with)
        plain = out['call_without_inner_split']['phase_ms']['crossval_perm']
        out['nested_null_ms'] = w['phase_ms']['crossval_nested_perm']
        out['plain_null_ms'] = plain
        out['ratio_nested_null_to_plain_null'] = round(w['phase_ms']['crossval_nested_perm'] / plain, 3)
        out['ratio_expected_from_the_fit_count'] = 1 + ni
        out['us_per_fit_nested_null'] = round(1e3 * w['phase_ms']['crossval_nested_perm'] / (P * n * (1 + ni)), 3)
        out['us_per_fit_plain_null'] = round(1e3 * plain / (P * n), 3)
        cv = res.cvres
        out['selected'] = dict(nested_ncomp_counts=np.bincount(cv.nested_ncomp, minlength=k + 1).tolist(),
                               perm_nested_ncomp_total=cv.perm_nested_ncomp.sum(axis=1).tolist(),
                               nested_mse_pvals=float(cv.nested_mse_pvals))
    if args.parent_without:
        with open(args.parent_without) as fh:
            out['call_without_inner_split_parent_commit'] = json.load(fh)['call_without_inner_split']
    if args.kernel_stats:
        out['kernel_stats'] = dict(cv_perm=max(1, P // 10), fits=max(1, P // 10) * n * (1 + ni) + n * (1 + ni) + n * (1 + P // 10),
                                   source='rocprofv3 --kernel-trace --stats of --kernel-run, a run of its own',
                                   kernels=kernel_rows(args.kernel_stats))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
