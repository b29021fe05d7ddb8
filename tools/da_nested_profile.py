"""Time the nested cross-validation of pls_da (inner_split, inner_select) at BASELINE config 5's X against
pls_regression's nested call on the same one-hot Y, and write profiles/da_nested_c5.json.

    python tools/da_nested_profile.py [--reps 3] [--out profiles/da_nested_c5.json] [--quick] [--auc]
                                      [--unchanged-only] [--parent FILE] [--root DIR]
                                      [--kernel-run] [--kernel-stats FILE]

S = 1000, B = 100 000, G = 4 classes, k = 15, 100 outer x 10 inner splits, cv_perm = 1000 on one GPU, a fixed-budget
engine, n_perm = n_boot = 0: 1.1 million SIMPLS fits in the nested null.  All calls get the SAME outer masks
(stratified), inner codes and permutations, so they solve the same fits.

1. ``pls_da(inner_split=10)`` (selection on the pooled balanced accuracy; every fit classified), ``pls_regression(
   inner_split=10)`` on the one-hot Y (selection on the inner mse; nothing classified) and ``pls_da`` without the
   keyword, ALTERNATED in one process after one warm-up of each: ``--reps`` rounds, every repeat kept, medians, with the
   wall time of the phases.  The expectation to hold the result against: the regression nested call plus the per-fit
   classification share that profiles/da_c5.json shows for the plain cross-validation.
2. ``--unchanged-only`` runs the two calls that exist at the parent commit alone -- ``pls_regression(inner_split=10)``
   and ``pls_da`` without the keyword -- and ``--root DIR`` imports the package from another checkout (the parent
   commit's), so the same program measures both sides; ``--parent FILE`` copies the parent's record into the output.
3. ``--kernel-run`` makes one nested pls_da call at cv_perm = 100 and writes nothing: the program to put behind
   ``rocprofv3 --kernel-trace --stats --`` in a run of its own.  ``--kernel-stats FILE`` copies the rows of that run's
   kernel_stats.csv for the selection and reduction kernels, the counting kernels, k_sd_cv_score and the solver.

``--quick``: B = 2000, 10 outer x 3 inner splits, cv_perm = 50 (a rehearsal).  ``--auc``: the pls_da calls with
``auc=True``."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

KERNELS = ('k_sd_cvn_', 'k_sd_cv_class', 'k_sd_cv_auc', 'k_sd_cv_score', 'k_sd_cvp_', 'k_sd_init', 'k_sd_step',
           'k_sd_final', 'k_nt_')


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
    ap.add_argument('--auc', action='store_true')
    ap.add_argument('--unchanged-only', action='store_true')
    ap.add_argument('--parent', default=None)
    ap.add_argument('--kernel-run', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    out_path = args.out or os.path.join(root, 'profiles', 'da_nested_c5.json')
    S, B, G, k, n, ni, P = (1000, 2000, 4, 15, 10, 3, 50) if args.quick else (1000, 100000, 4, 15, 100, 10, 1000)
    rs = np.random.RandomState(0)
    y = rs.permutation(np.arange(S) % G)
    X = rs.randn(S, B)
    nf = B // 10
    X[:, :nf] += (0.1 * rs.randn(G, nf))[y]               # class means shifted on a tenth of the features
    onehot = np.zeros((S, G))
    onehot[np.arange(S), y] = 1.0
    masks = rsmp.gen_stratified_splits(y, n, seed=6, test_size=0.25)
    # the inner folds, stratified as pls_da draws them -- written out with gen_stratified_splits so that the program
    # also runs against a checkout whose _draw_inner_codes knows no classes
    inner = np.full((S, n, ni), 2, dtype=np.uint8)
    r_in = np.random.RandomState(8)
    for s in range(n):
        rows = np.flatnonzero(masks[:, s])
        inner[rows, s, :] = rsmp.gen_stratified_splits(y[rows], ni, seed=r_in, test_size=0.25)
    perms = rsmp.gen_permsamp([S], 1, P, seed=7, verbose=False)
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=n, cvsamples=masks, seed=1, verbose=False, _engine=eng)
    nest = dict(inner_split=ni, innersamples=inner)
    da_kw = dict(auc=True) if args.auc else {}

    def timed(fn, phases=None, perms_=None):
        p = perms if perms_ is None else perms_
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(cv_perm=p.shape[1], cvpermsamples=p, _phases=phases)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    legs = dict(pls_regression_nested=lambda **c: pls.pls_regression(X, onehot, **nest, **c, **kw),
                pls_da_plain=lambda **c: pls.pls_da(X, y, **da_kw, **c, **kw))
    if not args.unchanged_only:
        legs['pls_da_nested'] = lambda **c: pls.pls_da(X, y, inner_select='balanced_accuracy', **nest, **da_kw, **c, **kw)
    if args.kernel_run:
        timed(legs['pls_da_nested'], perms_=perms[:, :max(1, P // 10)])
        eng.close()
        return
    out = dict(shape=dict(S=S, B=B, G=G, n_components=k, test_split=n, inner_split=ni, cv_perm=P, auc=bool(args.auc)),
               reps=args.reps, fits_nested_null=P * n * (1 + ni), fits_plain_null=P * n)
    times = {name: [] for name in legs}
    phases = {name: {} for name in legs}
    last = {}
    for name, fn in legs.items():                          # warm-up at full size (allocations, code objects)
        timed(fn)
    for _ in range(args.reps):
        for name, fn in legs.items():
            t, last[name] = timed(fn, phases[name])
            times[name].append(t)
    eng.close()
    for name in legs:
        ts = times[name]
        out[name] = dict(wall_s=round(float(np.median(ts)), 4), wall_s_all=[round(t, 4) for t in ts],
                         spread_s=round(float(max(ts) - min(ts)), 4),
                         phase_ms={key: round(val / len(ts), 2) for key, val in phases[name].items()
                                   if key.startswith('crossval')})
    if not args.unchanged_only:
        a, b = out['pls_da_nested']['phase_ms'], out['pls_regression_nested']['phase_ms']
        plain = out['pls_da_plain']['phase_ms']
        out['nested_null_ms'] = dict(pls_da=a['crossval_nested_perm'], pls_regression=b['crossval_nested_perm'],
                                     ratio=round(a['crossval_nested_perm'] / b['crossval_nested_perm'], 4))
        out['us_per_fit_nested_null'] = dict(pls_da=round(1e3 * a['crossval_nested_perm'] / (P * n * (1 + ni)), 3),
                                             pls_regression=round(1e3 * b['crossval_nested_perm'] / (P * n * (1 + ni)), 3))
        out['us_per_fit_plain_null_pls_da'] = round(1e3 * plain['crossval_perm'] / (P * n), 3)
        cv = last['pls_da_nested'].cvres
        reg = last['pls_regression_nested'].cvres
        out['selected'] = dict(nested_ncomp_counts=np.bincount(cv.nested_ncomp, minlength=k + 1).tolist(),
                               perm_nested_ncomp_total=cv.perm_nested_ncomp.sum(axis=1).tolist(),
                               nested_balanced_accuracy_mean=round(float(np.mean(cv.nested_balanced_accuracy)), 4),
                               best_row_of_balanced_accuracy=round(float(cv.balanced_accuracy.mean(axis=1).max()), 4),
                               nested_balanced_accuracy_pvals=float(cv.nested_balanced_accuracy_pvals),
                               inner_mse_bit_identical_to_pls_regression=bool(np.array_equal(cv.inner_mse, reg.inner_mse)))
    if args.parent:
        with open(args.parent) as fh:
            parent = json.load(fh)
        out['parent_commit'] = {name: parent[name] for name in ('pls_regression_nested', 'pls_da_plain')}
    if args.kernel_stats:
        out['kernel_stats'] = dict(cv_perm=max(1, P // 10),
                                   source='rocprofv3 --kernel-trace --stats of --kernel-run, a run of its own',
                                   kernels=kernel_rows(args.kernel_stats))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
