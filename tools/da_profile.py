"""Time pls_da against pls_regression on the same one-hot Y at BASELINE config 5's X and write profiles/da_c5.json.

    python tools/da_profile.py [--reps 5] [--out profiles/da_c5.json] [--quick] [--auc]

S = 1000, B = 100 000, G = 4 classes, k = 15, test_split = 100, cv_perm = 1000 (100 000 permuted fits) on one GPU, a
fixed-budget engine, n_perm = n_boot = 0.  Both calls get the SAME split masks (stratified) and the same permutations, so
they solve the same fits; pls_da also classifies them (k_sd_cv_class) and ships the confusion counts.

1. Wall time of the two public calls, ALTERNATED (A B A B ...) after one warm-up of each: ``--reps`` pairs, every repeat
   kept, medians, and the median of the per-pair differences.
2. The kernel-class split (plsx_kernel_timing; runs of their own, event timing on) of one call of each, alternated too:
   k_sd_cv_class next to k_sd_cv_score, the solver and its products.
3. The counts of the two routes agree with each other where they overlap: the regression keys of the two results are
   compared bit for bit (recorded, not timed).

``--quick``: B = 2000, test_split = 20, cv_perm = 50 (a rehearsal).

``--auc``: the same shape, masks and permutations, but the two calls that alternate are ``pls_da(..., auc=True)`` and
``pls_da(...)``: what the AUC counts (k_sd_cv_auc) add to the call.  Written to profiles/da_auc_c5.json, with
k_sd_cv_auc next to k_sd_cv_class and k_sd_cv_score in the kernel-class split and the keys of the call without ``auc``
compared bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--auc', action='store_true')
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    out_path = args.out or os.path.join(root, 'profiles', 'da_auc_c5.json' if args.auc else 'da_c5.json')
    S, B, G, k = (1000, 2000, 4, 15) if args.quick else (1000, 100000, 4, 15)
    n, P = (20, 50) if args.quick else (100, 1000)
    rs = np.random.RandomState(0)
    y = rs.permutation(np.arange(S) % G)
    X = rs.randn(S, B)
    nf = B // 10
    X[:, :nf] += (0.1 * rs.randn(G, nf))[y]               # class means shifted on a tenth of the features
    onehot = np.zeros((S, G))
    onehot[np.arange(S), y] = 1.0
    masks = rsmp.gen_stratified_splits(y, n, seed=6, test_size=0.25)
    perms = rsmp.gen_permsamp([S], 1, P, seed=7, verbose=False)
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=n, cvsamples=masks, cv_perm=P, cvpermsamples=perms, seed=1,
              verbose=False, _engine=eng)

    def call_da():
        return pls.pls_da(X, y, **kw)

    def call_reg():
        return pls.pls_regression(X, onehot, **kw)

    if args.auc:
        return profile_auc(args, pls, eng, X, y, kw, dict(S=S, B=B, G=G, n_components=k, test_split=n, cv_perm=P,
                                                          fits=n * (P + 1)), out_path)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    # warm-up at full size (allocations, code objects), then alternate
    _, res_da = timed(call_da)
    _, res_reg = timed(call_reg)
    t_da, t_reg = [], []
    for _ in range(args.reps):
        t_da.append(timed(call_da)[0])
        t_reg.append(timed(call_reg)[0])
    same = all(np.array_equal(res_da.cvres[key], res_reg.cvres[key], equal_nan=True) for key in res_reg.cvres.keys())
    acc, bal = pls.scores_from_confusion(res_da.cvres.confusion.sum(axis=-1))
    out = dict(shape=dict(S=S, B=B, G=G, n_components=k, test_split=n, cv_perm=P, fits=n * (P + 1)), reps=args.reps,
               wall_s_pls_da=round(float(np.median(t_da)), 4), wall_s_pls_da_all=[round(t, 4) for t in t_da],
               wall_s_pls_regression=round(float(np.median(t_reg)), 4),
               wall_s_pls_regression_all=[round(t, 4) for t in t_reg],
               wall_s_median_pair_difference=round(float(np.median(np.array(t_da) - np.array(t_reg))), 4),
               ratio_of_medians=round(float(np.median(t_da) / np.median(t_reg)), 4),
               shared_cvres_keys_bit_identical=bool(same),
               pooled_accuracy_per_c=[round(float(v), 4) for v in acc],
               accuracy_pvals=[round(float(v), 4) for v in res_da.cvres.accuracy_pvals])
    print(json.dumps(out), flush=True)

    # the kernel-class split: event timing on, runs of their own
    kern = {}
    for name, fn in (('pls_da', call_da), ('pls_regression', call_reg), ('pls_da_again', call_da)):
        eng.set_timing(True)
        fn()
        eng.sync()
        kern[name] = {key: [round(v[0], 2), v[1]] for key, v in eng.kernel_timing().items()}
        eng.set_timing(False)
    out['kernel_ms'] = kern
    total = sum(v[0] for v in kern['pls_da'].values())
    out['k_sd_cv_class_ms'] = kern['pls_da'].get('k_sd_cv_class', [0.0, 0])[0]
    out['k_sd_cv_score_ms'] = kern['pls_da'].get('k_sd_cv_score', [0.0, 0])[0]
    out['k_sd_cv_class_share_of_timed_kernels'] = round(out['k_sd_cv_class_ms'] / total, 4)
    out['k_sd_cv_score_share_of_timed_kernels'] = round(out['k_sd_cv_score_ms'] / total, 4)
    eng.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


def profile_auc(args, pls, eng, X, y, kw, shape, out_path):
    """``--auc``: pls_da(auc=True) against pls_da() on the same fits."""
    import torch

    def call_auc():
        return pls.pls_da(X, y, auc=True, **kw)

    def call_da():
        return pls.pls_da(X, y, **kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    _, res_auc = timed(call_auc)
    _, res_da = timed(call_da)
    t_auc, t_da = [], []
    for _ in range(args.reps):
        t_auc.append(timed(call_auc)[0])
        t_da.append(timed(call_da)[0])
    same = all(np.array_equal(res_auc.cvres[key], res_da.cvres[key], equal_nan=True) for key in res_da.cvres.keys())
    cv = res_auc.cvres
    oauc, omacro = pls.auc_from_counts(cv.auc_counts.sum(axis=-1))
    out = dict(shape=shape, reps=args.reps,
               wall_s_pls_da_auc=round(float(np.median(t_auc)), 4), wall_s_pls_da_auc_all=[round(t, 4) for t in t_auc],
               wall_s_pls_da=round(float(np.median(t_da)), 4), wall_s_pls_da_all=[round(t, 4) for t in t_da],
               wall_s_median_pair_difference=round(float(np.median(np.array(t_auc) - np.array(t_da))), 4),
               ratio_of_medians=round(float(np.median(t_auc) / np.median(t_da)), 4),
               shared_cvres_keys_bit_identical=bool(same),
               comparisons=int(cv.auc_counts[:, 1].sum() + cv.perm_auc_counts[:, 1].sum()),
               max_count=int(max(cv.auc_counts.max(), cv.perm_auc_counts.max())),
               pooled_macro_auc_per_c=[round(float(v), 4) for v in omacro],
               auc_macro_pvals=[round(float(v), 4) for v in cv.auc_macro_pvals])
    print(json.dumps(out), flush=True)
    kern = {}
    for name, fn in (('pls_da_auc', call_auc), ('pls_da', call_da), ('pls_da_auc_again', call_auc)):
        eng.set_timing(True)
        fn()
        eng.sync()
        kern[name] = {key: [round(v[0], 2), v[1]] for key, v in eng.kernel_timing().items()}
        eng.set_timing(False)
    out['kernel_ms'] = kern
    total = sum(v[0] for v in kern['pls_da_auc'].values())
    for key in ('k_sd_cv_auc', 'k_sd_cv_class', 'k_sd_cv_score'):
        out[key + '_ms'] = kern['pls_da_auc'].get(key, [0.0, 0])[0]
        out[key + '_share_of_timed_kernels'] = round(out[key + '_ms'] / total, 4)
    eng.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
