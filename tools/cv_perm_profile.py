"""Time the permutation test of pls_regression's cross-validation (cv_perm) at BASELINE config 5's solver shape and write
profiles/cv_perm_c5.json.

    python tools/cv_perm_profile.py [--reps 5] [--out profiles/cv_perm_c5.json] [--quick]
                                    [--yardstick-only] [--parent-yardstick FILE] [--root DIR]

S = 1000, B = 100 000, T = 20, k = 15, 100 splits on one GPU, a fixed-budget engine.  Three legs, each one warm-up call
and then ``--reps`` timed calls bracketed by device synchronisation; medians, every repeat kept.

1. The yardstick: plsx_simpls_crossval_batch on 8192 drawn splits, time per fit.  This leg uses only entries the
   library had before cv_perm existed: ``--yardstick-only`` runs it alone and ``--root DIR`` imports the package from
   another checkout (the parent commit's), so the same program measures both sides; ``--parent-yardstick FILE`` copies
   the parent's record into the output.
2. plsx_simpls_crossval_perm_batch under the 100 splits at P = 82 (8200 fits, the yardstick's batch size) and P = 1000
   (100 000 fits), time per fit; and the public call end to end (test_split=100, cv_perm=1000, n_perm = n_boot = 0).
3. The kernel-class split of the P = 1000 call (plsx_kernel_timing; a run of its own, event timing on).

``--quick``: B = 2000, 2048 splits, P = 21 / 100 (a rehearsal)."""
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
    ap.add_argument('--yardstick-only', action='store_true')
    ap.add_argument('--parent-yardstick', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    out_path = args.out or os.path.join(root, 'profiles', 'cv_perm_c5.json')
    S, B, T, k, n = (1000, 2000, 20, 15, 100) if args.quick else (1000, 100000, 20, 15, 100)
    n_yard, P_small, P_big = (2048, 21, 100) if args.quick else (8192, 82, 1000)
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)
    eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)

    def timed(fn, reps):
        fn()                                               # warm-up at full size (allocations)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts

    def leg(ts, fits):
        med = float(np.median(ts))
        return dict(fits=fits, wall_s=round(med, 5), wall_s_all=[round(t, 5) for t in ts],
                    us_per_fit=round(1e6 * med / fits, 3), fits_per_s=round(fits / med, 1))

    # ---- 1. the yardstick
    ymasks = rsmp.gen_splits([S], 1, n_yard, seed=5, test_size=0.25)
    dmy = torch.from_numpy(np.ascontiguousarray(ymasks.T, dtype=np.uint8)).to(eng.device)
    yo = [eng._zeros((n_yard, k, T)), eng._zeros((n_yard, k, T)), eng._zeros((n_yard, k + 1, T))]
    yard = leg(timed(lambda: eng.simpls_crossval_into(dmy, *yo), args.reps), n_yard)
    out = dict(shape=dict(S=S, B=B, T=T, n_components=k, test_split=n), reps=args.reps,
               yardstick_crossval_batch=yard)
    print(json.dumps(dict(yardstick_crossval_batch=yard)), flush=True)
    if args.yardstick_only:
        eng.close()
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')
        return
    if args.parent_yardstick:
        with open(args.parent_yardstick) as fh:
            out['yardstick_crossval_batch_parent_commit'] = json.load(fh)['yardstick_crossval_batch']

    # ---- 2. the new entry under the 100 splits
    masks = rsmp.gen_splits([S], 1, n, seed=6, test_size=0.25)
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    for name, P, reps in (('perm_batch_one_solver_batch', P_small, args.reps), ('perm_batch', P_big, max(3, args.reps // 2))):
        perms = rsmp.gen_permsamp([S], 1, P, seed=7, verbose=False)
        di = eng.rows_tensor(perms.T)
        po = [eng._zeros((P, k, T)), eng._zeros((P, k, T)), eng._zeros((P, k + 1))]
        out[name] = dict(leg(timed(lambda: eng.simpls_crossval_perm_into(dm, di, *po), reps), P * n), cv_perm=P)
        print(json.dumps({name: out[name]}), flush=True)
    # ---- 3. the kernel-class split of the large call (event timing on: a run of its own)
    eng.set_timing(True)
    eng.simpls_crossval_perm_into(dm, di, *po)
    eng.sync()
    out['kernel_ms_perm_batch'] = {key: [round(v[0], 2), v[1]] for key, v in eng.kernel_timing().items()}
    eng.set_timing(False)
    eng.set_timing(True)
    eng.simpls_crossval_into(dmy, *yo)
    eng.sync()
    out['kernel_ms_yardstick'] = {key: [round(v[0], 2), v[1]] for key, v in eng.kernel_timing().items()}
    eng.set_timing(False)
    eng.close()
    # ---- the public call end to end
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=n, seed=1, verbose=False, _engine=eng)
    phases = {}
    ts = timed(lambda: pls.pls_regression(X, Y, cv_perm=P_big, _phases=phases, **kw), max(3, args.reps // 2))
    ts0 = timed(lambda: pls.pls_regression(X, Y, **kw), max(3, args.reps // 2))
    out['public_call'] = dict(cv_perm=P_big, wall_s_with=round(float(np.median(ts)), 4), wall_s_all_with=[round(t, 4) for t in ts],
                              wall_s_without=round(float(np.median(ts0)), 4), wall_s_all_without=[round(t, 4) for t in ts0],
                              crossval_perm_phase_ms=round(phases.get('crossval_perm', 0.0) / (len(ts) + 1), 2))
    eng.close()
    out['ratio_perm_fit_to_yardstick_fit_equal_batch'] = round(
        out['perm_batch_one_solver_batch']['us_per_fit'] / yard['us_per_fit'], 4)
    out['ratio_perm_fit_to_yardstick_fit_large'] = round(out['perm_batch']['us_per_fit'] / yard['us_per_fit'], 4)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
