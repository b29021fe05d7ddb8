"""Time pls_regression(confounds=Z) at BASELINE config 5's solver shape and write profiles/confound_c5.json.

    python tools/confound_profile.py [--reps 3] [--out profiles/confound_c5.json] [--quick]

S = 1000, B = 100 000, T = 20, k = 15, q = 5, 100 splits, cv_perm = 1000, n_perm = n_boot = 0, one GPU, a fixed-budget
engine.  Two calls, alternated in one process after one warm-up each, bracketed by device synchronisation; medians,
every repeat kept:

(i)  the call with ``confounds=Z``: residuals on the device, the confound regression fitted per fold;
(ii) the same call without the keyword on host-residualised (X_r, Y_r) -- what the library could do before the keyword
     existed.  It is NOT the same statistic (its residuals leak the test rows into the training data); the host
     residualisation itself is timed apart and not counted.

Then one run of (i) with event timing on: the kernel-class split (plsx_kernel_timing), and from it the achieved bytes/s
of k_cf_resid (X read twice and written once, 3 x 8 S B bytes) and of k_cf_fold_K (K_s written, 8 S^2 bytes per split
and call; the K_r tiles it reads stay in cache).

``--quick``: B = 2000, 20 splits, cv_perm = 50 (a rehearsal)."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true')
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    out_path = args.out or os.path.join(root, 'profiles', 'confound_c5.json')
    S, B, T, k, q, n, P = (1000, 2000, 20, 15, 5, 20, 50) if args.quick else (1000, 100000, 20, 15, 5, 100, 1000)
    rs = np.random.RandomState(0)
    Z = rs.randn(S, q)
    X = rs.randn(S, B) + Z @ rs.randn(q, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T) + Z @ rs.randn(q, T)
    t0 = time.perf_counter()
    D = np.c_[np.ones(S), Z]
    Xr = X - D @ np.linalg.lstsq(D, X, rcond=None)[0]
    Yr = Y - D @ np.linalg.lstsq(D, Y, rcond=None)[0]
    host_resid_s = time.perf_counter() - t0
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=n, cv_perm=P, seed=1, verbose=False, _engine=eng)
    calls = dict(with_confounds=lambda ph=None: pls.pls_regression(X, Y, confounds=Z, _phases=ph, **kw),
                 host_residuals_no_keyword=lambda ph=None: pls.pls_regression(Xr, Yr, _phases=ph, **kw))
    times = {name: [] for name in calls}
    phases = {name: {} for name in calls}
    for name, fn in calls.items():                        # warm-up at full size (allocations)
        fn()
        torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn(phases[name])
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    out = dict(shape=dict(S=S, B=B, T=T, n_components=k, q=q, test_split=n, cv_perm=P), reps=args.reps,
               host_residualisation_s_not_counted=round(host_resid_s, 4))
    for name in calls:
        out[name] = dict(wall_s=round(float(np.median(times[name])), 4), wall_s_all=[round(t, 4) for t in times[name]],
                         phase_ms={key: round(v / args.reps, 2) for key, v in phases[name].items()})
    out['ratio_with_confounds_to_host_residuals'] = round(out['with_confounds']['wall_s'] /
                                                          out['host_residuals_no_keyword']['wall_s'], 4)
    # the kernel-class split of (i): event timing on, a run of its own
    eng.set_timing(True)
    calls['with_confounds']()
    torch.cuda.synchronize()
    kt = eng.kernel_timing()
    eng.set_timing(False)
    eng.close()
    out['kernel_ms_with_confounds'] = {key: [round(v[0], 3), v[1]] for key, v in kt.items()}
    if 'k_cf_resid' in kt:
        out['k_cf_resid_GBps'] = round(3 * 8.0 * S * (B + T) / (1e6 * kt['k_cf_resid'][0]), 1)
    if 'k_cf_fold_K' in kt:
        # (one launch per entry call forms the K_s of all n splits: the observed entry once, the permuted one once per
        # call of the front end's loop over the permutations)
        out['k_cf_fold_K_written_GBps'] = round(kt['k_cf_fold_K'][1] * n * 8.0 * S * S / (1e6 * kt['k_cf_fold_K'][0]), 1)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
