"""Time pls_regression(coef_components=c, coef_perm=True) against the same permutation leg without the series and write
profiles/coef_perm_c5.json.

    python tools/coef_perm_profile.py [--reps 3] [--out profiles/coef_perm_c5.json] [--quick] [--no-wide] [--once]

S = 1000, T = 20, k = 15, c = 6, n_perm = 5000, n_boot = 0 on one GPU, a fixed-budget engine, at B = 600 and -- unless
``--no-wide`` -- B = 100 000: one warm-up call of each kind, then ``--reps`` timed calls with and without ``coef_perm``,
alternating; medians.  Event timing per kernel class (plsx_kernel_timing): k_coef_prod is the class of the feature
pass (k_coef_perm_prod with k_coef_perm_max and k_col_sd: 2 B S T n_perm flop), k_sd_coef the A_p of the permutations,
k_simpls_dual the solver (weights on with the series, off without), against plsx_mfma_f64_peak of the same run.  The wall
time of the permutation leg is the front-end's phase ``permutations`` (ends in a device synchronise); ``coefs_perm`` is
the set-up of the series.  ``--once``: a single warm call with the keyword at the first shape and no JSON, the program to
put behind ``rocprofv3 --kernel-trace --stats --`` in a run of its own.  ``--quick``: n_perm = 600 (a rehearsal)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def profile(B, n, reps, once):
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, T, k, c = 1000, 20, 15, 6
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=n, n_boot=0, coef_components=c, seed=1, verbose=False, _engine=eng)

    def call(flag):
        phases = {}
        torch.cuda.synchronize()
        eng.set_timing(True)
        t0 = time.perf_counter()
        pls.pls_regression(X, Y, coef_perm=flag, _phases=phases, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kt = eng.kernel_timing()
        eng.set_timing(False)
        free, total = torch.cuda.mem_get_info(eng.device)
        return dict(wall_s=wall, phases=phases, kt=kt, in_use_gb=(total - free) / 2 ** 30)

    try:
        call(False)
        mem_without = call(False)['in_use_gb']           # (before the first call with the keyword allocates anything)
        call(True)
        if once:
            return None
        runs = {False: [], True: []}
        for _ in range(reps):
            for flag in (False, True):
                runs[flag].append(call(flag))
        peak = eng.mfma_f64_peak()
    finally:
        eng.close()

    def med(flag, fn):
        return float(np.median([fn(r) for r in runs[flag]]))

    def cls(name):
        return lambda r: r['kt'].get(name, (0.0, 0))[0]
    prod_ms = med(True, cls('k_coef_prod'))
    flop = 2.0 * B * S * T * n
    return dict(
        shape=dict(S=S, B=B, T=T, n_components=k, coef_components=c, n_perm=n, n_boot=0), reps=reps,
        wall_s_without=round(med(False, lambda r: r['wall_s']), 4), wall_s_with=round(med(True, lambda r: r['wall_s']), 4),
        wall_s_all_without=[round(r['wall_s'], 4) for r in runs[False]],
        wall_s_all_with=[round(r['wall_s'], 4) for r in runs[True]],
        permutations_phase_ms_without=round(med(False, lambda r: r['phases'].get('permutations', 0.0)), 2),
        permutations_phase_ms_with=round(med(True, lambda r: r['phases'].get('permutations', 0.0)), 2),
        coefs_perm_setup_ms=round(med(True, lambda r: r['phases'].get('coefs_perm', 0.0)), 2),
        host_finish_ms_without=round(med(False, lambda r: r['phases'].get('host_finish', 0.0)), 2),
        host_finish_ms_with=round(med(True, lambda r: r['phases'].get('host_finish', 0.0)), 2),
        feature_pass_ms=round(prod_ms, 2), feature_pass_brackets=runs[True][0]['kt'].get('k_coef_prod', (0.0, 0))[1],
        feature_pass_flop=flop, feature_pass_tflops=round(flop / (prod_ms * 1e9), 2) if prod_ms > 0 else None,
        k_sd_coef_ms=round(med(True, cls('k_sd_coef')), 2),
        k_simpls_dual_ms_without=round(med(False, cls('k_simpls_dual')), 2),
        k_simpls_dual_ms_with=round(med(True, cls('k_simpls_dual')), 2),
        mfma_f64_peak_tflops=round(peak, 1),
        device_mem_in_use_gb_without=round(mem_without, 2),
        device_mem_in_use_gb_with=round(max(r['in_use_gb'] for r in runs[True]), 2),
        kernel_ms_with={key: round(v[0], 2) for key, v in runs[True][-1]['kt'].items()},
        kernel_ms_without={key: round(v[0], 2) for key, v in runs[False][-1]['kt'].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coef_perm_c5.json'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--no-wide', action='store_true')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    n = 600 if args.quick else 5000
    out = {}
    for B in (600,) if (args.no_wide or args.once) else (600, 100000):
        got = profile(B, n, args.reps, args.once)
        if got is None:
            return
        out['B{}'.format(B)] = got
        print(json.dumps({'B': B, **got}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
