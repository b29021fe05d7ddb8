"""Time pls_regression(coef_components=c, coef_ci=True) at BASELINE config 5's shape and write profiles/coef_ci_c5.json.

    python tools/coef_ci_profile.py [--reps 5] [--out profiles/coef_ci_c5.json] [--quick] [--once]

S = 1000, B = 100 000, T = 20, k = 15, c = 7, n_boot = 5000, n_perm = 0 on one GPU, a fixed-budget engine: one
warm-up call of each kind, then ``--reps`` timed calls with and without ``coef_ci``, alternating; medians.  Event
timing per kernel class (plsx_kernel_timing): k_coef_prod (the feature pass, 2 B S T n flop), k_percentile (the
selection), k_nt_gemm with its own flop count for comparison, against plsx_mfma_f64_peak of the same run.  The wall
time of the closing pass is the front-end's phase ``coefs_ci`` (ends in a device synchronise).  Device memory in use
after a call of each kind (total - free: library buffers and torch's cache stay allocated, so this is the high-water
mark of the call).  ``--once``: a single warm call with the keyword and no JSON, the program to put behind
``rocprofv3 --kernel-trace --stats --`` in a run of its own.  ``--quick``: B = 2000, n_boot = 600 (a rehearsal)."""
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coef_ci_c5.json'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, B, T, k, c, n = (1000, 2000, 20, 15, 7, 600) if args.quick else (1000, 100000, 20, 15, 7, 5000)
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=0, n_boot=n, coef_components=c, seed=1, verbose=False, _engine=eng)

    def call(flag):
        phases = {}
        torch.cuda.synchronize()
        eng.set_timing(True)
        t0 = time.perf_counter()
        res = pls.pls_regression(X, Y, coef_ci=flag, _phases=phases, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kt = eng.kernel_timing()
        flops = eng.last_timing().get('nt_flops', 0.0)
        eng.set_timing(False)
        free, total = torch.cuda.mem_get_info(eng.device)
        return dict(wall_s=wall, phases=phases, kt=kt, nt_flops=flops, in_use_gb=(total - free) / 2 ** 30), res

    call(False)
    mem_without = call(False)[0]['in_use_gb']            # (before the first call with the keyword allocates anything)
    call(True)
    if args.once:
        return
    runs = {False: [], True: []}
    for _ in range(args.reps):
        for flag in (False, True):
            runs[flag].append(call(flag)[0])
    peak = eng.mfma_f64_peak()

    def med(flag, fn):
        return float(np.median([fn(r) for r in runs[flag]]))
    prod_ms = med(True, lambda r: r['kt'].get('k_coef_prod', (0.0, 0))[0])
    sel_ms = med(True, lambda r: r['kt'].get('k_percentile', (0.0, 0))[0]) - \
        med(False, lambda r: r['kt'].get('k_percentile', (0.0, 0))[0])
    nt_ms = med(True, lambda r: r['kt'].get('k_nt_gemm', (0.0, 0))[0])
    nt_flops = med(True, lambda r: r['nt_flops'])
    flop = 2.0 * B * S * T * n
    out = dict(
        shape=dict(S=S, B=B, T=T, n_components=k, coef_components=c, n_boot=n, n_perm=0), reps=args.reps,
        wall_s_without=round(med(False, lambda r: r['wall_s']), 4), wall_s_with=round(med(True, lambda r: r['wall_s']), 4),
        wall_s_all_without=[round(r['wall_s'], 4) for r in runs[False]],
        wall_s_all_with=[round(r['wall_s'], 4) for r in runs[True]],
        closing_pass_wall_ms=round(med(True, lambda r: r['phases'].get('coefs_ci', 0.0)), 2),
        k_coef_prod_ms=round(prod_ms, 2), k_coef_prod_launches=runs[True][0]['kt'].get('k_coef_prod', (0.0, 0))[1],
        k_percentile_ms_added=round(sel_ms, 2),
        k_coef_prod_flop=flop, k_coef_prod_tflops=round(flop / (prod_ms * 1e9), 2) if prod_ms > 0 else None,
        k_nt_gemm_ms=round(nt_ms, 2), k_nt_gemm_tflops=round(nt_flops / (nt_ms * 1e9), 2) if nt_ms > 0 else None,
        mfma_f64_peak_tflops=round(peak, 1),
        series_bytes_written_and_reread=2.0 * 8 * B * T * n, kept_stack_bytes=8.0 * n * T * S,
        device_mem_in_use_gb_without=round(mem_without, 2),
        device_mem_in_use_gb_with=round(max(r['in_use_gb'] for r in runs[True]), 2),
        kernel_ms_with={key: round(v[0], 2) for key, v in runs[True][-1]['kt'].items()},
        kernel_ms_without={key: round(v[0], 2) for key, v in runs[False][-1]['kt'].items()})
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
