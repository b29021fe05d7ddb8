"""Time the closing pass of pls_regression(vip_components=c) (plsx_simpls_vip_ci) and write profiles/vip_c5.json.

    python tools/vip_profile.py [--reps 5] [--out profiles/vip_c5.json] [--quick] [--once]

Two legs on one GPU, a fixed-budget engine, random data and a random stack (the pass does not care where its stack comes
from), one warm-up call and ``--reps`` timed calls each, medians:
  * S = 1000, c = 15, n = 5000, B = 600: event timing per kernel class (plsx_kernel_timing) -- k_coef_prod, under which
    k_vip_prod and k_vip_moments count (2 B S c n flop), and k_percentile (the selection) -- against
    plsx_mfma_f64_peak of the same run;
  * the same stack at the largest B of BASELINE config 5 that fits (B = 100 000 unless ``--b-large`` says otherwise): the
    whole closing pass, wall time between device synchronisations, its chunks and its kernel classes.
Time model: 2 B S c n flop (1.5e13 at c5, about 0.2 s at 72 TF/s) plus 16 B n bytes of series written and re-read.
``--once``: a single warm call of the large leg and no JSON, the program to put behind
``rocprofv3 --kernel-trace --stats --`` in a run of its own.  ``--quick``: n = 600, B = 2000 for the large leg (a
rehearsal)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(S, B, c, n, reps, once=False):
    import torch
    from pypyls_amd.engine import Engine
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = rs.randn(S, 2)
    eng = Engine(scratch_gb=48.0)
    try:
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), 2)
        stack = torch.randn((n, c, S), dtype=torch.float64, device=eng.device)
        runs = []
        for rep in range(1 if once else reps + 1):
            torch.cuda.synchronize()
            eng.set_timing(True)
            t0 = time.perf_counter()
            eng.simpls_vip_ci(stack, ci=95)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            kt = eng.kernel_timing()
            eng.set_timing(False)
            if rep:                                    # (the first call allocates the chunk: warm-up)
                runs.append(dict(wall_ms=1e3 * wall, kt=kt))
        if once:
            return None
        peak = eng.mfma_f64_peak()
        free, total = torch.cuda.mem_get_info(eng.device)
    finally:
        eng.close()

    def med(fn):
        return float(np.median([fn(r) for r in runs]))
    prod_ms = med(lambda r: r['kt'].get('k_coef_prod', (0.0, 0))[0])
    sel_ms = med(lambda r: r['kt'].get('k_percentile', (0.0, 0))[0])
    flop = 2.0 * B * S * c * n
    return dict(shape=dict(S=S, B=B, c=c, n=n), reps=reps,
                closing_pass_wall_ms=round(med(lambda r: r['wall_ms']), 2),
                closing_pass_wall_ms_all=[round(r['wall_ms'], 2) for r in runs],
                chunks=runs[0]['kt'].get('k_coef_prod', (0.0, 0))[1],
                k_vip_prod_and_moments_ms=round(prod_ms, 3), k_percentile_ms=round(sel_ms, 3),
                flop=flop, tflops=round(flop / (prod_ms * 1e9), 2) if prod_ms > 0 else None,
                mfma_f64_peak_tflops=round(peak, 1), series_bytes=8.0 * B * n, stack_bytes=8.0 * n * c * S,
                device_mem_in_use_gb=round((total - free) / 2 ** 30, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vip_c5.json'))
    ap.add_argument('--b-large', type=int, default=100000)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    S, c, n = 1000, 15, 600 if args.quick else 5000
    b_large = 2000 if args.quick else args.b_large
    if args.once:
        leg(S, b_large, c, n, 1, once=True)
        return
    out = dict(model='2 B S c n flop + 16 B n bytes of series', small=leg(S, 600, c, n, args.reps),
               large=leg(S, b_large, c, n, args.reps))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
