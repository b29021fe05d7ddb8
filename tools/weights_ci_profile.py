"""Time behavioral_pls(weights_ci=m) at the headline shape and write profiles/weights_ci_c4.json.

    python tools/weights_ci_profile.py [--reps 3] [--out profiles/weights_ci_c4.json] [--quick] [--once]

S = 500, B = 200 000, T' = 50 (one cell, 50 behaviours), n_boot = 5000, n_perm = 0 on one GPU, a fixed-budget engine.
For correlation mode and for ``covariance=True`` (null scale table), with m = 3 and m = 50: one warm-up call of each
kind, then ``--reps`` timed calls with and without ``weights_ci``, alternating; medians.  Event timing per kernel class
(plsx_kernel_timing): k_weights_prod (the feature pass, 2 B S m n flop), k_xprod_moments (the scale table: nothing else
counts there on a bootstrap-only call), k_percentile (the selection, less the share of ``y_loadings_ci``), k_build_A
(operand builders, k_weights_W, the kept operands), against plsx_mfma_f64_peak of the same run.  The wall time of the
closing pass is the front-end's phase ``weights_ci`` (ends in a device synchronise).  ``--once``: a single warm call
with the keyword (correlation mode, m = 50) and no JSON, the program to put behind ``rocprofv3 --kernel-trace --stats
--`` in a run of its own.  ``--quick``: B = 4000, n_boot = 600 (a rehearsal)."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weights_ci_c4.json'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, B, T, n = (500, 4000, 50, 600) if args.quick else (500, 200000, 50, 5000)
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    eng = Engine(scratch_gb=48.0)

    def call(m, covariance):
        phases = {}
        kw = dict(n_perm=0, n_boot=n, test_split=0, covariance=covariance, seed=1, verbose=False, _engine=eng,
                  _phases=phases)
        if m:
            kw['weights_ci'] = m
        torch.cuda.synchronize()
        eng.set_timing(True)
        t0 = time.perf_counter()
        pls.behavioral_pls(X, Y, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kt = eng.kernel_timing()
        eng.set_timing(False)
        return dict(wall_s=wall, phases=phases, kt=kt)

    if args.once:
        call(50, False)
        call(50, False)
        return
    out = dict(shape=dict(S=S, B=B, Tp=T, cells=1, n_boot=n, n_perm=0), reps=args.reps, modes={})
    for covariance in (False, True):
        for m in (3, 50):
            call(0, covariance)
            call(m, covariance)
            runs = {0: [], m: []}
            for _ in range(args.reps):
                for flag in (0, m):
                    runs[flag].append(call(flag, covariance))

            def med(flag, fn):
                return float(np.median([fn(r) for r in runs[flag]]))

            def kms(flag, name):
                return med(flag, lambda r: r['kt'].get(name, (0.0, 0))[0])
            prod_ms = kms(m, 'k_weights_prod')
            flop = 2.0 * B * S * m * n
            out['modes']['{}_m{}'.format('covariance' if covariance else 'correlation', m)] = dict(
                wall_s_without=round(med(0, lambda r: r['wall_s']), 4), wall_s_with=round(med(m, lambda r: r['wall_s']), 4),
                wall_s_all_without=[round(r['wall_s'], 4) for r in runs[0]],
                wall_s_all_with=[round(r['wall_s'], 4) for r in runs[m]],
                closing_pass_wall_ms=round(med(m, lambda r: r['phases'].get('weights_ci', 0.0)), 2),
                chunks=runs[m][0]['kt'].get('k_weights_prod', (0.0, 0))[1],
                k_weights_prod_ms=round(prod_ms, 2), k_weights_prod_flop=flop,
                k_weights_prod_tflops=round(flop / (prod_ms * 1e9), 2) if prod_ms > 0 else None,
                scale_table_ms=round(kms(m, 'k_xprod_moments') - kms(0, 'k_xprod_moments'), 2),
                k_percentile_ms_added=round(kms(m, 'k_percentile') - kms(0, 'k_percentile'), 2),
                builders_ms_added=round(kms(m, 'k_build_A') - kms(0, 'k_build_A'), 2),
                series_bytes_written_and_reread=2.0 * 8 * B * m * n, kept_stack_bytes=8.0 * n * m * T,
                kernel_ms_with={key: round(v[0], 2) for key, v in runs[m][-1]['kt'].items()})
            print(json.dumps({k: v for k, v in out['modes'].items()}), flush=True)
    out['mfma_f64_peak_tflops'] = round(eng.mfma_f64_peak(), 1)
    out['k_coef_prod_tflops_recorded_at_B_100000'] = 53.0
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
