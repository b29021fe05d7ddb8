"""Time behavioral_pls(weights_perm=m) at the headline shape and write profiles/weights_perm_c4.json.

    python tools/weights_perm_profile.py [--reps 3] [--out profiles/weights_perm_c4.json] [--quick] [--once]

S = 500, B = 200 000, T' = 50 (one cell, 50 behaviours), n_perm = 5000, n_boot = 0 on one GPU, a fixed-budget engine.
For correlation mode and for ``covariance=True``, with m = 3 and m = 50: one warm-up call of each kind, then ``--reps``
timed calls with and without ``weights_perm``, alternating; medians.  Event timing per kernel class
(plsx_kernel_timing): k_coef_prod is the class of the feature pass (k_coef_perm_prod with k_coef_perm_max and k_col_rsd:
2 B S m n_perm flop; nothing else counts there on a PLS-C call), k_build_A the operand builders (k_perm_W_behav, less the
permutation leg's own builders: the difference to the call without the keyword), against plsx_mfma_f64_peak of the same
run.  The wall time of the pass is the front-end's phase ``weights_perm`` (ends in a device synchronise).  Unless
``--no-coef-perm``, tools/coef_perm_profile.py's B = 100 000 shape (S = 1000, T = 20) is then timed in the same session
with one repetition, so that the rate of the same kernel on the SIMPLS coefficients stands next to it.  ``--once``: a
single warm call with the keyword (correlation mode, m = 50) and no JSON, the program to put behind ``rocprofv3
--kernel-trace --stats --`` in a run of its own.  ``--quick``: B = 4000, n_perm = 600 (a rehearsal)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weights_perm_c4.json'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--no-coef-perm', action='store_true')
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
        kw = dict(n_perm=n, n_boot=0, test_split=0, covariance=covariance, seed=1, verbose=False, _engine=eng,
                  _phases=phases)
        if m:
            kw['weights_perm'] = m
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
    out = dict(shape=dict(S=S, B=B, Tp=T, cells=1, n_perm=n, n_boot=0), reps=args.reps, modes={})
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
            prod_ms = kms(m, 'k_coef_prod')
            flop = 2.0 * B * S * m * n
            out['modes']['{}_m{}'.format('covariance' if covariance else 'correlation', m)] = dict(
                wall_s_without=round(med(0, lambda r: r['wall_s']), 4), wall_s_with=round(med(m, lambda r: r['wall_s']), 4),
                wall_s_all_without=[round(r['wall_s'], 4) for r in runs[0]],
                wall_s_all_with=[round(r['wall_s'], 4) for r in runs[m]],
                permutations_phase_ms_without=round(med(0, lambda r: r['phases'].get('permutations', 0.0)), 2),
                permutations_phase_ms_with=round(med(m, lambda r: r['phases'].get('permutations', 0.0)), 2),
                weights_perm_pass_wall_ms=round(med(m, lambda r: r['phases'].get('weights_perm', 0.0)), 2),
                host_finish_ms_without=round(med(0, lambda r: r['phases'].get('host_finish', 0.0)), 2),
                host_finish_ms_with=round(med(m, lambda r: r['phases'].get('host_finish', 0.0)), 2),
                feature_pass_brackets=runs[m][0]['kt'].get('k_coef_prod', (0.0, 0))[1],
                k_coef_perm_prod_ms=round(prod_ms, 2), k_coef_perm_prod_flop=flop,
                k_coef_perm_prod_tflops=round(flop / (prod_ms * 1e9), 2) if prod_ms > 0 else None,
                builders_ms=round(kms(m, 'k_build_A') - kms(0, 'k_build_A'), 2),
                operand_bytes=8.0 * n * m * S,
                kernel_ms_with={key: round(v[0], 2) for key, v in runs[m][-1]['kt'].items()},
                kernel_ms_without={key: round(v[0], 2) for key, v in runs[0][-1]['kt'].items()})
            print(json.dumps({k: v for k, v in out['modes'].items()}), flush=True)
    out['mfma_f64_peak_tflops'] = round(eng.mfma_f64_peak(), 1)
    eng.close()
    if not args.no_coef_perm:
        # the same kernel on the SIMPLS coefficients, in this session (S = 1000: twice the contraction depth per tile)
        import coef_perm_profile
        got = coef_perm_profile.profile(4000 if args.quick else 100000, n, 1, False)
        out['coef_perm_same_session'] = dict(shape=got['shape'], feature_pass_ms=got['feature_pass_ms'],
                                             feature_pass_tflops=got['feature_pass_tflops'])
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
