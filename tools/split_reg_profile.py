"""Time the split-half reliability of pls_regression (n_split) at BASELINE config 5's solver shape and write
profiles/split_reg_c5.json.

    python tools/split_reg_profile.py [--reps 3] [--out profiles/split_reg_c5.json] [--quick]
                                      [--baseline-only] [--parent-baseline FILE] [--root DIR]

S = 1000, B = 100 000, T = 20, k = 15, n_split = 100, n_perm = 1000, n_boot = 0 on one GPU, a fixed-budget engine.  Every
leg is one warm-up call and then ``--reps`` timed calls bracketed by device synchronisation; medians, every repeat kept.

1. The baseline: the public call with ``n_split=0``.  This leg uses only what the package had before n_split existed:
   ``--baseline-only`` runs it alone and ``--root DIR`` imports the package from another checkout (the parent
   commit's), so the same program measures both sides; ``--parent-baseline FILE`` copies the parent's record into the
   output.
2. The public call with ``n_split=100`` and the wall time of its split-half leg (``_phases``).
3. plsx_simpls_split_half_batch on the 1000 permutations in the front-end's blocks of 128 arrangements with event
   timing on (a run of its own): the kernel-class split, and beside it plsx_simpls_perm_batch on the same blocks -- the
   solver's own share of k_nt_gemm, which the difference removes.  The products with K are 4 S^2 k flop per split.

``--quick``: B = 2000, n_split = 10, n_perm = 64 (a rehearsal)."""
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
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--parent-baseline', default=None)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    out_path = args.out or os.path.join(root, 'profiles', 'split_reg_c5.json')
    S, B, T, k, ns, P = (1000, 2000, 20, 15, 10, 64) if args.quick else (1000, 100000, 20, 15, 100, 1000)
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)

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

    def write(out):
        print(json.dumps(out), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')

    # ---- 1. the baseline: the same call without split-half
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=k, n_perm=P, n_boot=0, seed=1, verbose=False, _engine=eng)
    ts0 = timed(lambda: pls.pls_regression(X, Y, **kw), args.reps)
    out = dict(shape=dict(S=S, B=B, T=T, n_components=k, n_split=ns, n_perm=P), reps=args.reps,
               public_call_without=dict(wall_s=round(float(np.median(ts0)), 4), wall_s_all=[round(t, 4) for t in ts0]))
    if args.baseline_only:
        eng.close()
        return write(out)
    if args.parent_baseline:
        with open(args.parent_baseline) as fh:
            out['public_call_without_parent_commit'] = json.load(fh)['public_call_without']

    # ---- 2. the public call with split-half
    phases = {}
    ts = timed(lambda: pls.pls_regression(X, Y, n_split=ns, _phases=phases, **kw), args.reps)
    out['public_call_with'] = dict(wall_s=round(float(np.median(ts)), 4), wall_s_all=[round(t, 4) for t in ts],
                                   split_half_phase_ms=round(phases.get('split_half', 0.0) / (len(ts) + 1), 2))
    eng.close()

    # ---- 3. the entry on the front-end's blocks, event timing on
    eng = Engine(scratch_gb=48.0)
    eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)
    perms = rsmp.gen_permsamp([S], 1, P, seed=7, verbose=False)
    blocks = []
    for a in range(0, P, 128):
        b = min(P, a + 128)
        m = rsmp.gen_splits_seeded([S], 1, ns, np.arange(a, b), test_size=0.5, rows=True, warn=False)[0]
        blocks.append((eng.rows_tensor(perms[:, a:b].T), torch.from_numpy(m).to(eng.device),
                       eng._empty((b - a, ns, k)), eng._empty((b - a, ns, k)), eng._empty((b - a, k))))

    def split_leg():
        for dp, dm, uc, vc, _ in blocks:
            eng.simpls_split_half_into(dp, dm, uc, vc)

    def solver_leg():
        for dp, _, _, _, pv in blocks:
            eng.simpls_perm_into(dp, pv)

    tl = timed(split_leg, args.reps)
    out['entry_blocks_of_128'] = dict(wall_s=round(float(np.median(tl)), 4), wall_s_all=[round(t, 4) for t in tl])
    for name, fn in (('kernel_ms_split_half', split_leg), ('kernel_ms_solver_alone', solver_leg)):
        fn()
        eng.sync()
        eng.set_timing(True)
        fn()
        eng.sync()
        out[name] = {key: [round(v[0], 2), v[1]] for key, v in eng.kernel_timing().items()}
        eng.set_timing(False)
    eng.close()
    flop = 4.0 * S * S * k * ns * P
    nt = out['kernel_ms_split_half'].get('k_nt_gemm', [0.0, 0])[0] - out['kernel_ms_solver_alone'].get('k_nt_gemm', [0.0, 0])[0]
    out['k_products'] = dict(flop=flop, k_nt_gemm_ms=round(nt, 2), tflops=round(flop / (nt * 1e-3) / 1e12, 2) if nt > 0 else None)
    write(out)


if __name__ == '__main__':
    main()
