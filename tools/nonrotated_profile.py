"""Time non-rotated PLS (plsx_set_contrasts) against the ordinary SVD legs and write profiles/nonrotated_<shape>.json.

    python tools/nonrotated_profile.py [--shape c4|c3|quick] [--reps 3] [--n 1008] [--out DIR] [--once]

Shapes: c4 (behavioral, 500 x 200 000, T' = 50) and c3 (mean-centred, 200 x 50 000, groups [25] * 4, 2 conditions,
T' = 8), three orthonormal contrasts each; ``quick`` is a rehearsal size.  Per shape, in ONE process and on two
fixed-budget engines -- the feature pass (option no_dual_perm) and the library's default routes -- ``--n`` permutations
and ``--n`` bootstraps are run with the contrasts set and in SVD mode, alternated ``--reps`` times after one warm-up
round of both.  A leg is the wall time between two device synchronisations around the C-ABI call(s) of the leg
(plsx_perm_batch; plsx_boot_begin / _batch / _finish); the index rows are on the device before the clock starts.

The JSON holds every time, the medians, and per leg the run-to-run spread (max - min over its repetitions, the larger
of the two modes): the condition of the change is ``contrast median <= ordinary median + spread`` for every leg
("no_slower").  Kernel classes of one contrast round (plsx_kernel_timing) are recorded for orientation only.

``--once``: one warm round and one more contrast round on the feature-pass engine, no JSON: the program to put behind
``rocprofv3 --kernel-trace --stats --`` in a run of its own.  k_contrast_norms reads 8 T'pp Bpad bytes per resample
(printed as ``norms_bytes_per_resample``); its time comes from that trace."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    'c4': dict(method='behavioral', groups=[500], n_cond=1, B=200000, T=50),
    'c3': dict(method='meancentered', groups=[25, 25, 25, 25], n_cond=2, B=50000, T=0),
    'quick': dict(method='behavioral', groups=[40, 40], n_cond=1, B=3000, T=5),
}


def make(shape, n):
    from pypyls_amd import resampling
    cfg = SHAPES[shape]
    rs = np.random.RandomState(0)
    S = sum(cfg['groups']) * cfg['n_cond']
    X = rs.randn(S, cfg['B'])
    Y = rs.randn(S, cfg['T']) + 0.2 * X[:, :1] if cfg['method'] == 'behavioral' else None
    cells = resampling.cell_of_row(cfg['groups'], cfg['n_cond'])
    perms = np.stack([rs.permutation(S) for _ in range(n)]).astype(np.int32)            # (n, S) rows
    boots = np.zeros((n, S), dtype=np.int32)
    for c in range(int(cells.max()) + 1):
        rows = np.flatnonzero(cells == c)
        boots[:, rows] = rows[rs.randint(0, rows.size, size=(n, rows.size))]
    Tp = len(cfg['groups']) * cfg['n_cond'] * (cfg['T'] if cfg['method'] == 'behavioral' else 1)
    V = np.linalg.qr(rs.randn(Tp, 3))[0]
    return cfg, X, Y, cells, perms, boots, V


def run(shape, n, reps, once):
    import torch
    from pypyls_amd.engine import Engine
    cfg, X, Y, cells, perms, boots, V = make(shape, n)
    engines = {'feature_pass': Engine(scratch_gb=40.0, options={'no_dual_perm': 1})}
    if not once:
        engines['default_routes'] = Engine(scratch_gb=40.0)
    out = {}
    try:
        for route, eng in engines.items():
            eng.set_data(X, Y, cells, len(cfg['groups']), cfg['n_cond'], 0 if cfg['method'] == 'behavioral' else 1)
            d_perm, d_boot = eng.rows_tensor(perms), eng.rows_tensor(boots)
            sv_out = eng._zeros((n, eng.L))
            dist = eng._zeros((n, eng.Tp, eng.L))

            def bind(contrast):
                eng.set_contrasts(V if contrast else None)
                xw, sv, yw = eng.decompose_dev()
                if not contrast:
                    eng.svd_flip(xw, yw)
                eng.set_original(xw, sv, yw)

            def timed(fn):
                torch.cuda.synchronize(eng.device)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(eng.device)
                return 1e3 * (time.perf_counter() - t0)

            def boot_leg():
                usum, usq = eng._zeros((eng.B, eng.L)), eng._zeros((eng.B, eng.L))
                torch.cuda.synchronize(eng.device)
                t0 = time.perf_counter()
                eng.boot_begin(n)
                eng.boot_into(d_boot, usum, usq, dist)
                eng.boot_finish(usum, usq)
                torch.cuda.synchronize(eng.device)
                return 1e3 * (time.perf_counter() - t0)

            times = {m + '_' + leg: [] for m in ('contrast', 'ordinary') for leg in ('perm', 'boot')}
            classes = None
            for rep in range(2 if once else reps + 1):
                for mode in ('contrast', 'ordinary'):
                    if once and mode == 'ordinary':
                        continue
                    bind(mode == 'contrast')
                    eng.set_timing(rep == 1 and mode == 'contrast')
                    t_perm = timed(lambda: eng.perm_into(d_perm, sv_out))
                    t_boot = boot_leg()
                    if rep == 1 and mode == 'contrast':
                        classes = {k: (round(v[0], 3), v[1]) for k, v in eng.kernel_timing().items()}
                        eng.set_timing(False)
                    eng.sync()
                    if rep:                                # (round 0 maps the scratch and forms K: warm-up)
                        times[mode + '_perm'].append(t_perm)
                        times[mode + '_boot'].append(t_boot)
            rec = dict(dual_perm=bool(eng.last_timing()['dual_perm']), kernel_classes_contrast_round=classes,
                       norms_bytes_per_resample=8.0 * (4 * ((eng.Tp + 3) // 4)) * (128 * ((eng.B + eng.L + 127) // 128)))
            for leg in ('perm', 'boot'):
                c, o = times['contrast_' + leg], times['ordinary_' + leg]
                if not o:
                    continue
                spread = max(max(c) - min(c), max(o) - min(o))
                rec[leg] = dict(contrast_ms=[round(v, 3) for v in c], ordinary_ms=[round(v, 3) for v in o],
                                contrast_median_ms=round(float(np.median(c)), 3),
                                ordinary_median_ms=round(float(np.median(o)), 3), spread_ms=round(spread, 3),
                                no_slower=bool(np.median(c) <= np.median(o) + spread))
            out[route] = rec
    finally:
        for eng in engines.values():
            eng.close()
    return dict(shape=dict(name=shape, S=X.shape[0], B=X.shape[1], Tp=int(V.shape[0]), Lc=3, n_perm=n, n_boot=n),
                reps=reps, routes=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='c4', choices=sorted(SHAPES))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--n', type=int, default=1008)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    rec = run(args.shape, args.n, max(args.reps, 3), args.once)
    print(json.dumps(rec), flush=True)
    if args.once:
        return
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'nonrotated_{}.json'.format(args.shape)), 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
