"""Time multiblock_pls against behavioral_pls on the same general route and write profiles/multiblock_<shape>.json.

    python tools/multiblock_profile.py [--shape c4|quick] [--reps 3] [--n 1008] [--out DIR] [--commit ID]

Shape c4: X 500 x 200 000, T = 24 behaviours, two cells (groups [250, 250], one condition: T' = 2 + 48 = 50),
``--n`` permutations and ``--n`` bootstraps; ``quick`` is a rehearsal size.  In ONE process, on ONE fixed-budget engine
with the options no_fixed_x, no_dual_perm, no_compact_boot -- under which behavioral_pls takes the general feature-pass
route multiblock PLS always takes (run_xprod -> run_gram -> run_small, and run_urot for the bootstraps) -- the two
public calls are alternated ``--reps`` times after one warm-up round of both, with the same seeded index arrays.
Recorded per call: the wall time and the per-phase wall times of the front-end (each phase ends in a device
synchronisation).  One further round of each with event timing on gives the per-kernel-class times
(plsx_kernel_timing); from the multiblock round: the normalisation pass's share of the kernel time and of the two
resampling phases, and its achieved bytes/s against the model of 3 x 8 x T'pp x Bpad bytes per resample (one read for
the norms, one read and one write for the scaling).  No pass / fail threshold: the numbers are written down with the
shape and the commit."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    'c4': dict(groups=[250, 250], n_cond=1, B=200000, T=24),
    'quick': dict(groups=[40, 40], n_cond=1, B=3000, T=5),
}
OPTIONS = {'no_fixed_x': 1, 'no_dual_perm': 1, 'no_compact_boot': 1}


def make(shape, n):
    from pypyls_amd import resampling
    cfg = SHAPES[shape]
    rs = np.random.RandomState(0)
    S = sum(cfg['groups']) * cfg['n_cond']
    cells = resampling.cell_of_row(cfg['groups'], cfg['n_cond'])
    X = rs.randn(S, cfg['B'])
    X[:, :cfg['B'] // 10] += 0.5 * cells[:, None]               # a task effect in a tenth of the features
    Y = rs.randn(S, cfg['T']) + 0.2 * X[:, -1:]
    perms = resampling.gen_permsamp(cfg['groups'], cfg['n_cond'], seed=1, n_perm=n)
    boots = resampling.gen_bootsamp(cfg['groups'], cfg['n_cond'], seed=2, n_boot=n)
    return cfg, X, Y, perms, boots


def commit_id():
    try:
        out = subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True, timeout=10)
        return out.stdout.strip() or 'unknown'
    except (OSError, subprocess.SubprocessError):
        return 'unknown'


def run(shape, n, reps):
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    cfg, X, Y, perms, boots = make(shape, n)
    eng = Engine(scratch_gb=40.0, options=OPTIONS)
    kw = dict(groups=cfg['groups'], n_cond=cfg['n_cond'], n_perm=n, n_boot=n, permsamples=perms, bootsamples=boots,
              verbose=False, _engine=eng)

    def call(method, timing=False):
        phases = {}
        eng.set_timing(timing)
        torch.cuda.synchronize(eng.device)
        t0 = time.perf_counter()
        if method == 'multiblock':
            res = pls.multiblock_pls(X, Y, mean_centering=1, _phases=phases, **kw)
        else:
            res = pls.behavioral_pls(X, Y, test_split=0, _phases=phases, **kw)
        torch.cuda.synchronize(eng.device)
        wall = 1e3 * (time.perf_counter() - t0)
        classes = {k: [round(v[0], 3), v[1]] for k, v in eng.kernel_timing().items()} if timing else None
        eng.set_timing(False)
        return res, wall, {k: round(v, 3) for k, v in phases.items()}, classes

    rec = {m: dict(wall_ms=[], phases_ms=[]) for m in ('multiblock', 'behavioral')}
    try:
        for rep in range(reps + 1):
            for method in ('multiblock', 'behavioral'):
                res, wall, phases, _ = call(method)
                if rep:                                         # (round 0 maps the scratch: warm-up)
                    rec[method]['wall_ms'].append(round(wall, 3))
                    rec[method]['phases_ms'].append(phases)
                rec[method]['Tp'] = int(res['y_weights'].shape[0])
                rec[method]['top_singvals'] = [float(v) for v in res['singvals'][:3]]
        for method in ('multiblock', 'behavioral'):
            _, wall, phases, classes = call(method, timing=True)
            lt = eng.last_timing()                              # (the layout of the method's last cross-product launch)
            rec[method]['timed_round'] = dict(wall_ms=round(wall, 3), phases_ms=phases, kernel_classes_ms=classes,
                                              superbatch=int(lt['superbatch']),
                                              resamples_per_group=int(lt['resamples_per_group']))
        Tp, L, B = rec['multiblock']['Tp'], min(rec['multiblock']['Tp'], X.shape[1]), X.shape[1]
    finally:
        eng.close()
    for method in rec:
        w = rec[method]['wall_ms']
        rec[method]['wall_median_ms'] = round(float(np.median(w)), 3)
        rec[method]['wall_spread_ms'] = round(max(w) - min(w), 3)
        keys = rec[method]['phases_ms'][0].keys()
        rec[method]['phases_median_ms'] = {k: round(float(np.median([p[k] for p in rec[method]['phases_ms']])), 3)
                                           for k in keys}
    tr = rec['multiblock']['timed_round']
    kc = tr['kernel_classes_ms']
    norm_ms, norm_launches = kc.get('k_mb_rownorm', [0.0, 0])
    tpp, bpad = 4 * ((Tp + 3) // 4), 128 * ((B + L + 127) // 128)
    resamples = 2 * n + 1                                       # (every permutation and bootstrap, the original once)
    model_bytes = 3.0 * 8.0 * tpp * bpad * resamples
    kernel_total = sum(v[0] for v in kc.values())
    resampling_ms = tr['phases_ms'].get('permutations', 0.0) + tr['phases_ms'].get('bootstraps', 0.0)
    normalisation = dict(
        ms=norm_ms, launches=norm_launches, resamples=resamples, model_bytes_per_resample=3.0 * 8.0 * tpp * bpad,
        model_gb=round(model_bytes / 1e9, 3),
        achieved_tb_per_s=round(model_bytes / (norm_ms * 1e-3) / 1e12, 3) if norm_ms > 0 else None,
        share_of_kernel_time=round(norm_ms / kernel_total, 4) if kernel_total > 0 else None,
        share_of_resampling_phases=round(norm_ms / resampling_ms, 4) if resampling_ms > 0 else None,
        note='event times of the timed round; the model counts one read for the norms, one read and one write for '
             'the scaling')
    return dict(shape=dict(name=shape, S=X.shape[0], B=B, T=cfg['T'], groups=cfg['groups'], n_cond=cfg['n_cond'],
                           Tp_multiblock=Tp, Tp_behavioral=rec['behavioral']['Tp'], n_perm=n, n_boot=n),
                options=OPTIONS, scratch_gb=40.0, reps=reps, methods=rec, normalisation=normalisation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='c4', choices=sorted(SHAPES))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--n', type=int, default=1008)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    ap.add_argument('--commit', default=None, help='recorded as is (default: git rev-parse HEAD, or "unknown")')
    args = ap.parse_args()
    rec = run(args.shape, args.n, max(args.reps, 2))
    rec['commit'] = args.commit or commit_id()
    print(json.dumps(rec), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'multiblock_{}.json'.format(args.shape)), 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
