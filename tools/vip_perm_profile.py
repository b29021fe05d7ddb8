"""Time pls_regression(vip_components=c, vip_perm=True) against the same call without the keyword and write
profiles/vip_perm_c5.json.

    python tools/vip_perm_profile.py [--reps 3] [--out profiles/vip_perm_c5.json] [--quick] [--no-wide]
                                     [--parent-root DIR] [--without-only]

S = 1000, T = 20, k = c = 15, n_perm = 5000, n_boot = 0 on one GPU, a fixed-budget engine, at B = 600 and -- unless
``--no-wide`` -- B = 100 000: one warm-up call of each kind, then ``--reps`` timed calls with and without ``vip_perm``,
alternating; medians and every repetition.  Event timing per kernel class (plsx_kernel_timing): k_coef_prod is the class
of the feature pass (k_vip_perm_prod with k_coef_perm_max: 2 B S c n_perm flop), k_sd_coef the scaled dual weights of
the permutations (k_sd_vip), k_simpls_dual the solver (weights on with the series, off without), against
plsx_mfma_f64_peak of the same run.  The wall time of the permutation leg is the front-end's phase ``permutations``
(ends in a device synchronise); ``vip_perm`` is the set-up of the series.

The yardstick, in the same process on the same stack: a random stack (n_perm, c, S) goes through
plsx_simpls_vip_perm_test (k_vip_perm_prod + k_coef_perm_max) and through plsx_simpls_vip_ci (k_vip_prod + k_vip_moments
under the same class; its percentile selection is another class and is left out), alternating, ``--reps`` times each.

``--parent-root DIR``: a built tree of the parent commit.  Before this process touches the GPU, fresh child processes
run ``--without-only`` (the call WITHOUT the keyword, which the parent has too) alternately on this tree and on DIR; their
wall times go into the JSON as ``without_keyword_vs_parent``.  ``--quick``: n_perm = 600 (a rehearsal)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, T, K, C = 1000, 20, 15, 15


def _data(B):
    rs = np.random.RandomState(0)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    return X, Y


def without_only(B, n, reps):
    """The call without the keyword, as the parent commit has it: wall times of ``reps`` calls after one warm-up."""
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    X, Y = _data(B)
    eng = Engine(scratch_gb=48.0)
    try:
        walls = []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pls.pls_regression(X, Y, n_components=K, n_perm=n, n_boot=0, vip_components=C, seed=1, verbose=False,
                               _engine=eng)
            torch.cuda.synchronize()
            if i:
                walls.append(round(time.perf_counter() - t0, 4))
    finally:
        eng.close()
    return walls


def profile(B, n, reps):
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    X, Y = _data(B)
    eng = Engine(scratch_gb=48.0)
    kw = dict(n_components=K, n_perm=n, n_boot=0, vip_components=C, seed=1, verbose=False, _engine=eng)

    def call(flag):
        phases = {}
        torch.cuda.synchronize()
        eng.set_timing(True)
        t0 = time.perf_counter()
        pls.pls_regression(X, Y, vip_perm=flag, _phases=phases, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kt = eng.kernel_timing()
        eng.set_timing(False)
        free, total = torch.cuda.mem_get_info(eng.device)
        return dict(wall_s=wall, phases=phases, kt=kt, in_use_gb=(total - free) / 2 ** 30)

    def stack_pass(which, d_stack, d_obs):
        torch.cuda.synchronize()
        eng.set_timing(True)
        if which == 'perm':
            count = torch.zeros((B,), dtype=torch.int32, device=eng.device)
            eng.simpls_vip_perm_test(d_stack, d_obs, count, eng._zeros((n,)))
        else:
            eng.simpls_vip_ci(d_stack)
        eng.sync()
        ms = eng.kernel_timing().get('k_coef_prod', (0.0, 0))
        eng.set_timing(False)
        return ms

    try:
        call(False)
        mem_without = call(False)['in_use_gb']           # (before the first call with the keyword allocates anything)
        call(True)
        runs = {False: [], True: []}
        for _ in range(reps):
            for flag in (False, True):
                runs[flag].append(call(flag))
        # the yardstick: the data stay bound from the last call
        gen = torch.Generator(device=eng.device)
        gen.manual_seed(1)
        d_stack = torch.randn((n, C, S), dtype=torch.float64, device=eng.device, generator=gen)
        d_obs = eng._dev(np.full(B, np.sqrt(float(B) * C * S)), np.float64)
        yard = {'perm': [], 'prod': []}
        for which in ('perm', 'prod'):
            stack_pass(which, d_stack, d_obs)
        for _ in range(reps):
            for which in ('perm', 'prod'):
                yard[which].append(stack_pass(which, d_stack, d_obs))
        del d_stack
        peak = eng.mfma_f64_peak()
    finally:
        eng.close()

    def med(flag, fn):
        return float(np.median([fn(r) for r in runs[flag]]))

    def cls(name):
        return lambda r: r['kt'].get(name, (0.0, 0))[0]
    prod_ms = med(True, cls('k_coef_prod'))
    flop = 2.0 * B * S * C * n
    yp, yv = [r[0] for r in yard['perm']], [r[0] for r in yard['prod']]
    return dict(
        shape=dict(S=S, B=B, T=T, n_components=K, vip_components=C, n_perm=n, n_boot=0), reps=reps,
        wall_s_without=round(med(False, lambda r: r['wall_s']), 4), wall_s_with=round(med(True, lambda r: r['wall_s']), 4),
        wall_s_all_without=[round(r['wall_s'], 4) for r in runs[False]],
        wall_s_all_with=[round(r['wall_s'], 4) for r in runs[True]],
        permutations_phase_ms_without=round(med(False, lambda r: r['phases'].get('permutations', 0.0)), 2),
        permutations_phase_ms_with=round(med(True, lambda r: r['phases'].get('permutations', 0.0)), 2),
        vip_perm_setup_ms=round(med(True, lambda r: r['phases'].get('vip_perm', 0.0)), 2),
        host_finish_ms_without=round(med(False, lambda r: r['phases'].get('host_finish', 0.0)), 2),
        host_finish_ms_with=round(med(True, lambda r: r['phases'].get('host_finish', 0.0)), 2),
        feature_pass_ms=round(prod_ms, 2), feature_pass_ms_all=[round(cls('k_coef_prod')(r), 2) for r in runs[True]],
        feature_pass_brackets=runs[True][0]['kt'].get('k_coef_prod', (0.0, 0))[1],
        feature_pass_flop=flop, feature_pass_tflops=round(flop / (prod_ms * 1e9), 2) if prod_ms > 0 else None,
        k_sd_vip_ms=round(med(True, cls('k_sd_coef')), 2),
        k_simpls_dual_ms_without=round(med(False, cls('k_simpls_dual')), 2),
        k_simpls_dual_ms_with=round(med(True, cls('k_simpls_dual')), 2),
        yardstick=dict(
            stack='random (n_perm, c, S), same process, alternating',
            k_vip_perm_prod_ms_all=[round(v, 2) for v in yp], k_vip_prod_with_moments_ms_all=[round(v, 2) for v in yv],
            k_vip_perm_prod_ms=round(float(np.median(yp)), 2), k_vip_prod_with_moments_ms=round(float(np.median(yv)), 2),
            k_vip_perm_prod_tflops=round(flop / (float(np.median(yp)) * 1e9), 2),
            k_vip_prod_with_moments_tflops=round(flop / (float(np.median(yv)) * 1e9), 2),
            brackets=dict(perm=yard['perm'][0][1], prod=yard['prod'][0][1])),
        mfma_f64_peak_tflops=round(peak, 1),
        device_mem_in_use_gb_without=round(mem_without, 2),
        device_mem_in_use_gb_with=round(max(r['in_use_gb'] for r in runs[True]), 2),
        kernel_ms_with={key: round(v[0], 2) for key, v in runs[True][-1]['kt'].items()},
        kernel_ms_without={key: round(v[0], 2) for key, v in runs[False][-1]['kt'].items()})


def against_parent(parent_root, B, n, reps, rounds=2):
    """Fresh processes, alternating: this tree, the parent's, this tree, ...; each prints its wall times."""
    out = {'change': [], 'parent': []}
    for _ in range(rounds):
        for name, root in (('change', ROOT), ('parent', parent_root)):
            cmd = [sys.executable, os.path.abspath(__file__), '--without-only', '--root', root, '--reps', str(reps),
                   '--shape-b', str(B)] + (['--quick'] if n != 5000 else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300, check=True)
            out[name] += json.loads(r.stdout.strip().splitlines()[-1])
    return dict(wall_s_all_change=out['change'], wall_s_all_parent=out['parent'],
                wall_s_change=round(float(np.median(out['change'])), 4),
                wall_s_parent=round(float(np.median(out['parent'])), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vip_perm_c5.json'))
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--no-wide', action='store_true')
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--without-only', action='store_true')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--shape-b', type=int, default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    n = 600 if args.quick else 5000
    if args.without_only:
        print(json.dumps(without_only(args.shape_b or 600, n, args.reps)), flush=True)
        return
    shapes = (600,) if args.no_wide else (600, 100000)
    parent = {}
    if args.parent_root:                               # (child processes first: this one has not touched the GPU yet)
        for B in shapes:
            parent[B] = against_parent(args.parent_root, B, n, args.reps)
            print(json.dumps({'B': B, 'without_keyword_vs_parent': parent[B]}), flush=True)
    out = {}
    for B in shapes:
        got = profile(B, n, args.reps)
        if B in parent:
            got['without_keyword_vs_parent'] = parent[B]
        out['B{}'.format(B)] = got
        print(json.dumps({'B': B, **got}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
