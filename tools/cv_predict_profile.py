"""Time what the out-of-fold predictions (cv_predict=) add to a cross-validated call, and check that the call WITHOUT the
keyword costs what it cost at the parent commit; write profiles/cv_predict_c5.json (pls_regression) or
profiles/cv_predict_c4.json (behavioral_pls).

    python tools/cv_predict_profile.py [--behavioral] [--reps 5] [--out FILE] [--quick]
                                       [--without-only] [--root DIR] [--compare-parent DIR [--rounds 3]]
                                       [--kernel-run] [--kernel-stats FILE [--merge-only]]

pls_regression: BASELINE config 5's solver shape, S = 1000, B = 100 000, T = 20, k = 15, 100 splits, no permutations and
no bootstraps (the cross-validation is the leg the keyword touches).  ``--behavioral``: the headline shape, S = 500,
B = 200 000, T = 50, 100 splits.  One GPU, a fixed-budget engine.

1. The public call with ``cv_predict=True`` and the same call without it, ALTERNATED in one process after one warm-up of
   each (``--reps`` pairs, every call bracketed by device synchronisation; medians, every repeat kept), with the wall
   time of the ``crossval`` phase.
2. ``--without-only`` runs the call without the keyword alone and prints its record; ``--root DIR`` imports the package
   from another checkout (the parent commit's, with its own library).  ``--compare-parent DIR`` is the driver of the one
   condition this feature has to meet: it starts ``--without-only`` alternately on DIR and on this checkout, ``--rounds``
   times each, a fresh process every time, and writes both sets of times and the parent's run-to-run spread into the
   output.  Met when this checkout's median is not above the parent's slowest repeat.
3. ``--kernel-run`` makes one call with the keyword and writes nothing: the program to put behind
   ``rocprofv3 --kernel-trace --stats --`` in a run of its own.  ``--kernel-stats FILE`` copies the rows of that run's
   kernel_stats.csv (or of its ``*_results.db``) for the new kernels and the kernels they stand behind into the output (``--merge-only``: into an
   output that exists, without timing anything).

``--quick``: B = 2000, 10 splits (a rehearsal)."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

KERNELS = ('k_sd_cv_pred', 'k_sd_cv_score', 'k_cv_pred_export', 'k_cv_final', 'k_sd_step', 'k_sd_init', 'k_sd_final',
           'k_nt_', 'k_gram', 'k_xprod')


def kernel_rows(path):
    """The rows of the kernels of interest from rocprofv3's kernel statistics: a kernel_stats.csv, or the rocpd
    database (``*_results.db``, view ``top_kernels``, durations in microseconds) newer versions write by default."""
    rows = {}
    if path.endswith('.db'):
        import sqlite3
        with sqlite3.connect(path) as db:
            for name, calls, total, avg in db.execute('select name, total_calls, total_duration, average from top_kernels'):
                name = name.split('(')[0].replace('void ', '').strip()
                if any(key in name for key in KERNELS):
                    rows[name[:60]] = dict(calls=int(calls), total_ms=round(float(total) / 1e3, 3),
                                           avg_ms=round(float(avg) / 1e3, 4))
        return rows
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r['Name'].split('(')[0].replace('void ', '').strip()
            if any(key in name for key in KERNELS):
                rows[name[:60]] = dict(calls=int(r['Calls']), total_ms=round(float(r['TotalDurationNs']) / 1e6, 3),
                                       avg_ms=round(float(r['AverageNs']) / 1e6, 4))
    return rows


def leg(ts, phases):
    return dict(wall_s=round(float(np.median(ts)), 4), wall_s_all=[round(t, 4) for t in ts],
                crossval_ms=round(phases.get('crossval', 0.0) / max(len(ts), 1), 2))


def compare_parent(args, here, out_path):
    """Alternate the call without the keyword between the parent's checkout and this one, a fresh process each."""
    base = [sys.executable, os.path.abspath(__file__), '--without-only', '--reps', str(args.reps)] + \
        (['--behavioral'] if args.behavioral else []) + (['--quick'] if args.quick else [])
    runs = dict(parent=[], this=[])
    for _ in range(args.rounds):
        for side, root in (('parent', os.path.abspath(args.compare_parent)), ('this', here)):
            r = subprocess.run(base + ['--root', root], stdout=subprocess.PIPE, text=True, check=True, timeout=900)
            runs[side].append(json.loads(r.stdout.strip().splitlines()[-1])['call_without_keyword'])
    out = {}
    if os.path.exists(out_path):
        with open(out_path) as fh:
            out = json.load(fh)
    med = {side: [r['wall_s'] for r in rs] for side, rs in runs.items()}
    every = {side: [t for r in rs for t in r['wall_s_all']] for side, rs in runs.items()}
    cv = {side: [r['crossval_ms'] for r in rs] for side, rs in runs.items()}
    out['without_keyword_parent_vs_this'] = dict(
        how='--without-only alternated between the parent commit\'s checkout and this one, a fresh process each, '
            '{} rounds of {} timed calls after a warm-up'.format(args.rounds, args.reps),
        parent_wall_s_medians=med['parent'], this_wall_s_medians=med['this'],
        parent_wall_s_range=[min(every['parent']), max(every['parent'])],
        this_wall_s_range=[min(every['this']), max(every['this'])],
        parent_wall_s_median=round(float(np.median(every['parent'])), 4),
        this_wall_s_median=round(float(np.median(every['this'])), 4),
        parent_crossval_ms=cv['parent'], this_crossval_ms=cv['this'],
        parent_crossval_ms_range=[min(cv['parent']), max(cv['parent'])],
        this_median_not_above_the_parents_slowest_repeat=bool(float(np.median(every['this'])) <= max(every['parent'])))
    print(json.dumps(out['without_keyword_parent_vs_this']), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--behavioral', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--without-only', action='store_true')
    ap.add_argument('--compare-parent', default=None)
    ap.add_argument('--kernel-run', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--merge-only', action='store_true')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = os.path.abspath(args.root)
    out_path = args.out or os.path.join(here, 'profiles', 'cv_predict_c4.json' if args.behavioral else 'cv_predict_c5.json')
    if args.compare_parent:
        compare_parent(args, here, out_path)
        return
    if args.merge_only:                                    # --kernel-stats FILE into an existing output, nothing timed
        with open(out_path) as fh:
            out = json.load(fh)
        out['kernel_stats'] = dict(source='rocprofv3 --kernel-trace --stats of --kernel-run, a run of its own',
                                   kernels=kernel_rows(args.kernel_stats))
        with open(out_path, 'w') as fh:
            json.dump(out, fh, indent=1)
            fh.write('\n')
        print(json.dumps(out['kernel_stats']), flush=True)
        return
    sys.path.insert(0, root)
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    rs = np.random.RandomState(0)
    if args.behavioral:
        S, B, T, n = (500, 2000, 50, 10) if args.quick else (500, 200000, 50, 100)
        X = rs.randn(S, B)
        Y = rs.randn(S, T) + 0.5 * X[:, :T]
        shape = dict(S=S, B=B, T=T, test_split=n)
    else:
        S, B, T, k, n = (1000, 2000, 20, 15, 10) if args.quick else (1000, 100000, 20, 15, 100)
        X = rs.randn(S, B)
        Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
        shape = dict(S=S, B=B, T=T, n_components=k, test_split=n)
    eng = Engine(scratch_gb=48.0)

    def call(keyword, phases=None):
        extra = dict(cv_predict=True) if keyword else {}
        t0 = time.perf_counter()
        if args.behavioral:
            res = pls.behavioral_pls(X, Y, n_perm=0, n_boot=0, n_split=0, test_split=n, test_size=0.25, seed=1,
                                     verbose=False, _engine=eng, _phases=phases, **extra)
        else:
            res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, test_split=n, seed=1, verbose=False,
                                     _engine=eng, _phases=phases, **extra)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    if args.kernel_run:
        call(True)
        eng.close()
        return
    out = dict(shape=shape, reps=args.reps, stack_bytes=8 * S * T * n)
    call(False)                                            # warm-up at full size (allocations)
    if not args.without_only:
        call(True)
    t_with, t_without, ph_with, ph_without = [], [], {}, {}
    for _ in range(args.reps):
        t_without.append(call(False, ph_without)[0])
        if not args.without_only:
            t_with.append(call(True, ph_with)[0])
    eng.close()
    out['call_without_keyword'] = leg(t_without, ph_without)
    if args.without_only:
        print(json.dumps(dict(call_without_keyword=out['call_without_keyword'])), flush=True)
        return
    out['call_with_keyword'] = leg(t_with, ph_with)
    out['added_wall_s'] = round(out['call_with_keyword']['wall_s'] - out['call_without_keyword']['wall_s'], 4)
    out['added_crossval_ms'] = round(out['call_with_keyword']['crossval_ms'] - out['call_without_keyword']['crossval_ms'], 2)
    if os.path.exists(out_path):                           # (a record of --compare-parent written before stays)
        with open(out_path) as fh:
            old = json.load(fh)
        for key in ('without_keyword_parent_vs_this', 'kernel_stats'):
            if key in old:
                out[key] = old[key]
    if args.kernel_stats:
        out['kernel_stats'] = dict(source='rocprofv3 --kernel-trace --stats of --kernel-run, a run of its own',
                                   kernels=kernel_rows(args.kernel_stats))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
