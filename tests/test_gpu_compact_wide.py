"""Compact bootstrap blocks with four column tiles per wave (k_xprod_compact NC = 4: blocks of 256 feature columns,
lane c of a wave holds columns 4c .. 4c+3 of the wave's 64) against the oracle and against the two-tile blocks.

Every element of R receives the same products in the same k order at either width and 1 / std the same operations, so
the two widths must agree bit for bit -- in R and in everything downstream of it.  Each case

* runs eng.boot through the wide blocks and compares ``distrib`` (1e-9 per LV) and sum U / sum U^2 (1e-8 per live LV)
  with ref.single_boot, the tolerances of test_gpu_boot_followers;
* runs the same call with the option ``no_compact_wide`` and asserts numpy.array_equal on all three, and on R itself
  (Engine.crosscov with ``crosscov_sparse``).

The width that ran is asserted from Engine.last_timing()['compact_col_tiles'].  T' = 49 .. 52 (four tiles of rows with
the tail) takes the wide blocks by default; every other case forces them with the test-only option
``compact_wide_always``.  What the cases reach:

  T'  16 one tile (no tail form)    20 tail with 4 rows     33 tail with 1 live row      48 three full tiles
      50 four tiles, tail, moment rows (the headline)       52 full tail: no spare row, 1 / std from the table
  B   37 one partly live wave, the block's other waves beyond the last column       325 the last block's waves 2, 3
      beyond it        1037 five blocks, the last with one live wave
  S   12 a single stage       97 odd and even stage counts      174 the contraction length of the follower tests
  cells 1; 2 (one group, two conditions); 5 (more than the scale registers: the LDS scale table)
  bootstraps per call 1; 8 (one full sweep of 8 groups); 9 (and one more)

Data: replica_expect.synth.  Every case prints its figures before it asserts.  Per LV means per live LV of the original
(singular value above 1e-4 of the first, as in test_gpu_boot_followers): all of them except at S = 12, where R has rank
11 and the oracle's own ``distrib`` of a dead LV is 0 / 0.
"""
import json

import numpy as np
import pytest

from conftest import assert_close_per_lv
from oracle import cpu_ref as ref
from replica_expect import synth
import compact_expect as ce

gpu = pytest.mark.gpu

RTOL_DISTRIB, RTOL_SUMS = 1e-9, 1e-8

# (T', B, groups, n_cond, bootstraps)
CASES = [
    (50, 1037, [174], 1, 9),            # the headline variant: moment row of one cell, ragged last block, 8 + 1 groups
    (50, 325, [87], 2, 8),              # two cells, two moment rows: exactly the tail tile's spare rows
    (50, 1037, [20, 20, 19, 19, 19], 1, 9),   # five cells: the LDS scale table
    (52, 325, [97], 1, 8),              # full tail: no moment row, the scale from the table in registers
    (20, 1037, [20, 20, 19, 19, 19], 1, 9),   # two tiles with the tail, LDS scale table
    (20, 37, [87], 2, 1),
    (33, 325, [97], 1, 9),              # three tiles, one live row in the tail
    (48, 1037, [87], 2, 8),             # three full tiles, no spare row, two cells in registers
    (50, 37, [12], 1, 8),               # S = 12: blocks of one stage
    (16, 37, [12], 1, 1),               # one tile
]


def default_wide(Tp):
    """compact_boot_wide (plsx_xprod.hip): four tiles of rows with the tail."""
    return ce.m_tiles(Tp) == 4 and ce.has_tail(Tp)


def test_cases_cover_what_they_are_listed_for():
    assert {c[0] for c in CASES} == {16, 20, 33, 48, 50, 52}
    assert {c[1] for c in CASES} == {37, 325, 1037}
    assert {sum(c[2]) * c[3] for c in CASES} == {12, 97, 174}
    assert {len(c[2]) * c[3] for c in CASES} == {1, 2, 5}
    assert {c[4] for c in CASES} == {1, 8, 9}
    assert [ce.m_tiles(tp) for tp in (16, 20, 33, 48, 50, 52)] == [1, 2, 3, 3, 4, 4]
    assert [ce.has_tail(tp) for tp in (16, 20, 33, 48, 50, 52)] == [False, True, True, False, True, True]
    assert [default_wide(tp) for tp in (16, 20, 33, 48, 49, 52, 53)] == [False, False, False, False, True, True, False]


def _run(Tp, B, groups, n_cond, boots, wide):
    """-> (sum U, sum U^2, distrib (n, T', L), R (n, T', B)), last_timing() of the boot call, the original."""
    from pypyls_amd import hostmath, resampling as rsmp
    from pypyls_amd.engine import Engine
    S, J = sum(groups) * n_cond, len(groups) * n_cond
    X, Y = synth(S, B, Tp // J, seed=Tp)
    options = dict(compact_boot_always=1, crosscov_sparse=1)
    if not wide:
        options['no_compact_wide'] = 1
    elif not default_wide(Tp):
        options['compact_wide_always'] = 1
    eng = Engine(options=options)
    try:
        eng.set_data(X, Y, rsmp.cell_of_row(groups, n_cond), len(groups), n_cond, 0)
        assert eng.Tp == Tp
        xw, sv, yw = eng.decompose()
        xw, yw = hostmath.sign_convention(xw, yw)
        eng.set_original(xw, sv, yw)
        usum, usq, dist = eng.boot(boots)
        tm = eng.last_timing()
        R = eng.crosscov(xsrc=boots, ysrc=boots)
        tm_r = eng.last_timing()
    finally:
        eng.close()
    what = "T'={} width {}".format(Tp, 4 if wide else 2)
    for t in (tm, tm_r):
        ce.pin_compact(t, Tp, what)
        assert t.get('compact_col_tiles') == (4.0 if wide else 2.0), (
            '{}: the launch reports compact_col_tiles = {} (full report: {})'.format(what, t.get('compact_col_tiles'), t))
    return (usum.cpu().numpy(), usq.cpu().numpy(), np.moveaxis(dist, -1, 0), R), (X, Y, xw, sv)


def _worst_per_lv(a, b, keep):
    a, b = np.asarray(a)[..., keep], np.asarray(b)[..., keep]
    axes = tuple(range(a.ndim - 1))
    return float(np.max(np.max(np.abs(a - b), axis=axes) / np.max(np.abs(b), axis=axes)))


@gpu
@pytest.mark.parametrize('Tp,B,groups,n_cond,n', CASES)
def test_wide_blocks(Tp, B, groups, n_cond, n):
    from pypyls_amd import resampling as rsmp
    boots = np.asarray(rsmp.gen_bootsamp(groups, n_cond, n, seed=1000 + Tp + B, verbose=False))
    (usum, usq, dist, R), (X, Y, xw, sv) = _run(Tp, B, groups, n_cond, boots, True)
    (usum2, usq2, dist2, R2), _ = _run(Tp, B, groups, n_cond, boots, False)
    spec = ref.Spec('behavioral', groups, n_cond)
    live = sv > 1e-4 * sv[0]
    want_us, want_uq, want_d = np.zeros_like(usum), np.zeros_like(usq), []
    for i in range(n):
        wd, wu = ref.single_boot(spec, X, Y, boots[:, i], xw, np.diag(sv))
        want_d.append(wd)
        want_us += wu
        want_uq += wu ** 2
    want_d = np.stack(want_d)
    equal = dict(R=bool(np.array_equal(R, R2)), distrib=bool(np.array_equal(dist, dist2)),
                 usum=bool(np.array_equal(usum, usum2)), usq=bool(np.array_equal(usq, usq2)))
    print('compact_wide_parity ' + json.dumps(dict(
        case="T'={} B={} S={} cells={} n={}".format(Tp, B, sum(groups) * n_cond, len(groups) * n_cond, n),
        distrib=_worst_per_lv(dist, want_d, live), usum=_worst_per_lv(usum, want_us, live),
        usq=_worst_per_lv(usq, want_uq, live), live=int(live.sum()), equal_to_two_tiles=equal), sort_keys=True))
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(usum)) and np.all(np.isfinite(usq))
    for i in range(n):
        assert_close_per_lv(dist[i], want_d[i], 1, RTOL_DISTRIB, what='bootstrap {} distrib'.format(i), keep=live)
    assert_close_per_lv(usum, want_us, 1, RTOL_SUMS, what='sum U', keep=live)
    assert_close_per_lv(usq, want_uq, 1, RTOL_SUMS, what='sum U^2', keep=live)
    assert all(equal.values()), 'four column tiles per wave against two: array_equal {}'.format(equal)
