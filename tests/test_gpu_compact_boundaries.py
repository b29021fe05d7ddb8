"""The block boundaries of the compact cross-product blocks (k_xprod_compact): what its prologue and its last pass do
that the sweeps of test_gpu_compact_blocks.py do not pin.

A block stages everything besides its A stages and X rows behind ONE barrier: every lane fetches the row-table entries
of stage 0 for itself, the live entries of the table (whole stages) go to LDS as byte offsets four per thread and trip,
and the row maps get an LDS area of their own.  The last pass of the loop fetches the 1 / std of the block's cells for
the epilogue, per lane into registers up to compact_scale_regs(KT) = min(KT, 4) cells and by LDS-DMA into the wave's
own LDS area beyond; the epilogue is stores only.

* table copy: S = 61 and 150 (fewer table entries than the block has threads), 530 (three strides of 256 threads) and
  1100 (a second trip of the four-entries-per-thread copy), resamples of compact_expect.edge_resamples -- the first has
  3 distinct rows, fewer than one stage: the stage that lanes fetch for themselves is the partial last one and reads
  padding;
* scale path: J = 1, J at the register / LDS threshold and one past it, at one tile and at four tiles with and without
  the 4x4x4 tail;
* dead waves and dead blocks: B = 1037 and 1101 (the upper half of the last 128-column block beyond ldr in one, not in
  the other), 11 bootstraps (the last sweep of eight groups is partial: blocks that leave before the barrier), R and
  the chain behind it.  One resample is one group here, so a group of a launch never has fewer rows than its block has
  room for (rows_valid == rows_per_group): that guard of the prologue is reached by no compact launch;
* split halves at T' = 50, S = 150: epilogue 5 and epilogue 8 + reader on the row-count edges.

Data: replica_expect.synth, routes pinned from Engine.last_timing (compact_expect.pin_compact), R against
oracle.cpu_ref.gen_covcorr.  Tolerances are the project's: R 1e-10, distrib 1e-9, sum U / sum U^2 1e-8 per LV,
split-half correlations 1e-7 against the oracle and 1e-9 between routes.  Every case prints one JSON line of its worst
errors before it asserts.
"""
import json

import numpy as np
import pytest

from oracle import cpu_ref as ref
from replica_expect import synth
import compact_expect as ce

gpu = pytest.mark.gpu

RTOL_R, RTOL_SPLIT_ORACLE, RTOL_SPLIT_ROUTES = 1e-10, 1e-7, 1e-9


def _report(case, **figs):
    print('compact_boundaries_parity ' + json.dumps(dict(case=case, **figs), sort_keys=True))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def scale_regs(mt):
    """compact_scale_regs(KT) of plsx_k_xprod.h: cells whose 1 / std a lane of epilogue 3 keeps in registers."""
    return min(ce.stage_ksteps(mt), 4)


def _crosscov_vs_oracle(case, groups, n_cond, T, B, inds, seed, fraction=None):
    """R of the resamples `inds` (S, n) through plsx_crosscov_batch with the compact bootstrap route forced, every
    resample against gen_covcorr of the resampled data."""
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    J = len(groups) * n_cond
    S, Tp = sum(groups) * n_cond, J * T
    X, Y = synth(S, B, T, seed=seed)
    spec = ref.Spec('behavioral', groups, n_cond)
    eng = Engine(options=dict(compact_boot_always=1, crosscov_sparse=1))
    eng.set_data(X, Y, rsmp.cell_of_row(groups, n_cond), len(groups), n_cond, 0)
    try:
        assert eng.Tp == Tp
        got = eng.crosscov(xsrc=inds, ysrc=inds)
        tm = eng.last_timing()
    finally:
        eng.close()
    ce.pin_compact(tm, Tp, case)
    errs = [_rel(got[i], ref.gen_covcorr(spec, X[inds[:, i]], Y[inds[:, i]], spec.dummy)) for i in range(inds.shape[1])]
    figs = dict(R=max(errs), worst_resample=int(np.argmax(errs)), n=int(inds.shape[1]),
                row_fraction=tm['compact_row_fraction'])
    _report(case, **figs)
    assert np.all(np.isfinite(got)), case
    for i, e in enumerate(errs):
        assert e <= RTOL_R, '{}: R of resample {} vs oracle: rel err {:.3e} > {:g}'.format(case, i, e, RTOL_R)
    if fraction is not None:
        assert abs(tm['compact_row_fraction'] - fraction) <= 1e-12, \
            '{}: compact_row_fraction {!r} where the distinct rows of the resamples give {!r}'.format(
                case, tm['compact_row_fraction'], fraction)


# ----------------------------------------------------------------------------------------------------------------
# the copy of the row table
# ----------------------------------------------------------------------------------------------------------------

# (S, T'): 61 rows at 8 tiles (KT = 1: 16 k-steps, 64 entries), 150 at the headline's four tiles with the tail (KT = 3:
# 38 k-steps -> 13 stages, 156 entries), 530 (133 k-steps -> 45 stages, 540 entries: threads 0..27 copy a third one)
# and 1100 (275 k-steps -> 92 stages, 1104 entries: the copy's second trip, 80 threads)
TABLE_COPY = [(61, 116), (150, 50), (530, 50), (1100, 50)]


def test_table_copy_cases_sit_where_they_should():
    for S, Tp in TABLE_COPY:
        KT = ce.stage_ksteps(ce.m_tiles(Tp))
        entries = -(-(-(-S // 4)) // KT) * KT * 4
        assert (entries < 256) == (S in (61, 150)) and (entries > 512) == (S >= 530) and (entries > 1024) == (S == 1100)


@gpu
@pytest.mark.parametrize('S,Tp', TABLE_COPY)
def test_table_copy(S, Tp):
    """compact_expect.edge_resamples: exactly d distinct rows, d over the stage edges from 3 (one partial stage: the
    entries every lane fetches for itself are the block's only ones, padded with row 0, which those resamples never
    draw) to all S (every entry of the table live), plus ordinary draws."""
    KT = ce.stage_ksteps(ce.m_tiles(Tp))
    inds, distinct = ce.edge_resamples(S, KT, seed=S + Tp)
    assert distinct[0] == 3
    assert inds.shape[1] % 8 != 0
    _crosscov_vs_oracle("table copy S={} T'={}".format(S, Tp), [S], 1, Tp, 1037, inds, seed=S + Tp,
                        fraction=ce.row_fraction(distinct, S))


# ----------------------------------------------------------------------------------------------------------------
# the scales of the epilogue: registers or LDS
# ----------------------------------------------------------------------------------------------------------------

# (cells J, behaviours per cell T): one tile (threshold 4), four tiles with the tail (T' = 49..52, threshold 3) and
# without it (53..64, threshold 3)
SCALE_PATH = [(1, 13), (4, 3), (5, 3), (1, 50), (3, 17), (4, 13), (1, 53), (3, 18), (4, 16)]


def test_scale_path_cases_straddle_the_threshold():
    seen = set()
    for J, T in SCALE_PATH:
        mt = ce.m_tiles(J * T)
        assert mt in (1, 4)
        where = 'one' if J == 1 else 'registers' if J <= scale_regs(mt) else 'lds'
        assert J in (1, scale_regs(mt), scale_regs(mt) + 1)
        seen.add((mt, ce.has_tail(J * T), where))
    assert seen == {(1, False, w) for w in ('one', 'registers', 'lds')} | \
        {(4, t, w) for t in (False, True) for w in ('one', 'registers', 'lds')}


@gpu
@pytest.mark.parametrize('J,T', SCALE_PATH)
def test_scale_path(J, T):
    """J groups of 40 subjects, one condition: J cells with a 1 / std row each per resample, 11 ordinary bootstraps
    (gen_bootsamp draws inside the groups)."""
    from pypyls_amd import resampling as rsmp
    groups = [40] * J
    inds = np.asarray(rsmp.gen_bootsamp(groups, 1, 11, seed=100 * J + T, verbose=False))
    mt = ce.m_tiles(J * T)
    _crosscov_vs_oracle("scale path T'={} J={} ({} tile{}{}, {})".format(
        J * T, J, mt, 's' if mt > 1 else '', ', tail' if ce.has_tail(J * T) else '',
        'registers' if J <= scale_regs(mt) else 'LDS'), groups, 1, T, 1037, inds, seed=100 * J + T)


# ----------------------------------------------------------------------------------------------------------------
# dead waves and dead blocks
# ----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('B', [1037, 1101])
def test_dead_waves_and_dead_blocks(B):
    """T' = 50: with the L = 50 columns of the distrib operand the rows of R are 1087 -> 1088 (8.5 blocks of 128: the
    last block's upper two waves lie beyond ldr and leave after the loop, having met every barrier) or 1151 -> 1152
    (9 whole blocks).  11 bootstraps: groups 11..15 of the second sweep and the column blocks that pad the grid to a
    multiple of eight leave before the barrier as whole blocks.  R of the edge resamples, then the chain (distrib from
    the last column blocks, sum U, sum U^2) as test_chain_behind_the_compact_blocks checks it."""
    from test_gpu_boot_followers import _Shape, _check_boot
    Tp = 50
    inds, distinct = ce.edge_resamples(150, 3, seed=B)
    assert inds.shape[1] % 8 != 0
    _crosscov_vs_oracle("dead waves B={} R".format(B), [150], 1, Tp, B, inds, seed=B,
                        fraction=ce.row_fraction(distinct, 150))
    case = "dead waves B={} chain".format(B)
    sh = _Shape(Tp, B)
    figs = {}
    try:
        sh.eng.set_option('compact_boot_always', 1)
        boots = sh.samples('boot', 11, 7000 + B)
        usum, usq, dist, tm = sh.boot(boots)
        ce.pin_compact(tm, Tp, case)
        assert tm['xprod_launches'] == 1 and tm['xprod_resamples'] == 11, tm
        failures = _check_boot(sh, (usum, usq, dist), boots, 7000 + B, np.arange(11), figs)
    finally:
        sh.close()
        _report(case, **figs.get('boot', {}))
    assert not failures, '{}:\n  '.format(case) + '\n  '.join(failures)


# ----------------------------------------------------------------------------------------------------------------
# split halves at the headline's T'
# ----------------------------------------------------------------------------------------------------------------

@gpu
def test_split_halves_at_the_headline_shape():
    """T' = 50, S = 150: first halves of exactly n1 rows over the stage edges (compact_expect.first_half_masks),
    original arrangement and one permutation.  The default route is epilogue 8 + the one-pass reader, split_two_readers
    gives epilogue 5; both against ref.split_half at 1e-7 and against the dense fused blocks at 1e-9, as
    test_split_blocks_at_every_stage_edge holds its cases."""
    from test_gpu_compact_blocks import _SplitData, _pin_split, _worst_split
    Tp = 50
    masks, counts = ce.first_half_masks(150, ce.stage_ksteps(ce.m_tiles(Tp)), seed=Tp)
    data = _SplitData(Tp, masks, seed=Tp)
    case = "split halves T'=50"
    runs = {'default': data.run(), 'split_two_readers': data.run(split_two_readers=1)}
    _pin_split(runs['default'][2], case, split_route=1, split_blocks=8, split_reader=12)
    _pin_split(runs['split_two_readers'][2], case + ', split_two_readers', split_route=0, split_blocks=5,
               split_reader=0)
    dense = data.run(split_inblock=1)
    _pin_split(dense[2], case + ', split_inblock', split_route=0, split_blocks=1, split_reader=0)
    want = data.oracle()
    figs, failures = {}, []
    for name, (uc, vc, _) in runs.items():
        figs[name] = dict(ucorr_oracle=_worst_split(uc, want[0]), vcorr_oracle=_worst_split(vc, want[1]),
                          ucorr_dense=_worst_split(uc, dense[0]), vcorr_dense=_worst_split(vc, dense[1]))
        for key, val in figs[name].items():
            tol = RTOL_SPLIT_ORACLE if key.endswith('oracle') else RTOL_SPLIT_ROUTES
            if not val <= tol:
                failures.append('{} route, {}: {:.3e} > {:g}'.format(name, key, val, tol))
    _report(case, first_half_rows=counts, **figs)
    assert not failures, '{}:\n  '.format(case) + '\n  '.join(failures)
