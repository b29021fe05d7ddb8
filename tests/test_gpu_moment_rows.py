"""First moments from the idle padding rows of the compact bootstrap blocks (k_xprod_compact, epilogue 3).

A compact block issues whole tiles: ceil(T'/16) tiles of 16 rows, or 16 (m - 1) + 4 rows when the last tile runs on
the 4x4x4 shape.  When the rows beyond T' are at least as many as the cells J (and J is at most the cells a lane keeps
in registers, compact_scale_regs(KT)), row T' + j of the block's A operand holds the multiplicities of cell j's drawn
rows: the block's own accumulators then deliver m1 = sum w x, the moment-only blocks contract X^2 only (k_xprod
epilogue 9: 16 or 24 tiles of 16 pairs each, raw m2 into the table that holds 1 / std on the other route), and the
compact epilogue forms 1 / std itself.  Engine.last_timing()['moment_rows'] says which route a launch took; the option
no_moment_rows forces the other one.

* 1: the padding-row geometry with one cell, both routes against the oracle, the route-to-route difference printed;
* 2: several cells, one shape whose moment rows sit in another tile than their cell's data rows, two fallbacks;
* 3: the three classes of the layout of the X^2-only blocks;
* 4: the Gram / solve / rotation chain behind the new route;
* 5: (CPU) the new summation order of m1 restated in float64 against a long-double evaluation.

Data and tolerances are those of test_gpu_compact_blocks: replica_expect.synth, B = 1037, S = 150, R against
ref.gen_covcorr at 1e-10, distrib 1e-9 and sum U / sum U^2 1e-8 per live LV.  Every case prints one JSON line of its
figures before it asserts.
"""
import json

import numpy as np
import pytest

from oracle import cpu_ref as ref
from replica_expect import synth
import compact_expect as ce

gpu = pytest.mark.gpu

B = 1037
S = 150
RTOL_R = 1e-10


def _report(case, **figs):
    print('moment_rows_parity ' + json.dumps(dict(case=case, **figs), sort_keys=True))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def spare_rows(Tp):
    """Rows a compact block of T' data rows issues beyond them (launch_cboot: the tail tile has 4 rows)."""
    mt = ce.m_tiles(Tp)
    return (16 * (mt - 1) + 4 if ce.has_tail(Tp) else 16 * mt) - Tp


def takes_moment_rows(Tp, J):
    """compact_moment_rows (plsx_xprod.hip): the cells fit the scale registers and the padding rows."""
    return J <= min(ce.stage_ksteps(ce.m_tiles(Tp)), 4) and spare_rows(Tp) >= J


def _crosscov(groups, n_cond, X, Y, inds, **options):
    """R of the resamples through the compact bootstrap route, last_timing()."""
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    eng = Engine(options=dict(compact_boot_always=1, crosscov_sparse=1, **options))
    try:
        eng.set_data(X, Y, rsmp.cell_of_row(groups, n_cond), len(groups), n_cond, 0)
        got = eng.crosscov(xsrc=inds, ysrc=inds)
        tm = eng.last_timing()
    finally:
        eng.close()
    return got, tm


def _oracle(groups, n_cond, X, Y, inds):
    spec = ref.Spec('behavioral', groups, n_cond)
    return [ref.gen_covcorr(spec, X[inds[:, i]], Y[inds[:, i]], spec.dummy) for i in range(inds.shape[1])]


def _gate(case, got, want):
    assert np.all(np.isfinite(got)), case
    errs = [_rel(got[i], want[i]) for i in range(len(want))]
    for i, e in enumerate(errs):
        assert e <= RTOL_R, '{}: R of resample {} vs oracle: rel err {:.3e} > {:g}'.format(case, i, e, RTOL_R)


def _pin_route(tm, Tp, expected, case):
    ce.pin_compact(tm, Tp, case)
    assert tm.get('moment_rows') == (1.0 if expected else 0.0), (
        'path moved: {} reports moment_rows = {} where the geometry says {} (full report: {})'.format(
            case, tm.get('moment_rows'), int(expected), tm))


# ----------------------------------------------------------------------------------------------------------------
# 1: padding-row geometry, one cell
# ----------------------------------------------------------------------------------------------------------------

GEOMETRY = [13, 49, 50, 51, 52, 48, 21, 53]


def test_geometry_cases_are_what_they_are_named_for():
    assert [spare_rows(tp) for tp in GEOMETRY] == [3, 3, 2, 1, 0, 0, 11, 11]
    assert [ce.has_tail(tp) for tp in GEOMETRY] == [False, True, True, True, True, False, False, False]
    assert [takes_moment_rows(tp, 1) for tp in GEOMETRY] == [True, True, True, True, False, False, True, True]
    assert ce.m_tiles(53) == 4 and ce.m_tiles(21) == 2


@gpu
@pytest.mark.parametrize('Tp', GEOMETRY)
def test_padding_row_geometry_one_cell(Tp):
    """13: one tile, 3 spare rows; 49, 50, 51: tail with 3, 2, 1 spare rows; 52: tail full, 48: full tile -- both fall
    back; 21: two tiles, no tail; 53: the first T' without the tail at four tiles.  edge_resamples at the variant's KT
    (3 distinct rows .. all S, one resample over the last five rows).  Each route is gated against the oracle; the
    largest relative difference between the routes is printed, not gated (measured on the MI355X: 0.0 in every case,
    profiles/moment_rows_compare.txt -- the fp64 MFMA adds a k-step's products one after the other and a zero weight
    adds an exact zero, so both routes run the same chain of additions)."""
    mt = ce.m_tiles(Tp)
    X, Y = synth(S, B, Tp, seed=Tp)
    inds, distinct = ce.edge_resamples(S, ce.stage_ksteps(mt), seed=Tp)
    want = _oracle([S], 1, X, Y, inds)
    case = "geometry T'={} ({} tiles{}, {} spare)".format(Tp, mt, ', tail' if ce.has_tail(Tp) else '', spare_rows(Tp))
    got, tm = _crosscov([S], 1, X, Y, inds)
    old, tm_old = _crosscov([S], 1, X, Y, inds, no_moment_rows=1)
    routes = max(_rel(got[i], old[i]) for i in range(len(want)))
    _report(case, moment_rows=tm.get('moment_rows'), R=max(_rel(got[i], want[i]) for i in range(len(want))),
            R_no_moment_rows=max(_rel(old[i], want[i]) for i in range(len(want))), route_to_route=routes)
    _pin_route(tm, Tp, takes_moment_rows(Tp, 1), case)
    _pin_route(tm_old, Tp, False, case + ', no_moment_rows')
    _gate(case, got, want)
    _gate(case + ', no_moment_rows', old, want)
    assert abs(tm['compact_row_fraction'] - ce.row_fraction(distinct, S)) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------
# 2: cells
# ----------------------------------------------------------------------------------------------------------------

# (groups, n_cond, T, route): T' = 50, J = 2 has exactly two spare rows, both in the tail tile while cell 0's data rows
# are tiles 0 and 1; T' = 21, J = 3; T' = 48 has no spare row; T' = 56, J = 4 has eight but J > compact_scale_regs(3)
CELLS = [([75, 75], 1, 25, True), ([50] * 3, 1, 7, True), ([50] * 3, 1, 16, False), ([38] * 4, 1, 14, False)]


@gpu
@pytest.mark.parametrize('groups,n_cond,T,route', CELLS)
def test_cells(groups, n_cond, T, route):
    from pypyls_amd import resampling as rsmp
    J = len(groups) * n_cond
    Tp, rows = J * T, sum(groups) * n_cond
    assert takes_moment_rows(Tp, J) == route
    if Tp == 50:
        assert spare_rows(Tp) == J and ce.m_tiles(Tp) - 1 > (T - 1) // 16     # (moment row of cell 0: another tile)
    if Tp == 56:
        assert spare_rows(Tp) >= J and ce.m_tiles(Tp) == 4 and J > min(ce.stage_ksteps(4), 4)
    X, Y = synth(rows, B, T, seed=Tp)
    inds = np.asarray(rsmp.gen_bootsamp(groups, n_cond, 11, seed=J * T, verbose=False))
    want = _oracle(groups, n_cond, X, Y, inds)
    case = "cells T'={} J={}".format(Tp, J)
    got, tm = _crosscov(groups, n_cond, X, Y, inds)
    _report(case, moment_rows=tm.get('moment_rows'), R=max(_rel(got[i], want[i]) for i in range(len(want))))
    _pin_route(tm, Tp, route, case)
    _gate(case, got, want)


# ----------------------------------------------------------------------------------------------------------------
# 3: layouts of the X^2-only blocks
# ----------------------------------------------------------------------------------------------------------------

# moment2_layout (plsx_xprod.hip): blocks of 256 pairs (16 tiles) when they issue fewer tiles than blocks of 384 pairs
# (24 tiles) by a sixth or more, as moment_layout chooses between 128 and 192: <= 256 pairs one 16-tile block,
# 257 .. 384 one 24-tile block, 385 .. 512 two 16-tile blocks of which the second is partly empty
MOMENT2_CLASSES = ((1, 256), (257, 384), (385, 512))


def moment2_layout(npairs):
    """-> (pairs per block, blocks), the rule of moment2_layout restated."""
    t384, t256 = -(-npairs // 384) * 24, -(-npairs // 256) * 16
    pairs = 256 if t256 * 6 < t384 * 5 else 384
    return pairs, -(-npairs // pairs)


def test_moment2_classes():
    want = ((256, 1), (384, 1), (256, 2))
    for (lo, hi), w in zip(MOMENT2_CLASSES, want):
        assert moment2_layout(lo) == w and moment2_layout(hi) == w, (lo, hi)
    assert moment2_layout(504) == (256, 2)                  # (the headline launch: 32 tile passes)


@gpu
@pytest.mark.parametrize('cls,n', list(enumerate((11, 300, 400))))
def test_layouts_of_the_x2_only_blocks(cls, n):
    from pypyls_amd import resampling as rsmp
    Tp = 50
    assert MOMENT2_CLASSES[cls][0] <= n <= MOMENT2_CLASSES[cls][1]
    X, Y = synth(S, B, Tp, seed=Tp)
    inds = np.asarray(rsmp.gen_bootsamp([S], 1, n, seed=n, verbose=False))
    want = _oracle([S], 1, X, Y, inds)
    case = "layout T'=50 n={} ({} pairs per block x {})".format(n, *moment2_layout(n))
    got, tm = _crosscov([S], 1, X, Y, inds)
    _report(case, moment_rows=tm.get('moment_rows'), R=max(_rel(got[i], want[i]) for i in range(len(want))))
    _pin_route(tm, Tp, True, case)
    _gate(case, got, want)


# ----------------------------------------------------------------------------------------------------------------
# 4: the chain behind it
# ----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('Tp', [50, 21])
def test_chain_behind_the_moment_rows(Tp):
    """eng.boot with the compact blocks forced and the new route pinned, 11 ordinary bootstraps: distrib at 1e-9 per
    LV, sum U and sum U^2 at 1e-8 per live LV against ref.single_boot (the checks of test_gpu_boot_followers)."""
    from test_gpu_boot_followers import _Shape, _check_boot, B_SMALL
    assert B_SMALL == B
    case = "chain T'={}".format(Tp)
    sh = _Shape(Tp, B)
    figs = {}
    try:
        sh.eng.set_option('compact_boot_always', 1)
        boots = sh.samples('boot', 11, 7000 + Tp)
        usum, usq, dist, tm = sh.boot(boots)
        _pin_route(tm, Tp, True, case)
        failures = _check_boot(sh, (usum, usq, dist), boots, 7000 + Tp, np.arange(11), figs)
    finally:
        sh.close()
        _report(case, **figs.get('boot', {}))
    assert not failures, '{}:\n  '.format(case) + '\n  '.join(failures)


# ----------------------------------------------------------------------------------------------------------------
# 5: the new summation order of m1, on the CPU
# ----------------------------------------------------------------------------------------------------------------

def moment_rows_model_R(X, Y, inds):
    """compact_expect.kernel_model_R with m1 the way the padding row forms it: over the drawn rows only, in rank
    (= row) order, one k-step of four rows at a time -- the four products of a k-step are summed, then added to the
    accumulator.  m2 stays the sum of the moment-only blocks, the variance formula is the same."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n = np.float64(len(inds))
    Xc = X - X.sum(axis=0) / np.float64(len(X))
    rows, w = np.unique(inds, return_counts=True)
    w = w.astype(np.float64)
    Yr = Y[inds]
    mean = Yr.sum(axis=0) / n
    rstd = 1 / np.sqrt(((Yr - mean) ** 2).sum(axis=0) / (n - 1))
    A = (w[:, None] * (Y[rows] - mean) * rstd / (n - 1)).T
    xs = Xc[rows]
    C = A @ xs
    m1 = np.zeros(xs.shape[1])
    for k in range(0, len(rows), 4):
        m1 = m1 + (w[k:k + 4, None] * xs[k:k + 4]).sum(axis=0)
    m2 = (w[:, None] * xs * xs).sum(axis=0)
    var = (m2 - m1 * m1 / n) / (n - 1)
    return C / np.sqrt(var)


@pytest.mark.parametrize('Tp', GEOMETRY)
def test_moment_row_margin(Tp):
    """The restatement above against compact_expect.exact_R (long double, no raw moments) on the data and resamples of
    case 1: within a tenth of 1e-10, the margin test_raw_moment_margin establishes for the arithmetic of the other
    route."""
    X, Y = synth(S, B, Tp, seed=Tp)
    inds, _ = ce.edge_resamples(S, ce.stage_ksteps(ce.m_tiles(Tp)), seed=Tp)
    worst = max(_rel(moment_rows_model_R(X, Y, inds[:, i]), ce.exact_R(X, Y, inds[:, i])) for i in range(inds.shape[1]))
    _report("margin T'={}".format(Tp), moment_row_arithmetic=worst)
    assert worst <= 0.1 * RTOL_R, worst
