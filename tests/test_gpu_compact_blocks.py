"""Every compiled variant of the compact cross-product blocks (k_xprod_compact: one bootstrap / one split per block,
contracting over the rows IT uses) at every edge of their stage loop, against the oracle.

The kernel is compiled once per tile count ceil(T'/16) = 1..13, with a second form at 2..13 tiles whose last tile
holds <= 4 live rows and runs on the 4x4x4 shape (25 bootstrap variants, epilogue 3), and for split halves at 1..4
tiles with epilogue 5 (both z-scored halves) or 8 (raw first-half sums for the one-pass reader): 12 reachable split
variants.  A block contracts over ksteps = ceil(rows / 4) k-steps in nkt = ceil(ksteps / KT) LDS stages, full stages
first, then one partial stage, prefetching stage min(kt + 1, nkt - 1): five sweeps put the row count on every edge.

* A: R itself (option crosscov_sparse) of every bootstrap variant, resamples with exactly d distinct rows;
* B: several cells, and the three layouts of the moment-only blocks that write the 1 / std table;
* C: the Gram / solve / rotation chain behind the variants test_compact_blocks_equal_dense_blocks does not reach;
* D: split-half blocks, first halves of exactly n1 rows, epilogue 5 and epilogue 8 + reader;
* E: the option split_reader8 (the other compiled forms of the one-pass reader) bit for bit.

Data: replica_expect.synth (bench.py's), correlation mode, B = 1037 (no multiple of 128; with the L columns of the
distrib operand 9 or 10 column blocks of 128: more than one row of eight in the block-id map).  Every case pins its
route from Engine.last_timing (the split-half cases from its keys split_blocks / split_reader and from
Engine.split_route) and prints one JSON line of its worst errors before it asserts.  Tolerances are the project's own:
R against the oracle 1e-10 (test_separate_moments_layout_equals_in_block), distrib 1e-9 and sum U / sum U^2 1e-8 per
LV (test_gpu_boot_followers), split-half correlations 1e-7 against the oracle and 1e-9 between routes
(test_split_half_one_pass_reader).  test_raw_moment_margin re-derives on the CPU that 1e-10 is far outside what the
kernel's raw-moment arithmetic and the oracle lose on this data.  profiles/compact_blocks_parity.txt has the figures.
"""
import json

import numpy as np
import pytest

from oracle import cpu_ref as ref
from replica_expect import synth
import compact_expect as ce

gpu = pytest.mark.gpu

B = 1037
RTOL_R, RTOL_SPLIT_ORACLE, RTOL_SPLIT_ROUTES = 1e-10, 1e-7, 1e-9
# sweep A: three stages of 12 k-steps fit into 150 rows at KT = 12, 6, 4, 3; KT = 2, 1 need fewer rows
S_SMALL_MT, S_LARGE_MT = 150, 61


def _report(case, **figs):
    print('compact_blocks_parity ' + json.dumps(dict(case=case, **figs), sort_keys=True))


def _engine(groups, n_cond, X, Y, **options):
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    eng = Engine(options=options)
    eng.set_data(X, Y, rsmp.cell_of_row(groups, n_cond), len(groups), n_cond, 0)
    return eng


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _crosscov_vs_oracle(case, groups, n_cond, T, inds, seed, compact=True, fraction=None):
    """R of the resamples `inds` (S, n) through plsx_crosscov_batch with the bootstrap route forced, every resample
    against gen_covcorr of the resampled data."""
    J = len(groups) * n_cond
    S, Tp = sum(groups) * n_cond, J * T
    X, Y = synth(S, B, T, seed=seed)
    spec = ref.Spec('behavioral', groups, n_cond)
    eng = _engine(groups, n_cond, X, Y, compact_boot_always=1, crosscov_sparse=1)
    try:
        assert eng.Tp == Tp
        got = eng.crosscov(xsrc=inds, ysrc=inds)
        tm = eng.last_timing()
    finally:
        eng.close()
    if compact:
        ce.pin_compact(tm, Tp, case)
    else:
        ce.pin_dense(tm, case)
    errs = [_rel(got[i], ref.gen_covcorr(spec, X[inds[:, i]], Y[inds[:, i]], spec.dummy)) for i in range(inds.shape[1])]
    figs = dict(R=max(errs), worst_resample=int(np.argmax(errs)), n=int(inds.shape[1]),
                row_fraction=tm['compact_row_fraction'])
    if fraction is not None:
        figs['row_fraction_expected'] = fraction
    _report(case, **figs)
    assert np.all(np.isfinite(got)), case
    for i, e in enumerate(errs):
        assert e <= RTOL_R, '{}: R of resample {} vs oracle: rel err {:.3e} > {:g}'.format(case, i, e, RTOL_R)
    if fraction is not None:
        assert abs(tm['compact_row_fraction'] - fraction) <= 1e-12, \
            '{}: compact_row_fraction {!r} where the distinct rows of the resamples give {!r}'.format(
                case, tm['compact_row_fraction'], fraction)
    return tm


# ----------------------------------------------------------------------------------------------------------------
# the margin of 1e-10, on the CPU
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('Tp', [8, 50, 208])
def test_raw_moment_margin(Tp):
    """The compact route takes 1 / std of a resampled feature from its raw moments, var = (m2 - m1^2 / n) / (n - 1),
    which cancels when few distinct rows are drawn.  A float64 restatement of that arithmetic (compact_expect.
    kernel_model_R) and the oracle, both against a long-double evaluation, on data and resamples made as sweep A makes
    them (synth seeded with T', edge_resamples: 3 distinct rows .. all S; T' = 208 is sweep A's own case, 8 and 50 are
    one- and four-tile shapes of their own): each stays within a tenth of the 1e-10 that sweeps A and B allow.
    Measured: restatement <= 1.5e-12 (3 distinct rows; <= 1e-14 from 12 on), oracle <= 1.2e-14."""
    mt = ce.m_tiles(Tp)
    S = S_SMALL_MT if mt <= 4 else S_LARGE_MT
    X, Y = synth(S, B, Tp, seed=Tp)
    inds, distinct = ce.edge_resamples(S, ce.stage_ksteps(mt), seed=Tp)
    spec = ref.Spec('behavioral', [S], 1)
    worst_model = worst_oracle = 0.0
    for i in range(inds.shape[1]):
        exact = ce.exact_R(X, Y, inds[:, i])
        worst_model = max(worst_model, _rel(ce.kernel_model_R(X, Y, inds[:, i]), exact))
        worst_oracle = max(worst_oracle, _rel(ref.gen_covcorr(spec, X[inds[:, i]], Y[inds[:, i]], spec.dummy), exact))
    _report("margin T'={}".format(Tp), raw_moment_arithmetic=worst_model, oracle=worst_oracle)
    assert worst_model <= 0.1 * RTOL_R and worst_oracle <= 0.1 * RTOL_R, (worst_model, worst_oracle)


# ----------------------------------------------------------------------------------------------------------------
# sweep A: every bootstrap variant at every stage edge
# ----------------------------------------------------------------------------------------------------------------

SWEEP_A = [13] + [16 * (m - 1) + r for m in range(2, 14) for r in (4, 5)] + [16, 64, 208]


def test_sweep_a_reaches_every_variant():
    assert len(SWEEP_A) == 28 and len(set(SWEEP_A)) == 28
    assert {(ce.m_tiles(tp), ce.has_tail(tp)) for tp in SWEEP_A} == \
        {(1, False)} | {(m, t) for m in range(2, 14) for t in (False, True)}


@gpu
@pytest.mark.parametrize('Tp', SWEEP_A)
def test_bootstrap_variant_at_every_stage_edge(Tp):
    """One group, one condition: T' = 16 (m - 1) + 4 is the last value with the 4x4x4 tail tile and + 5 the first
    without it, for m = 2..13 tiles; 13, 16, 64, 208 the one-tile variant, full last tiles and the bound.  The
    resamples (compact_expect.edge_resamples) draw exactly d distinct rows, d over {3, 4, 5, 4 KT, 4 KT + 1, 8 KT - 1,
    8 KT, 8 KT + 1, 12 KT, S}: one (partial) stage, a last k-step with one live row padded with row 0 -- which those
    resamples never draw -- an exact multiple of KT, one k-step into the next stage, all S rows; one over the last
    five rows of X, three ordinary draws.  compact_row_fraction is the only view of the row counts k_drawn_mask /
    k_split_rank hand the blocks."""
    mt = ce.m_tiles(Tp)
    S = S_SMALL_MT if mt <= 4 else S_LARGE_MT
    inds, distinct = ce.edge_resamples(S, ce.stage_ksteps(mt), seed=Tp)
    assert inds.shape[1] % 8 != 0
    _crosscov_vs_oracle("sweep A T'={} ({} tiles{})".format(Tp, mt, ', tail' if ce.has_tail(Tp) else ''), [S], 1, Tp,
                        inds, seed=Tp, fraction=ce.row_fraction(distinct, S))


@gpu
def test_past_the_bound_the_dense_blocks_run():
    """T' = 209 with both options set: no compact variant exists, the launch is dense and R is still right."""
    S = S_LARGE_MT
    inds, _ = ce.edge_resamples(S, 1, seed=209)
    _crosscov_vs_oracle("sweep A T'=209 (dense)", [S], 1, 209, inds, seed=209, compact=False)


# ----------------------------------------------------------------------------------------------------------------
# sweep B: cells, and the layouts of the moment-only blocks
# ----------------------------------------------------------------------------------------------------------------

# (groups, n_cond, T) -> resample counts whose (resample, cell) pairs fall into each class of moment_layout:
# <= 128 pairs one 16-tile block, 129..192 one 24-tile block, 193..256 two 16-tile blocks (the second partial)
SWEEP_B = [
    ([20, 20], 1, 58, (11, 70, 100)),               # T' = 116, J = 2: 22, 140, 200 pairs
    ([15, 15, 15], 1, 44, (11, 50, 70)),            # T' = 132, J = 3: 33, 150, 210 pairs
    ([12, 12], 2, 37, (11, 40, 60)),                # T' = 148, J = 4: 44, 160, 240 pairs
    ([6] * 8, 4, 6, (3, 5, 7)),                     # T' = 192, J = 32 (the bound on J): 96, 160, 224 pairs
    ([6] * 8, 4, 1, (3, 5, 7)),                     # T' = 32, one behaviour per cell
]


MOMENT_CLASSES = ((1, 128), (129, 192), (193, 256))


@gpu
@pytest.mark.parametrize('groups,n_cond,T,n,cls',
                         [(g, c, t, n, k) for g, c, t, ns in SWEEP_B for k, n in enumerate(ns)])
def test_cells_and_moment_block_layouts(groups, n_cond, T, n, cls):
    """Several cells (per-cell z-scores of Y, one 1 / std row per (resample, cell) pair, mom_idx = the row's cell) with
    ordinary gen_bootsamp draws; the number of resamples picks the moment-only launch: k_xprod<16, ., ., 8, 4> with one
    block, k_xprod<24, ., ., 12, 4>, or two 16-tile blocks of which the second is partly empty."""
    from pypyls_amd import resampling as rsmp
    J = len(groups) * n_cond
    assert MOMENT_CLASSES[cls][0] <= n * J <= MOMENT_CLASSES[cls][1], (n, J, cls)
    inds = np.asarray(rsmp.gen_bootsamp(groups, n_cond, n, seed=J * T, verbose=False))
    _crosscov_vs_oracle("sweep B T'={} J={} n={}".format(J * T, J, n), groups, n_cond, T, inds, seed=J * T)


@gpu
def test_more_than_32_cells_leave_the_compact_route():
    """33 cells: the block's scale tiles no longer fit (compact_boot_ok), the dense blocks run, R is still right."""
    from pypyls_amd import resampling as rsmp
    groups, n_cond, T = [6] * 11, 3, 2
    inds = np.asarray(rsmp.gen_bootsamp(groups, n_cond, 5, seed=33, verbose=False))
    _crosscov_vs_oracle("sweep B T'=66 J=33 (dense)", groups, n_cond, T, inds, seed=33, compact=False)


# ----------------------------------------------------------------------------------------------------------------
# sweep C: the chain behind each variant test_compact_blocks_equal_dense_blocks does not reach
# ----------------------------------------------------------------------------------------------------------------

SWEEP_C = [21, 36, 69, 84, 85, 101, 116, 132, 133, 148, 149, 164, 165, 181, 196]


@gpu
@pytest.mark.parametrize('Tp', SWEEP_C)
def test_chain_behind_the_compact_blocks(Tp):
    """eng.boot with the compact blocks forced, 11 ordinary bootstraps, data and S = 3 T' + 24 of
    test_gpu_boot_followers (whose checks these are): distrib -- columns [B, B + L) of R, which the compact blocks
    write from their last column blocks and sweep A does not gather -- at 1e-9 per LV, sum U and sum U^2 at 1e-8 per
    live LV, against ref.single_boot.  The oracle's U_r moves by <= 9.5e-15 per LV and its distrib by <= 3.1e-15
    under a 4e-16 perturbation of the data at these shapes (profiles/compact_blocks_parity.txt)."""
    from test_gpu_boot_followers import _Shape, _check_boot, B_SMALL
    assert B_SMALL == B
    case = "sweep C T'={} ({} tiles{})".format(Tp, ce.m_tiles(Tp), ', tail' if ce.has_tail(Tp) else '')
    sh = _Shape(Tp, B)
    figs = {}
    try:
        sh.eng.set_option('compact_boot_always', 1)
        boots = sh.samples('boot', 11, 5000 + Tp)
        usum, usq, dist, tm = sh.boot(boots)
        ce.pin_compact(tm, Tp, case)
        assert tm['xprod_launches'] == 1 and tm['xprod_resamples'] == 11, tm
        failures = _check_boot(sh, (usum, usq, dist), boots, 5000 + Tp, np.arange(11), figs)
    finally:
        sh.close()
        _report(case, **figs.get('boot', {}))
    assert not failures, '{}:\n  '.format(case) + '\n  '.join(failures)


# ----------------------------------------------------------------------------------------------------------------
# sweeps D and E: split-half blocks
# ----------------------------------------------------------------------------------------------------------------

S_SPLIT = 150


class _SplitData(object):
    """One group, one condition, S = 150: data, the original arrangement plus one permutation, and the oracle's
    correlations of the masks it is asked about (computed once per arrangement and mask set)."""

    def __init__(self, Tp, masks, seed):
        from pypyls_amd import resampling as rsmp
        self.Tp, self.groups = Tp, [S_SPLIT]
        self.X, self.Y = synth(S_SPLIT, B, Tp, seed=seed)
        self.spec = ref.Spec('behavioral', self.groups, 1)
        self.masks = masks                                                    # (S, ns), used for both arrangements
        self.perms = np.asarray(rsmp.gen_permsamp(self.groups, 1, 1, seed=seed + 1, verbose=False))

    def run(self, **options):
        """-> (ucorr, vcorr) (2, L, ns): original arrangement, permuted arrangement; how both passes ran: split_route()
        and last_timing()'s split_blocks (0 unfused, 1 dense fused, 5 / 8 compact blocks with that epilogue) and
        split_reader (waves per block of the one-pass reader, + 100 with the wave kinds in runs of four; 0 none)."""
        eng = _engine(self.groups, 1, self.X, self.Y, **options)

        def route():
            tm = eng.last_timing()
            return dict(split_route=eng.split_route(), split_blocks=tm.get('split_blocks'),
                        split_reader=tm.get('split_reader'))
        try:
            u0, v0 = eng.split_half(self.masks)
            r0 = route()
            u1, v1 = eng.split_half(self.masks[None], perms=self.perms)
            r1 = route()
        finally:
            eng.close()
        assert r0 == r1, 'the original and the permuted arrangement took different routes: {} / {}'.format(r0, r1)
        return np.concatenate([u0, u1]), np.concatenate([v0, v1]), r1

    def oracle(self):
        us, vs = [], []
        for Yp in (self.Y, self.Y[self.perms[:, 0]]):
            U, d, V = ref.decompose(self.spec, self.X, Yp)
            di = np.linalg.inv(d)
            uv = [ref.split_half(self.spec, self.X, Yp, U @ di, V @ di, self.masks[:, [i]])
                  for i in range(self.masks.shape[1])]
            us.append(np.stack([u for u, _ in uv], axis=-1))
            vs.append(np.stack([v for _, v in uv], axis=-1))
        return np.stack(us), np.stack(vs)


def _pin_split(got, what, **pinned):
    moved = {k: got.get(k) for k, v in pinned.items() if got.get(k) != v}
    assert not moved, (
        'path moved: {} reports {} where this test pins {} (full report: {}). The split-half kernels this case is '
        'written for no longer run at this shape: re-pin the case, or move it to a shape that still takes that '
        'path.'.format(what, moved, pinned, got))


def _worst_split(got, want):
    """worst over (arrangement, split) of max |got - want| / max |want| -- assert_close per split, as the split tests
    compare."""
    return max(_rel(got[p][:, i], want[p][:, i]) for p in range(got.shape[0]) for i in range(got.shape[2]))


SWEEP_D = [13, 20, 21, 36, 37, 52, 53, 64]


@gpu
@pytest.mark.parametrize('Tp', SWEEP_D)
def test_split_blocks_at_every_stage_edge(Tp):
    """First halves of exactly n1 rows, n1 over {3, 4, 5, 4 KT, 4 KT + 1, 8 KT, 8 KT + 1, S - 3} (compact_expect.
    first_half_masks; row 0 in no half whose size is no multiple of 4), original arrangement and one permutation.
    T' = 13, 53, 64 take epilogue 5 (pinned: split_blocks == 5, no reader); 20, 21, 36, 37, 52 epilogue 8 and the
    one-pass reader (split_blocks == 8, split_route() == 1), and epilogue 5 again under split_two_readers; the
    comparison runs under split_inblock are pinned to the dense fused blocks (split_blocks == 1).  That is
    k_xprod_compact<1..4, ., 5, .> with and without the tail and <2..4, ., 8, .> -- at four tiles the reader's
    T' <= 52 always has the tail.  ucorr / vcorr
    against ref.split_half at 1e-7 and against the dense fused layout (split_inblock) at 1e-9."""
    mt = ce.m_tiles(Tp)
    masks, counts = ce.first_half_masks(S_SPLIT, ce.stage_ksteps(mt), seed=Tp)
    data = _SplitData(Tp, masks, seed=Tp)
    reader = Tp in (20, 21, 36, 37, 52)
    case = "sweep D T'={} ({} tiles{})".format(Tp, mt, ', tail' if Tp - 16 * (mt - 1) <= 4 else '')
    runs = {'default': data.run()}
    if reader:
        _pin_split(runs['default'][2], case, split_route=1, split_blocks=8, split_reader=12)
        runs['split_two_readers'] = data.run(split_two_readers=1)
        _pin_split(runs['split_two_readers'][2], case + ', split_two_readers', split_route=0, split_blocks=5,
                   split_reader=0)
    else:
        _pin_split(runs['default'][2], case, split_route=0, split_blocks=5, split_reader=0)
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


SWEEP_E = [20, 21, 28, 32, 36, 37, 44, 48, 52]


@gpu
@pytest.mark.parametrize('Tp', SWEEP_E)
def test_split_reader8_forms_are_bit_equal(Tp):
    """Option split_reader8 selects the other compiled forms of the one-pass reader k_split_fused<NB> /
    k_split_fused12<NB>, NB = ceil(T'/4) = 5..13 row blocks: bit 0 the 8-wave block whose matrix waves build the tiles
    themselves ("same products, same order", include/plsx.h), bit 1 the wave -> role map, which moves roles between
    waves and no operand between sums.  7 ordinary splits, original arrangement and one permutation: values 1, 2, 3
    give the bits of value 0, and last_timing()'s split_reader says that each value launched its own form (12 / 8
    waves, + 100 for the wave kinds in runs of four)."""
    from pypyls_amd import resampling as rsmp
    masks = np.asarray(rsmp.gen_splits([S_SPLIT], 1, 7, seed=Tp))
    data = _SplitData(Tp, masks, seed=100 + Tp)
    base = data.run()
    case = "sweep E T'={} NB={}".format(Tp, -(-Tp // 4))
    _pin_split(base[2], case, split_route=1, split_blocks=8, split_reader=12)
    assert np.all(np.isfinite(base[0])) and np.all(np.isfinite(base[1]))
    figs, failures = {}, []
    for value in (1, 2, 3):
        uc, vc, route = data.run(split_reader8=value)
        _pin_split(route, '{}, split_reader8 = {}'.format(case, value), split_route=1, split_blocks=8,
                   split_reader={1: 8, 2: 112, 3: 108}[value])
        figs[str(value)] = max(_rel(uc, base[0]), _rel(vc, base[1]))
        if not (np.array_equal(uc, base[0]) and np.array_equal(vc, base[1])):
            failures.append('split_reader8 = {} differs from 0 (max rel diff {:.3e})'.format(value, figs[str(value)]))
    _report(case, max_rel_diff=figs)
    assert not failures, "sweep E T'={}: ".format(Tp) + '; '.join(failures)
