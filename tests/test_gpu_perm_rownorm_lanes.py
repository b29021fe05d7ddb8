"""Projected permutations with transposed accumulators (k_xprod epilogue 10: MFMA operands exchanged, lane-local row
norms, 16 partials per row through LDS) and the chunked builder (k_build_A_proj: z-scores once per (row, behaviour)).

Reference: oracle.cpu_ref.single_perm per entry at 1e-9, the tolerance of the fixed-X permutation tests.  Every case
asserts that the projected route ran.  Shapes (the data of a shape is _data(S, B, T, seed = S + T + B)):

* every column slot of a block: column c of a 64-column block sits in wave c / 16, register (c % 16) / 4, lane row
  c % 4.  T' = 1 and T' = 2 at S = 24, B from 1 to 65: each B adds columns to slots the B before it left empty, and a
  dropped or doubled slot changes a norm by far more than 1e-9.
* every row slot: T' = T = 50 fills the 400 rows of a group (25 tiles x 16 lanes, no padding row) at two (S = 56) and
  three (S = 72) k-steps per stage; n = 9 makes a second group that holds one permutation.
* zero rows inside the last live tile: nine permutations of T' = 7 (63 rows: 15 of the fourth tile's 16) and of
  T' = 10 (two cells of 33; 90 rows: 10 of the sixth tile's 16); the rows behind them carry no resample.
* builder chunks of 64 rows: cells of 63, 64, 65, 129 and 2 x 65 rows, and four cells of 16; the builder's other
  paths: chunks of 52 rows (T = L = 55) and V0 read from global memory (T = L = 56).
* bits: run twice, each permutation alone, another slot order and the pre-permuted stack give the same bits.

Margins on the CPU (oracle alone) for these shapes and seeds: every original spectrum has d_min / d_max >= 5.07e-4
(the route needs every LV live at 1e-6), and the expected values of a case span at most a factor 31.1.
"""
import numpy as np
import pytest

from oracle import cpu_ref as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def _data(S, B, T, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T)
    k = min(B, T)
    Y[:, :k] += 0.4 * X[:, :k]
    return X, Y


def _bind(X, Y, groups, n_cond, options=None, scratch_gb=None, method=0, contrasts=None):
    """A bound engine on the feature-pass permutation route with the device's own decomposition as the original."""
    from pypyls_amd import hostmath, resampling as rsmp
    from pypyls_amd.engine import Engine
    eng = Engine(options=options, scratch_gb=scratch_gb)
    eng.set_data(X, Y, rsmp.cell_of_row(groups, n_cond), len(groups), n_cond, method)
    if contrasts is not None:
        eng.set_contrasts(contrasts)
    xw, sv, yw = eng.decompose()
    xw, yw = hostmath.sign_convention(xw, yw)
    eng.set_original(xw, sv, yw)
    eng.set_perm_path(False)
    return eng, xw, sv, yw


def _assert_entries(got, want, what):
    rel = np.abs(got - want) / np.abs(want)
    assert np.all(rel <= RTOL), '{}: entry {} rel err {:.3e}'.format(what, np.unravel_index(np.argmax(rel), rel.shape),
                                                                    rel.max())
    return rel.max()


COLUMN_B = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
ROW_B = [50, 51, 52, 63, 64, 65, 127, 128, 129]

# (S, T, groups, n_cond, B, n)
COLUMN_SLOTS = [(24, T, [24], 1, B, 9) for T in (1, 2) for B in COLUMN_B if B >= T]
ROW_SLOTS = [(S, 50, [S], 1, B, 9) for S in (56, 72) for B in ROW_B]
PADDING_ROWS = [(64, 7, [64], 1, 40, 9), (66, 5, [33, 33], 1, 40, 9)]
BUILDER_CHUNKS = [
    (63, 2, [63], 1, 40, 9),
    (64, 7, [64], 1, 40, 9),
    (65, 2, [65], 1, 40, 9),
    (129, 1, [129], 1, 40, 9),
    (130, 3, [65, 65], 1, 40, 9),
    (64, 2, [16, 16], 2, 40, 9),
]
# the builder's other paths: a chunk shorter than 64 rows (T = L = 55: 52 rows, so 72 rows are two chunks) and the
# block of V0 left in global memory (T L > 3072: T = L = 56)
BUILDER_PATHS = [
    (72, 55, [72], 1, 64, 9),
    (72, 56, [72], 1, 64, 9),
]


def _run_shape(S, T, groups, n_cond, B, n):
    from pypyls_amd import resampling as rsmp
    X, Y = _data(S, B, T, seed=S + T + B)
    eng, xw, sv, yw = _bind(X, Y, groups, n_cond)
    try:
        assert eng.L == eng.Tp, 'the shape is meant to have L == T\''
        perms = rsmp.gen_permsamp(groups, n_cond, n, seed=B, verbose=False)
        eng.set_timing(True)
        got = eng.perm(perms)
        tm = eng.last_timing()
        eng.set_timing(False)
    finally:
        eng.close()
    assert tm['perm_projected'] == 1, tm
    spec = ref.Spec('behavioral', groups, n_cond)
    want = np.stack([ref.single_perm(spec, X, Y, perms[:, i], yw)[0] for i in range(n)], -1)
    what = 'S {} T {} groups {} n_cond {} B {} n {}'.format(S, T, groups, n_cond, B, n)
    worst = _assert_entries(got, want, what)
    print('row norms from transposed tiles, {}: worst entry rel err {:.2e}'.format(what, worst))


@pytest.mark.parametrize('S,T,groups,n_cond,B,n', COLUMN_SLOTS)
def test_every_column_slot(S, T, groups, n_cond, B, n):
    _run_shape(S, T, groups, n_cond, B, n)


@pytest.mark.parametrize('S,T,groups,n_cond,B,n', ROW_SLOTS)
def test_every_row_slot(S, T, groups, n_cond, B, n):
    _run_shape(S, T, groups, n_cond, B, n)


@pytest.mark.parametrize('S,T,groups,n_cond,B,n', PADDING_ROWS)
def test_padding_rows_in_the_last_tile(S, T, groups, n_cond, B, n):
    _run_shape(S, T, groups, n_cond, B, n)


@pytest.mark.parametrize('S,T,groups,n_cond,B,n', BUILDER_CHUNKS)
def test_builder_chunks(S, T, groups, n_cond, B, n):
    _run_shape(S, T, groups, n_cond, B, n)


@pytest.mark.parametrize('S,T,groups,n_cond,B,n', BUILDER_PATHS)
def test_builder_paths(S, T, groups, n_cond, B, n):
    _run_shape(S, T, groups, n_cond, B, n)


def test_bits():
    """T' = 50, B = 129, 19 permutations: the batch twice, each permutation alone, another slot order and the
    perm_ystack route give the same bits."""
    from pypyls_amd import resampling as rsmp
    S, T, B, n = 72, 50, 129, 19
    X, Y = _data(S, B, T, seed=50)
    perms = rsmp.gen_permsamp([S], 1, n, seed=51, verbose=False)
    eng, xw, sv, yw = _bind(X, Y, [S], 1)
    try:
        eng.set_timing(True)
        got = eng.perm(perms)
        tm = eng.last_timing()
        twice = eng.perm(perms)
        alone = np.stack([eng.perm(perms[:, i:i + 1])[:, 0] for i in range(n)], -1)
        order = np.r_[np.arange(11, 19), np.arange(0, 11)]            # every permutation in another slot and group
        moved = eng.perm(perms[:, order])
        stack = eng.perm_ystack(np.stack([Y[perms[:, i]] for i in range(n)]), rotate=True)
        tm_stack = eng.last_timing()
        eng.set_timing(False)
    finally:
        eng.close()
    assert tm['perm_projected'] == 1 and tm_stack['perm_projected'] == 1, (tm, tm_stack)
    spec = ref.Spec('behavioral', [S], 1)
    want = np.stack([ref.single_perm(spec, X, Y, perms[:, i], yw)[0] for i in range(n)], -1)
    _assert_entries(got, want, 'bits case')
    assert np.array_equal(twice, got)
    assert np.array_equal(alone, got)
    assert np.array_equal(moved, got[:, order])
    assert np.array_equal(stack, got)
