"""Helpers of tests/test_gpu_compact_blocks.py: the compiled variants of k_xprod_compact, resamples and split masks
that put a block's contraction length on every edge of its stage loop, the route pin, and a CPU restatement of the
kernel's raw-moment arithmetic.  Not a test module."""
import numpy as np


def m_tiles(Tp):
    return -(-Tp // 16)


def has_tail(Tp):
    """The last tile holds <= 4 live rows and runs on the 4x4x4 shape (launch_cboot; T' <= 16 has no tail form)."""
    mt = m_tiles(Tp)
    return mt >= 2 and Tp - 16 * (mt - 1) <= 4


def stage_ksteps(mt):
    """k-steps per LDS stage of the compact blocks of mt tiles (launch_cboot / launch_csplit; PLSX_CKT = 3 at 4)."""
    return 3 if mt == 4 else max(1, 12 // mt)


def edge_counts(KT, S):
    """Row counts that put ksteps = ceil(d / 4) and nkt = ceil(ksteps / KT) on every edge of the stage loop: a single
    (partial) stage, a last k-step with one live row, an exact stage, one k-step / one row into the second stage, the
    last k-step of the second stage missing, two exact stages, one row into the third, three exact stages, all S."""
    want = [3, 4, 5, 4 * KT, 4 * KT + 1, 8 * KT - 1, 8 * KT, 8 * KT + 1, 12 * KT, S]
    out = []
    for d in want:
        d = int(min(max(d, 1), S))
        if d not in out:
            out.append(d)
    return out


def draw_exactly(rs, S, rows):
    """An index array of S draws over exactly the rows `rows`: each at least once, the rest on random ones of them;
    sorted, as gen_bootsamp's are."""
    rows = np.asarray(rows, dtype=int)
    assert 1 <= len(rows) <= S
    inds = np.concatenate([rows, rows[rs.randint(len(rows), size=S - len(rows))]])
    return np.sort(inds)


def edge_resamples(S, KT, seed, n_plain=3):
    """-> inds (S, n) int, distinct (n,): one resample per edge count (edge_counts) whose d rows are random ones --
    never row 0 when d is no multiple of 4, so that the padding entries of the row table point at a row the oracle
    does not use -- one over the LAST 5 rows of X, `n_plain` ordinary draws with replacement, and one more when that
    makes a multiple of 8 (the last sweep of eight groups is then partial)."""
    rs = np.random.RandomState(seed)
    cols = []
    for d in edge_counts(KT, S):
        if d == S:
            rows = np.arange(S)
        elif d % 4:
            rows = 1 + rs.permutation(S - 1)[:d]
        else:
            rows = rs.permutation(S)[:d]
        cols.append(draw_exactly(rs, S, rows))
    cols.append(draw_exactly(rs, S, np.arange(S - 5, S)))
    for _ in range(n_plain):
        cols.append(np.sort(rs.randint(S, size=S)))
    if len(cols) % 8 == 0:
        cols.append(np.sort(rs.randint(S, size=S)))
    inds = np.stack(cols, axis=1)
    distinct = np.array([len(np.unique(inds[:, i])) for i in range(inds.shape[1])])
    edges = edge_counts(KT, S)
    assert list(distinct[:len(edges)]) == edges and distinct[len(edges)] == 5
    for i, d in enumerate(distinct[:len(edges) + 1]):
        assert d % 4 == 0 or d == S or 0 not in inds[:, i], (i, d)
    return inds, distinct


def row_fraction(distinct, S):
    """compact_row_fraction of a launch whose blocks contract over `distinct` rows: whole k-steps of 4."""
    distinct = np.asarray(distinct)
    return float(np.mean(4 * ((distinct + 3) // 4))) / S


def first_half_masks(S, KT, seed):
    """(S, n) bool split masks whose first half has exactly n1 rows, n1 over the stage edges (3, 4, 5, 4 KT, 4 KT + 1,
    8 KT, 8 KT + 1) and S - 3 (a second half of three rows); row 0 is in no first half whose size is no multiple of
    4."""
    rs = np.random.RandomState(seed)
    counts = []
    for n1 in [3, 4, 5, 4 * KT, 4 * KT + 1, 8 * KT, 8 * KT + 1, S - 3]:
        if 3 <= n1 <= S - 3 and n1 not in counts:
            counts.append(n1)
    masks = np.zeros((S, len(counts)), dtype=bool)
    for i, n1 in enumerate(counts):
        rows = (1 + rs.permutation(S - 1)[:n1]) if n1 % 4 else rs.permutation(S)[:n1]
        masks[rows, i] = True
    assert list(masks.sum(axis=0)) == counts
    return masks, counts


def pin_compact(tm, Tp, what):
    """The launch behind last_timing() `tm` ran compact blocks of ceil(T'/16) tiles, one resample each."""
    pinned = dict(resamples_per_group=1, m_tiles=m_tiles(Tp))
    moved = [k for k, v in pinned.items() if tm.get(k) != v]
    if not tm.get('compact_row_fraction', 0.0) > 0.0:
        moved.insert(0, 'compact_row_fraction')
    assert not moved, (
        'path moved: {} reports {} where this test pins compact_row_fraction > 0, {} (full report: {}). The compact '
        'cross-product variant this case is written for no longer runs at this shape: re-pin the case, or move it to '
        'a shape that still takes that path.'.format(what, {k: tm.get(k) for k in moved}, pinned, tm))


def pin_dense(tm, what):
    assert tm.get('compact_row_fraction') == 0.0, (
        'path moved: {} reports compact_row_fraction = {} where this test pins the dense blocks (full report: {}): '
        're-pin the case.'.format(what, tm.get('compact_row_fraction'), tm))


# ----------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic on the CPU (one cell, correlation mode)
# ----------------------------------------------------------------------------------------------------------------

def kernel_model_R(X, Y, inds, dtype=np.float64):
    """R (T, B) of the bootstrap `inds` the way the compact route forms it, in `dtype`: Y z-scored over the draws
    (two-pass mean / variance, k_build_A_behav), multiplicities folded into the operand, the contraction over the
    distinct rows of the globally column-centred X, and 1 / std of the resampled feature from its RAW moments
    m1 = sum w x, m2 = sum w x^2 (k_xprod EPI 4): var = (m2 - m1^2 / n) / (n - 1).  dtype = np.longdouble gives the
    same formulas in extended precision; that they agree is what bounds the cancellation in `var`."""
    X = np.asarray(X, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    n = dtype(len(inds))
    Xc = X - X.sum(axis=0) / dtype(len(X))
    rows, w = np.unique(inds, return_counts=True)
    w = w.astype(dtype)
    Yr = Y[inds]
    mean = Yr.sum(axis=0) / n
    rstd = 1 / np.sqrt(((Yr - mean) ** 2).sum(axis=0) / (n - 1))
    A = (w[:, None] * (Y[rows] - mean) * rstd / (n - 1)).T          # (T, d)
    xs = Xc[rows]
    C = A @ xs if dtype is np.float64 else _matmul(A, xs)
    m1 = (w[:, None] * xs).sum(axis=0)
    m2 = (w[:, None] * xs * xs).sum(axis=0)
    var = (m2 - m1 * m1 / n) / (n - 1)
    return C / np.sqrt(var)


def _matmul(A, Bm):
    """(numpy has no BLAS for long double: a plain sum of outer products)"""
    out = np.zeros((A.shape[0], Bm.shape[1]), dtype=A.dtype)
    for k in range(A.shape[1]):
        out += A[:, k:k + 1] * Bm[k:k + 1, :]
    return out


def exact_R(X, Y, inds):
    """The correlations of the resampled columns, every step in long double on the centred resample (no raw moments)."""
    Xr = np.asarray(X, dtype=np.longdouble)[inds]
    Yr = np.asarray(Y, dtype=np.longdouble)[inds]
    n = np.longdouble(len(inds))
    Xz = Xr - Xr.sum(axis=0) / n
    Yz = Yr - Yr.sum(axis=0) / n
    Xz = Xz / np.sqrt((Xz * Xz).sum(axis=0))
    Yz = Yz / np.sqrt((Yz * Yz).sum(axis=0))
    return _matmul(Yz.T.copy(), Xz)
