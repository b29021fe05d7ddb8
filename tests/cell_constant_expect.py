"""
Cell-constant features: the contract as numpy, on the hooks of oracle.cpu_ref.

A feature is cell-constant in (resample, cell) when the rows drawn into that cell hold bit-identical values.  The
reference z-scores it by a zero standard deviation (`xcorr`, pyls/compute.py:84-85; `rescale_test`,
pyls/compute.py:148-149) and returns NaN or inf; the oracle restates that (oracle/cpu_ref.py `xcorr` :55-69,
`_zscore_batch` :355-361, `_covcorr_rows` :386-407, `rescale_test` :495-502), and where the rounded mean of n equal
numbers misses them by an ulp it returns rounding garbage instead.  The device's rule is: z-score 0, everything else as
if the feature were not there.  `contract()` swaps those four hooks for versions that give a bit-constant feature column
a zero z-score and do the same arithmetic otherwise, so that every oracle entry built on them (`gen_covcorr`,
`single_perm`, `single_boot`, `batch_perm`, `batch_boot`, `split_half`, `single_crossval`, `run_plsc`) yields the
contract's expectation.  Behaviours that are constant on a cell stay what they are (NaN): `_yz_t` keeps the original
z-score.  Covariance mode scales nothing and is left alone.

The module also builds the data of the tests ("armed" columns: constants a kernel is likely to mis-scale) and emulates
the two rules the kernels had before the contract was pinned, to show that the armed data would have caught them.
"""
import contextlib

import numpy as np

from oracle import cpu_ref as ref


def bit_constant(A, axis=0):
    """True where every entry along ``axis`` has the bits of the first."""
    bits = np.ascontiguousarray(A, dtype=np.float64).view(np.int64)
    first = np.take(bits, [0], axis=axis)
    return np.all(bits == first, axis=axis)


def constant_cells(spec, X):
    """(J, B) bool: feature b is cell-constant in cell j of the (resampled) rows X."""
    return np.stack([bit_constant(X[c]) for c in spec.dummy.T.astype(bool)])


def _xcorr(X, Y, covariance=False):
    """oracle xcorr (cpu_ref.py:55-69) with the contract's rule for the columns of X."""
    X = np.asarray(X, dtype=float)
    Y = np.asarray(Y, dtype=float)
    if X.ndim != 2 or Y.ndim != 2 or len(X) != len(Y):
        raise ValueError('X and Y must be 2-D with the same number of rows')
    Xc = X - X.mean(axis=0)
    Yc = Y - Y.mean(axis=0)
    if not covariance:
        with np.errstate(divide='ignore', invalid='ignore'):
            Xc = Xc / X.std(axis=0, ddof=1)
            Yc = Yc / Y.std(axis=0, ddof=1)
        Xc[:, bit_constant(X)] = 0.0
    return (Yc.T @ Xc) / (len(X) - 1)


def _zscore_batch(A, covariance):
    """oracle _zscore_batch (cpu_ref.py:355-361) with the contract's rule."""
    Ac = A - A.mean(axis=-2, keepdims=True)
    if not covariance:
        with np.errstate(divide='ignore', invalid='ignore'):
            Ac = Ac / A.std(axis=-2, ddof=1, keepdims=True)
        Ac = np.where(bit_constant(A, axis=-2)[..., None, :], 0.0, Ac)
    return Ac


def _rescale_test(X_train, X_test, Y_train, U, V):
    """oracle rescale_test (cpu_ref.py:495-502): a feature that is constant on the training rows maps every test row
    to 0."""
    mu = X_train.mean(axis=0)
    sd = X_train.std(axis=0, ddof=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        X_resc = (X_test - mu) / sd
    X_resc[:, bit_constant(X_train) | (sd == 0)] = 0.0
    return (X_resc @ U @ V.T) + Y_train.mean(axis=0, keepdims=True)


@contextlib.contextmanager
def contract():
    """oracle.cpu_ref with the contract's rule in place of the reference's division by zero."""
    names = ('xcorr', '_zscore_batch', '_yz_t', '_covcorr_rows', 'rescale_test')
    saved = {k: getattr(ref, k) for k in names}
    zscore, covcorr_rows = saved['_zscore_batch'], saved['_covcorr_rows']

    def yz_t(spec, Y):                               # behaviours keep the reference's z-score
        return [np.ascontiguousarray(np.swapaxes(zscore(Y[:, c, :], spec.covariance), -1, -2))
                for c in ref._cell_slices(spec)]

    def rows(spec, X, Y, rows):                      # (raw moments, cpu_ref.py:403-405: zero the cells afterwards)
        with np.errstate(all='ignore'):
            out = covcorr_rows(spec, X, Y, rows)
        if not spec.covariance:
            T = Y.shape[1]
            for j, c in enumerate(ref._cell_slices(spec)):
                const = bit_constant(np.asarray(X, dtype=float)[rows[:, c]], axis=1)        # (n, B)
                out[:, j * T:(j + 1) * T, :] = np.where(const[:, None, :], 0.0, out[:, j * T:(j + 1) * T, :])
        return out

    ref.xcorr, ref._zscore_batch, ref._yz_t, ref._covcorr_rows, ref.rescale_test = \
        _xcorr, _zscore_batch, yz_t, rows, _rescale_test
    try:
        yield ref
    finally:
        for k, v in saved.items():
            setattr(ref, k, v)


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------

#: designs of the GPU tests: (groups, n_cond); [40] x 1: cell-constant means globally constant
DESIGNS = {'2g': ([20, 20], 1), '3c': ([12], 3), '1g': ([40], 1)}
N_CONST = 24
#: seeds of the armed data sets the GPU tests use
SEEDS = (0, 1, 2, 3)


class Armed(object):
    """X (S, B), Y (S, T) and where the armed columns are.

    dead     columns that are cell-constant in EVERY cell, whatever rows a within-cell resample draws: R is zero there,
             and every statistic equals that of ``X[:, keep]``
    partial  columns that are cell-constant in one cell and ordinary in the others
    sparse   the binary column with one non-zero row per cell (``sparse_rows``): constant in a bootstrap that misses
             the row
    keep     every column that is not dead
    """


def armed(design, B, T, seed=0):
    """The armed data of one design.  N_CONST columns of constants per cell -- 0.1, 1/3, random numbers times
    10^-3 .. 10^3 -- of which every second one is constant in ONE cell only; a binary column that is absent from
    cell 0 (its globally centred value there is -mu); the indicator of cell 0; a sparse binary column; an all-zero
    column; a globally constant non-zero column.  They sit at both ends of the feature range and in between."""
    groups, n_cond = DESIGNS[design] if isinstance(design, str) else design
    spec = ref.Spec('behavioral', groups, n_cond)
    rs = np.random.RandomState(seed)
    cells = [np.flatnonzero(c) for c in spec.dummy.T.astype(bool)]
    S, J = spec.dummy.shape
    X = rs.randn(S, B) + 3.0 * rs.rand(1, B)
    Y = rs.randn(S, T) + 1.5
    k = min(T, B)
    Y[:, :k] += 0.5 * X[:, :k]
    n_armed = N_CONST + 5
    assert B >= n_armed + 8
    cols = np.unique(np.r_[0, 1, B - 1, B - 2, rs.permutation(np.arange(2, B - 2))[:n_armed - 4]])
    cols = rs.permutation(cols)
    consts = np.r_[0.1, 1.0 / 3.0, rs.randn(N_CONST * J - 2) * 10.0 ** rs.randint(-3, 4, N_CONST * J - 2)]
    consts = rs.permutation(consts).reshape(N_CONST, J)
    out = Armed()
    dead, partial = [], []
    for i in range(N_CONST):
        b = cols[i]
        if i % 2 == 0 or J == 1:
            for j, rows in enumerate(cells):
                X[rows, b] = consts[i, j]
            dead.append(b)
        else:
            j = (i // 2) % J
            X[:, b] = consts[i, j] * (1.0 + 0.5 * rs.randn(S))   # ordinary in the other cells, around the same level:
            X[cells[j], b] = consts[i, j]                        # large per-cell offsets are another subject
            partial.append((b, j))
    b_absent, b_ind, b_sparse, b_zero, b_glob = cols[N_CONST:N_CONST + 5]
    X[:, b_absent] = (rs.rand(S) < 0.5).astype(float)
    for rows in cells[1:]:
        X[rows[:2], b_absent] = (0.0, 1.0)           # (never constant where it is present)
    X[cells[0], b_absent] = 0.0
    (dead if J == 1 else partial).append(b_absent if J == 1 else (b_absent, 0))
    X[:, b_ind] = 0.0
    X[cells[0], b_ind] = 1.0
    X[:, b_sparse] = 0.0
    out.sparse_rows = np.array([rows[rs.randint(len(rows))] for rows in cells])
    X[out.sparse_rows, b_sparse] = 1.0
    X[:, b_zero] = 0.0
    X[:, b_glob] = 3.7
    dead += [b_ind, b_zero, b_glob]
    out.spec, out.X, out.Y, out.groups, out.n_cond = spec, X, Y, list(groups), n_cond
    out.dead = np.array(sorted(dead))
    out.partial = sorted(partial)
    out.sparse = int(b_sparse)
    out.zero, out.glob, out.indicator = int(b_zero), int(b_glob), int(b_ind)
    out.keep = np.setdiff1d(np.arange(B), out.dead)
    out.cells = cells
    const = constant_cells(spec, X)
    assert const[:, out.dead].all() and all(const[j, b] for b, j in out.partial) and not const[:, b_sparse].any()
    assert const.sum() == J * len(out.dead) + len(out.partial)
    return out


def sparse_bootstraps(a, n, seed=0):
    """(S, n) within-cell bootstrap index arrays for armed data ``a``: resample i draws the non-zero row of the sparse
    column in cell j iff bit j of i is set -- so the column is constant in some cells of some resamples only."""
    rs = np.random.RandomState(seed)
    S = len(a.X)
    out = np.zeros((S, n), dtype=np.int64)
    for i in range(n):
        for j, rows in enumerate(a.cells):
            others = rows[rows != a.sparse_rows[j]]
            draw = others[rs.randint(len(others), size=len(rows))]
            if (i >> j) & 1:
                draw[rs.randint(len(rows))] = a.sparse_rows[j]
            out[rows, i] = draw
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the rules the kernels had before (emulated): scale = var > 0 ? 1 / sqrt(var) : 0
# ---------------------------------------------------------------------------------------------------------------------

def _centred(X):
    s = np.zeros(X.shape[1])
    for row in X:                                    # k_colmean: rows summed in order
        s = s + row
    return X - s / len(X)


def two_pass_scale(spec, X):
    """(J, B): the scale of the fixed-X route's former rule -- cell mean and squared deviations summed in row order
    over the globally centred X, var > 0."""
    Xc = _centred(np.asarray(X, dtype=float))
    out = []
    for c in spec.dummy.T.astype(bool):
        rows = Xc[c]
        s = np.zeros(X.shape[1])
        for r in rows:
            s = s + r
        mean = s / len(rows)
        q = np.zeros(X.shape[1])
        for r in rows:
            q = q + (r - mean) * (r - mean)
        var = q / (len(rows) - 1)
        with np.errstate(divide='ignore', invalid='ignore'):
            out.append(np.where(var > 0.0, 1.0 / np.sqrt(var), 0.0))
    return np.stack(out)


def raw_moment_scale(spec, X):
    """(J, B): the scale of the raw-moment sites' former rule -- (m2 - m1^2 / n) / (n - 1) > 0 with m1, m2 summed in
    row order over the globally centred X (the device's order differs; the rate at which the difference comes out
    positive does not depend on it much)."""
    Xc = _centred(np.asarray(X, dtype=float))
    out = []
    for c in spec.dummy.T.astype(bool):
        rows = Xc[c]
        n = len(rows)
        m1, m2 = np.zeros(X.shape[1]), np.zeros(X.shape[1])
        for r in rows:
            m1 = m1 + r
            m2 = m2 + r * r
        var = (m2 - m1 * m1 / n) / (n - 1.0)
        with np.errstate(divide='ignore', invalid='ignore'):
            out.append(np.where(var > 0.0, 1.0 / np.sqrt(var), 0.0))
    return np.stack(out)


def raw_moment_bound(n, cv):
    """The relative error a feature of within-cell coefficient of variation ``cv`` (std over root mean square of the
    globally centred values) may show on a raw-moment route: the difference m2 - m1^2 / n is known to 4 (n + 1) 2^-53
    m2 and the variance is cv^2 of m2 / n."""
    return 4.0 * (n + 1) * 2.0 ** -53 / cv ** 2
