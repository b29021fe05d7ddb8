"""Expected values of behavioral_pls / meancentered_pls(weights_ci=m), written on the hooks of the CPU oracle
(oracle/cpu_ref.py: single_boot, batch_boot, gen_covcorr): the per-bootstrap rotated weights U_b whose sums give the
bootstrap ratios, kept, and numpy's percentiles of them; and numpy's answer to the closing entry alone
(plsx_boot_weights_ci) for ANY stack of rotation operands.  Shared by tests/test_weights_ci_host.py and
tests/test_gpu_weights_ci.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref


def spec_of(method, groups, n_cond=1, covariance=False, mean_centering=0):
    return ref.Spec(method, groups, n_cond, covariance, mean_centering)


def original(spec, X, Y=None):
    """(x_weights (B, L), d (L, L)) of the original data, as run_plsc decomposes it."""
    Y = spec.dummy if spec.method == 'meancentered' else np.asarray(Y, dtype=float)
    U, d, _ = ref.decompose(spec, np.asarray(X, dtype=float), Y)
    return U, d


def weights_boot(spec, X, Y, inds, x_weights, d_orig):
    """(B, L, n): U_b of every column of ``inds`` (S, n) -- ``single_boot(...)[1]``, what run_plsc sums into the
    bootstrap ratios.  Behavioural PLS through the batched restatement, mean-centred PLS bootstrap by bootstrap."""
    X = np.asarray(X, dtype=float)
    inds = np.asarray(inds)
    if spec.method == 'behavioral':
        return ref.batch_boot(spec, X, np.asarray(Y, dtype=float), inds, x_weights, d_orig, sums=False)[1]
    Y = spec.dummy
    return np.stack([ref.single_boot(spec, X, Y, inds[:, i], x_weights, d_orig)[1] for i in range(inds.shape[1])], -1)


def ci_of(series, ci=95, weights=None):
    """series (B, L, n) -> (B, L, 2): np.percentile over the bootstraps, [..., 0] lower, [..., 1] upper (numpy's default
    linear interpolation; the original fit is not part of the series).  weights (n,) ints: how often each bootstrap
    counts (the replication trick of the batch-geometry tests): the series is the bootstraps repeated."""
    series = np.asarray(series, dtype=float)
    if weights is not None:
        series = np.repeat(series, np.asarray(weights, dtype=int), axis=-1)
    low = (100 - ci) / 2
    lo, hi = np.percentile(series, [low, 100 - low], axis=-1)
    return np.stack([lo, hi], axis=-1)


def weights_ci_expected(spec, X, Y, inds, m=None, ci=95, weights=None):
    U, d = original(spec, X, Y)
    boot = weights_boot(spec, X, Y, inds, U, d)
    return ci_of(boot if m is None else boot[:, :m], ci=ci, weights=weights)


def stack_series(spec, X, Y, rows, M):
    """(B, m, n): U_b = R_b^T M_b^T of the closing entry alone.  rows (n, S) index rows, M (n, m, T') ANY stack.  R_b is
    the cross-covariance matrix of the resampled rows as gen_covcorr forms it from X[rows[b]] itself -- two-pass
    z-scores, no raw moments."""
    X = np.asarray(X, dtype=float)
    Y = spec.dummy if spec.method == 'meancentered' else np.asarray(Y, dtype=float)
    out = []
    for r, Mb in zip(np.asarray(rows), np.asarray(M, dtype=float)):
        R = ref.gen_covcorr(spec, X[r], Y[r], spec.dummy)          # (T', B)
        out.append(R.T @ Mb.T)                                     # (B, m)
    return np.stack(out, axis=-1)


def stack_ci(spec, X, Y, rows, M, ci=95):
    """numpy's answer to plsx_boot_weights_ci -> (B, m, 2)."""
    return ci_of(stack_series(spec, X, Y, rows, M), ci=ci)


def within_cell_rows(spec, n, rs):
    """(n, S) random bootstrap index rows that resample inside every cell; a draw with fewer than two distinct subjects
    in a cell (no variance to scale by) is drawn again."""
    S = spec.dummy.shape[0]
    rows = np.zeros((n, S), dtype=np.int64)
    for c in spec.dummy.T.astype(bool):
        idx = np.flatnonzero(c)
        for i in range(n):
            while True:
                draw = idx[rs.randint(len(idx), size=len(idx))]
                if len(np.unique(draw)) >= min(2, len(idx)):
                    break
            rows[i, idx] = draw
    return rows
