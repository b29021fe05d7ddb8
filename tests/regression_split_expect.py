"""Expected values of pls_regression's split-half reliability (``n_split``), written on the CPU oracle
(oracle/cpu_ref.py: simpls, efficient_corr, get_mask) in feature space: BasePLS.split_half (pyls/base.py:366-397)
with the x_weights and y_loadings of SIMPLS in place of the singular vectors.  Shared by
tests/test_regression_split_host.py, tests/test_gpu_regression_split.py and tests/golden/make_split_golden.py; not a
test module."""
import warnings

import numpy as np

from oracle import cpu_ref as ref


def half_crosscov(X, Y):
    """D = (Y - ybar)^T (X - xbar), (T, B): the cross-covariance of one half without its 1 / (n - 1)."""
    return (Y - Y.mean(axis=0)).T @ (X - X.mean(axis=0))


def split_expected(X, Y, masks, k, perm=None, simpls=None, efficient_corr=None, get_mask=None):
    """X (S, B), Y (S, T), masks (S, n) bool with True = first half, perm (S,) or None: the arrangement is
    (X, Y[perm]).  Rows masked by get_mask(X, Y[perm]) belong to neither half.  Returns ucorr, vcorr (k, n): per split
    efficient_corr(D1^T Q, D2^T Q) over the features and efficient_corr(D1 W, D2 W) over the behaviours, with W, Q the
    x_weights and y_loadings of the k-component SIMPLS fit on all usable rows.  ``simpls`` / ``efficient_corr`` /
    ``get_mask``: other implementations of the three (the fixture generator passes the reference's own)."""
    simpls = simpls or (lambda x, y, c: ref.simpls(x, y, c))
    efficient_corr = efficient_corr or ref.efficient_corr
    get_mask = get_mask or ref.get_mask
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    if perm is not None:
        Y = Y[np.asarray(perm)]
    masks = np.asarray(masks, dtype=bool)
    ok = get_mask(X, Y)
    fit = simpls(X[ok], Y[ok], k)
    W, Q = fit['x_weights'], fit['y_loadings']
    n = masks.shape[1]
    ucorr, vcorr = np.zeros((k, n)), np.zeros((k, n))
    for s in range(n):
        h1, h2 = masks[:, s] & ok, ~masks[:, s] & ok
        D1, D2 = half_crosscov(X[h1], Y[h1]), half_crosscov(X[h2], Y[h2])
        with np.errstate(divide='ignore', invalid='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)          # (T = 1: the variance of one value)
            ucorr[:, s] = efficient_corr(D1.T @ Q, D2.T @ Q)
            vcorr[:, s] = efficient_corr(D1 @ W, D2 @ W)
    return ucorr, vcorr


def split_null(X, Y, perm_masks, perms, k, **impl):
    """perm_masks (P, S, n), perms (S, P): split_expected per permutation, stacked (P, k, n)."""
    out = [split_expected(X, Y, perm_masks[p], k, perm=np.asarray(perms)[:, p], **impl) for p in range(len(perm_masks))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def pvals_of(obs, null):
    """obs (k,), null (k, P): (#{null > obs} + 1) / (P + 1), strict (compute.perm_sig)."""
    return (np.sum(null > obs[:, None], axis=1) + 1) / (null.shape[1] + 1)


def corr_err(got, want):
    """max |got - want| over the entries where ``want`` is a number; the NaN of a side without variance must be NaN in
    both."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), 'NaN pattern differs: got {} NaN, want {}'.format(int(np.isnan(got).sum()),
                                                                                              int(nan.sum()))
    return float(np.max(np.abs(got - want)[~nan])) if (~nan).any() else 0.0
