"""Expected values of pls_regression's permutation test of the cross-validation (``cv_perm``), written on the CPU
oracle: for each permutation the whole cross-validation of tests/regression_cv_expect.py on ``(X, Y[perm])`` under the
same masks, then the plain mean over the splits; the p-values from the oracle's own observed and null values.  Shared
by tests/test_regression_cv_perm_host.py, tests/test_gpu_regression_cv_perm.py and
tests/golden/make_cv_perm_golden.py; not a test module."""
import numpy as np

from regression_cv_expect import cv_expected, abs_err, rel_err  # noqa: F401  (re-exported for the tests)


def split_means(cv):
    """dict(r, r2, mse) of cv_expected (or of a reference run) -> their means over the splits: (T, k), (T, k), (k + 1,)."""
    with np.errstate(invalid='ignore'):
        return dict(r=np.mean(cv['r'], axis=-1), r2=np.mean(cv['r2'], axis=-1), mse=np.mean(cv['mse'], axis=-1))


def null_of(cv_fn, X, Y, masks, perms, k):
    """cv_fn(X, Y[perm], masks, k) per column of perms (S, P), split-means stacked: r, r2 (T, k, P), mse (k + 1, P)."""
    perms = np.asarray(perms)
    out = [split_means(cv_fn(X, np.asarray(Y)[perms[:, p]], masks, k)) for p in range(perms.shape[1])]
    return {key: np.stack([o[key] for o in out], axis=-1) for key in ('r', 'r2', 'mse')}


def pvals_of(obs, null):
    """(#{null > obs} + 1) / (P + 1) on r and r2, (#{null < obs} + 1) / (P + 1) on mse; both strict."""
    P = null['r'].shape[-1]
    return dict(r=(np.sum(null['r'] > obs['r'][..., None], axis=-1) + 1) / (P + 1),
                r2=(np.sum(null['r2'] > obs['r2'][..., None], axis=-1) + 1) / (P + 1),
                mse=(np.sum(null['mse'] < obs['mse'][..., None], axis=-1) + 1) / (P + 1))


def cv_perm_expected(X, Y, masks, perms, k):
    """X (S, B), Y (S, T), masks (S, n) bool (True = training row), perms (S, P).  Returns dict(obs, null, pvals), each a
    dict over 'r', 'r2', 'mse'.  Rows masked by get_mask(X, Y[perm]) belong to neither side of any split."""
    obs = split_means(cv_expected(X, Y, masks, k))
    null = null_of(cv_expected, X, Y, masks, perms, k)
    return dict(obs=obs, null=null, pvals=pvals_of(obs, null))


def gaps(obs, null):
    """Smallest distance of an observed split-mean from any null value: absolute on r, relative to max(1, |v|) on r2
    and mse -- the form the device tolerance takes."""
    out = {}
    for key in ('r', 'r2', 'mse'):
        d = np.abs(null[key] - obs[key][..., None])
        if key != 'r':
            d = d / np.maximum(1.0, np.abs(obs[key][..., None]))
        out[key] = float(np.min(d))
    return out


def null_errs(got_r, got_r2, got_mse, null):
    return dict(r=abs_err(got_r, null['r']), r2=rel_err(got_r2, null['r2']), mse=rel_err(got_mse, null['mse']))
