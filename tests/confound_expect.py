"""Expected values of pls_regression(confounds=Z), written in numpy on the CPU oracle: the residuals of X and Y on
[1, Z], the cross-validation with the confound regression fitted on the training rows of every split (built on
tests/regression_cv_expect.py: ``cv_expected`` on that split's residuals), and its permutation null (definition 4 of
the feature: the residualised Y is permuted and residualised again per fold) with the p-value rule of
tests/regression_cv_perm_expect.py.  Shared by tests/test_confound_host.py and tests/test_gpu_confound.py; not a test
module."""
import numpy as np

from regression_cv_expect import cv_expected, abs_err, rel_err  # noqa: F401  (re-exported for the tests)
from regression_cv_perm_expect import split_means, pvals_of


def usable_rows(X, Y, Z):
    """A row is usable iff it is not NaN throughout in X, in Y or in Z."""
    X, Y, Z = np.asarray(X, dtype=float), np.asarray(Y, dtype=float), np.asarray(Z, dtype=float).reshape(len(X), -1)
    return ~(np.isnan(X).all(axis=1) | np.isnan(Y).all(axis=1) | np.isnan(Z).all(axis=1))


def design(Z, rows=None):
    """[1, Z] (S, q + 1); rows outside ``rows`` are zero."""
    Z = np.asarray(Z, dtype=float).reshape(len(Z), -1)
    D = np.c_[np.ones(len(Z)), Z]
    if rows is not None:
        D = np.where(np.asarray(rows, dtype=bool)[:, None], D, 0.0)
    return D


def residualise(A, Z, rows):
    """A (S, n) minus its least-squares fit on [1, Z] over ``rows`` (bool), applied to EVERY row of A."""
    A = np.asarray(A, dtype=float)
    D = design(Z)
    G = np.linalg.lstsq(D[rows], A[rows], rcond=None)[0]
    return A - D @ G


def _fold(X, Y, Z, tr, ok):
    """The data of one split: X and Y residualised by the regression of its usable training rows, unusable rows NaN."""
    Zf = np.where(ok[:, None], np.asarray(Z, dtype=float).reshape(len(X), -1), 0.0)
    Xs = residualise(np.where(ok[:, None], X, 0.0), Zf, tr & ok)
    Ys = residualise(np.where(ok[:, None], Y, 0.0), Zf, tr & ok)
    Xs[~ok], Ys[~ok] = np.nan, np.nan
    return Xs, Ys


def _stack(parts):
    return {key: np.concatenate([p[key] for p in parts], axis=-1) for key in parts[0]}


def cv_expected_confound(X, Y, Z, masks, k):
    """cv_expected with the confound regression fitted per split: for split s an lstsq of X and of Y on [1, Z] over its
    training rows, ALL rows residualised by it, then cv_expected on that one split.  Same keys and shapes."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    masks = np.asarray(masks, dtype=bool)
    ok = usable_rows(X, Y, Z)
    parts = []
    for s in range(masks.shape[1]):
        Xs, Ys = _fold(X, Y, Z, masks[:, s], ok)
        parts.append(cv_expected(Xs, Ys, masks[:, s:s + 1], k))
    return _stack(parts)


def cv_expected_global(X, Y, Z, masks, k):
    """The shortcut the feature exists to avoid: residuals taken once over the whole cohort, then cv_expected."""
    ok = usable_rows(X, Y, Z)
    Xr, Yr = _fold(np.asarray(X, dtype=float), np.asarray(Y, dtype=float), Z, ok, ok)
    return cv_expected(Xr, Yr, masks, k)


def cv_perm_expected_confound(X, Y, Z, masks, perms, k):
    """The null of cv_expected_confound: Y_{s,p} = M_s (Y_r[perm_p]) with Y_r the whole-cohort residuals of Y, X_s = M_s X;
    per permutation the mean over the splits.  Complete data only.  Returns dict(obs, null, pvals) as cv_perm_expected.
    The observed statistic is taken by the same arithmetic, as the identity arrangement M_s Y_r (= M_s Y to rounding):
    an identity column among ``perms`` then ties with it exactly, here as on the device, and the strict comparison of
    the p-value rule does not hang on rounding."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    masks, perms = np.asarray(masks, dtype=bool), np.asarray(perms)
    allr = np.ones(len(X), dtype=bool)
    Yr = residualise(Y, Z, allr)

    def arrangement(perm):
        parts = []
        for s in range(masks.shape[1]):
            tr = masks[:, s]
            parts.append(cv_expected(residualise(X, Z, tr), residualise(Yr[perm], Z, tr), masks[:, s:s + 1], k))
        return split_means(_stack(parts))
    obs = arrangement(np.arange(len(X)))
    out = [arrangement(perms[:, p]) for p in range(perms.shape[1])]
    null = {key: np.stack([o[key] for o in out], axis=-1) for key in ('r', 'r2', 'mse')}
    return dict(obs=obs, null=null, pvals=pvals_of(obs, null))
