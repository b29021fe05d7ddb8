"""Expected values of pls_regression's cross-validation, written on the CPU oracle (oracle/cpu_ref.py: simpls,
efficient_corr, r2_score_raw, get_mask).  Shared by tests/test_regression_cv_host.py, tests/test_gpu_regression_cv.py
and tests/golden/make_cv_golden.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref


def cv_expected(X, Y, masks, k):
    """X (S, B), Y (S, T), masks (S, n) bool with True = training row.  Rows masked by get_mask belong to neither side.
    Returns dict(r (T, k, n), r2 (T, k, n), sse (T, k + 1, n), mse (k + 1, n), n_test (n,)): the test rows predicted
    by the first c = 1 .. k SIMPLS components of the training rows plus the intercept; row 0 of sse / mse is the
    intercept-only model."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    masks = np.asarray(masks, dtype=bool)
    ok = ref.get_mask(X, Y)
    T, n = Y.shape[1], masks.shape[1]
    r, r2 = np.zeros((T, k, n)), np.zeros((T, k, n))
    sse, n_test = np.zeros((T, k + 1, n)), np.zeros(n, dtype=int)
    for s in range(n):
        tr, te = masks[:, s] & ok, ~masks[:, s] & ok
        fit = ref.simpls(X[tr], Y[tr], k)
        xm, ym = X[tr].mean(axis=0), Y[tr].mean(axis=0)
        scores = (X[te] - xm) @ fit['x_weights']                     # (n_te, k)
        Q = fit['y_loadings']                                        # (T, k)
        n_test[s] = te.sum()
        sse[:, 0, s] = np.sum((Y[te] - ym) ** 2, axis=0)
        for c in range(1, k + 1):
            pred = ym + scores[:, :c] @ Q[:, :c].T
            with np.errstate(divide='ignore', invalid='ignore'):
                r[:, c - 1, s] = ref.efficient_corr(Y[te], pred)
                r2[:, c - 1, s] = ref.r2_score_raw(Y[te], pred)
            sse[:, c, s] = np.sum((Y[te] - pred) ** 2, axis=0)
    return dict(r=r, r2=r2, sse=sse, mse=sse.sum(axis=0) / n_test[None, :], n_test=n_test)


def rel_err(got, want):
    """max |got - want| / max(1, |want|), elementwise -- the form the tolerance takes on r^2 and mse."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if want.size else 0.0


def abs_err(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want))) if want.size else 0.0
