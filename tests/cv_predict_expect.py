"""Expected out-of-fold predictions (``cv_predict=``), written on the CPU oracle (oracle/cpu_ref.py: simpls, get_mask,
efficient_corr, r2_score_raw) exactly as tests/regression_cv_expect.cv_expected forms its predictions -- which it then
reduces to scores and discards.  Shared by tests/test_cv_predict_host.py and tests/test_gpu_cv_predict*.py; not a test
module."""
import numpy as np

from oracle import cpu_ref as ref


def pred_expected(X, Y, masks, ncomp):
    """X (S, B), Y (S, T), masks (S, n) bool with True = training row, ncomp an int c or (n,) ints, one per split (0: an
    undefined split, all NaN).  Returns y_pred (S, T, n): for a usable test row i of split s
    ``[1, x_i] @ simpls(X_tr, Y_tr, c)['beta']`` = ybar_tr + sum_{j <= c} t_j[i] q_j, NaN on every other row (training
    rows and rows get_mask masks).  In the units of Y."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    masks = np.asarray(masks, dtype=bool)
    S, T, n = len(X), Y.shape[1], masks.shape[1]
    ncomp = np.broadcast_to(np.asarray(ncomp, dtype=int), (n,))
    ok = ref.get_mask(X, Y)
    out = np.full((S, T, n), np.nan)
    for s in range(n):
        c = int(ncomp[s])
        if c == 0:
            continue
        tr, te = masks[:, s] & ok, ~masks[:, s] & ok
        fit = ref.simpls(X[tr], Y[tr], c)
        xm, ym = X[tr].mean(axis=0), Y[tr].mean(axis=0)
        out[te, :, s] = ym + ((X[te] - xm) @ fit['x_weights']) @ fit['y_loadings'].T
    return out


def usable_test_rows(X, Y, masks):
    """(S, n) bool: the usable test rows of every split -- where y_pred is not NaN."""
    return ~np.asarray(masks, dtype=bool) & ref.get_mask(np.asarray(X, dtype=float), np.asarray(Y, dtype=float))[:, None]


def scores_from_pred(y_pred, y_true):
    """The scores the cross-validation reduces its predictions to, recomputed from them: y_pred (S, T, n) with NaN off
    the test rows, y_true (S, T) or (S, T, n) -> dict(r (T, n), r2 (T, n), sse (T, n), n_test (n,), mse (n,)):
    efficient_corr, r2_score_raw and the summed squared error over the test rows of every split."""
    y_pred = np.asarray(y_pred, dtype=float)
    y_true = np.asarray(y_true, dtype=float)
    S, T, n = y_pred.shape
    if y_true.ndim == 2:
        y_true = np.broadcast_to(y_true[:, :, None], y_pred.shape)
    r, r2, sse, n_test = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n)), np.zeros(n, dtype=int)
    for s in range(n):
        te = ~np.isnan(y_pred[:, 0, s])
        y, p = y_true[te, :, s], y_pred[te, :, s]
        n_test[s] = te.sum()
        with np.errstate(divide='ignore', invalid='ignore'):
            r[:, s] = ref.efficient_corr(y, p)
            r2[:, s] = ref.r2_score_raw(y, p)
        sse[:, s] = np.sum((y - p) ** 2, axis=0)
    return dict(r=r, r2=r2, sse=sse, n_test=n_test, mse=sse.sum(axis=0) / n_test)


def da_pred_expected(X, codes, masks, c):
    """pls_da: the predicted RAW indicators (S, G, n) of the c-component model and ``predicted`` (S, n) int32, the first
    maximum on the usable test rows, -1 elsewhere."""
    codes = np.asarray(codes, dtype=int)
    G = int(codes.max()) + 1
    Y = np.zeros((len(codes), G))
    Y[np.arange(len(codes)), codes] = 1.0
    y_pred = pred_expected(X, Y, masks, c)
    te = ~np.isnan(y_pred[:, 0, :])
    predicted = np.where(te, np.argmax(np.where(np.isnan(y_pred), -np.inf, y_pred), axis=1), -1).astype(np.int32)
    return y_pred, predicted


def confusion_from_predicted(predicted, codes, G):
    """(G, G, n) int64 [true, predicted, split] recounted from ``predicted`` (S, n) (-1: not a test row)."""
    predicted, codes = np.asarray(predicted), np.asarray(codes, dtype=int)
    n = predicted.shape[1]
    conf = np.zeros((G, G, n), dtype=np.int64)
    for s in range(n):
        te = predicted[:, s] >= 0
        np.add.at(conf[:, :, s], (codes[te], predicted[te, s]), 1)
    return conf


def auc_mann_whitney(v, positive):
    """u2 / (2 pairs) of scores v against positive (bool): Mann-Whitney with ties one half, from integer counts."""
    v, positive = np.asarray(v, dtype=float), np.asarray(positive, dtype=bool)
    a, b = v[positive][:, None], v[~positive][None, :]
    u2 = 2 * int((a > b).sum()) + int((a == b).sum())
    pairs = int(positive.sum()) * int((~positive).sum())
    return u2 / (2.0 * pairs) if pairs else np.nan


def trapezoid(fpr, tpr):
    fpr, tpr = np.asarray(fpr, dtype=float), np.asarray(tpr, dtype=float)
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def rel_err(got, want):
    """max |got - want| / max(1, |want|) over the entries that are not NaN in both; the NaN patterns must agree."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN patterns differ'
    live = ~np.isnan(want)
    return float(np.max(np.abs(got[live] - want[live]) / np.maximum(1.0, np.abs(want[live])))) if live.any() else 0.0


def behav_pred_expected(spec, X, Y, masks):
    """behavioral_pls: y_pred (S, T, n), the prediction tests/crossval_expect.single forms and reduces to r / r2 -- for a
    test row of cell j ``zmap(x; training rows of cell j) @ U_live @ V_live[jT:(j+1)T].T + mean_train_j(Y)`` -- NaN on
    the training rows.  ``masks`` (S, n) bool, True = training row."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    masks = np.asarray(masks, dtype=bool)
    T, n = Y.shape[1], masks.shape[1]
    dummy = spec.dummy.astype(bool)
    out = np.full((len(X), T, n), np.nan)
    for s in range(n):
        mask = masks[:, s]
        R = ref.gen_covcorr(spec, X[mask], Y[mask], dummy[mask])
        _, d, V = ref.svd(R)
        d = np.diag(d).copy()
        live = d > ref.RANK_RTOL * d.max()
        V_live = V[:, live]
        U_live = R.T @ V_live / d[live]
        for j in range(dummy.shape[1]):
            tr, te = dummy[:, j] & mask, dummy[:, j] & ~mask
            if not te.any():
                continue
            mu, sd = X[tr].mean(axis=0), X[tr].std(axis=0, ddof=1)
            out[te, :, s] = ((X[te] - mu) / sd) @ U_live @ V_live[j * T:(j + 1) * T].T + Y[tr].mean(axis=0, keepdims=True)
    return out


def behav_fold_expected(spec, X, Y, Z, masks):
    """behavioral_pls(confounds=Z): per split the fold residuals X_s, Y_s (tests/confound_expect.residualise fitted on
    the training rows, applied to every row) -> (y_pred, y_true), both (S, T, n) with NaN on the training rows."""
    from confound_expect import residualise
    masks = np.asarray(masks, dtype=bool)
    n = masks.shape[1]
    y_pred = np.full((len(X), np.asarray(Y).shape[1], n), np.nan)
    y_true = np.full(y_pred.shape, np.nan)
    for s in range(n):
        tr = masks[:, s]
        Xs, Ys = residualise(X, Z, tr), residualise(Y, Z, tr)
        y_pred[:, :, s] = behav_pred_expected(spec, Xs, Ys, masks[:, s:s + 1])[:, :, 0]
        y_true[~tr, :, s] = Ys[~tr]
    return y_pred, y_true
