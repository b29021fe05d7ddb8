"""Expected values of pls_regression's nested cross-validation of n_components (inner_split=), written on the CPU
oracle (oracle/cpu_ref.py: simpls, efficient_corr, r2_score_raw, get_mask) in the style of tests/regression_cv_expect.py.
Shared by tests/test_regression_nested_host.py and tests/test_gpu_regression_nested.py; not a test module.

Codes: 1 = training row, 0 = test row, 2 = on neither side.  ``codes`` (S, n, 1 + ni): ``[:, s, 0]`` is outer split s
(1 / 0 only), ``[:, s, 1:]`` its inner folds (2 on every outer test row)."""
import numpy as np

from oracle import cpu_ref as ref


def fit_scores(X, Y, code, k):
    """One fit of the list: SIMPLS with k components on the usable rows of code 1, scored on the usable rows of code 0.
    -> r, r2 (T, k), sse (T, k + 1), n_test.  Rows masked by get_mask(X, Y) are on neither side."""
    ok = ref.get_mask(X, Y)
    tr, te = (code == 1) & ok, (code == 0) & ok
    T = Y.shape[1]
    fit = ref.simpls(X[tr], Y[tr], k)
    xm, ym = X[tr].mean(axis=0), Y[tr].mean(axis=0)
    scores = (X[te] - xm) @ fit['x_weights']
    Q = fit['y_loadings']
    r, r2, sse = np.zeros((T, k)), np.zeros((T, k)), np.zeros((T, k + 1))
    sse[:, 0] = np.sum((Y[te] - ym) ** 2, axis=0)
    for c in range(1, k + 1):
        pred = ym + scores[:, :c] @ Q[:, :c].T
        with np.errstate(divide='ignore', invalid='ignore'):
            r[:, c - 1] = ref.efficient_corr(Y[te], pred)
            r2[:, c - 1] = ref.r2_score_raw(Y[te], pred)
        sse[:, c] = np.sum((Y[te] - pred) ** 2, axis=0)
    return r, r2, sse, int(te.sum())


def fit_mse(sse, n_test):
    """sum_t sse[c][t] / n_test, t ascending: (k + 1,)."""
    out = np.zeros(sse.shape[1])
    for t in range(sse.shape[0]):
        out = out + sse[t]
    with np.errstate(divide='ignore', invalid='ignore'):
        return out / n_test


def select(inner_mse):
    """The selection rule on inner_mse (k + 1,): the first minimum over c = 1 .. k, a NaN is never smaller, c = 0 is not
    a candidate; 0 where the minimum is not finite."""
    best = 1
    for c in range(2, len(inner_mse)):
        if inner_mse[c] < inner_mse[best]:
            best = c
    return best if np.isfinite(inner_mse[best]) else 0


def nested_expected(X, Y, codes, k, perm=None):
    """One arrangement (X, Y) or (X, Y[perm]).  -> dict(inner_mse (k + 1, n), ncomp (n,) int, r, r2 (T, n), mse (n,))."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    if perm is not None:
        Y = Y[np.asarray(perm)]
    codes = np.asarray(codes)
    n, ni, T = codes.shape[1], codes.shape[2] - 1, Y.shape[1]
    inner_mse, ncomp = np.zeros((k + 1, n)), np.zeros(n, dtype=np.int64)
    r, r2, mse = np.full((T, n), np.nan), np.full((T, n), np.nan), np.full(n, np.nan)
    for s in range(n):
        acc = np.zeros(k + 1)
        for j in range(1, ni + 1):                                   # (the inner folds in ascending order)
            _, _, sse, nte = fit_scores(X, Y, codes[:, s, j], k)
            acc = acc + fit_mse(sse, nte)
        inner_mse[:, s] = acc / ni
        ncomp[s] = c = select(inner_mse[:, s])
        if c:
            fr, fr2, sse, nte = fit_scores(X, Y, codes[:, s, 0], k)
            r[:, s], r2[:, s], mse[s] = fr[:, c - 1], fr2[:, c - 1], fit_mse(sse, nte)[c]
    return dict(inner_mse=inner_mse, ncomp=ncomp, r=r, r2=r2, mse=mse)


def split_mean(v):
    """The plain mean over the outer splits (last axis), in split order."""
    v = np.asarray(v, dtype=float)
    acc = np.zeros(v.shape[:-1])
    for s in range(v.shape[-1]):
        acc = acc + v[..., s]
    return acc / v.shape[-1]


def nested_perm_expected(X, Y, codes, k, perms):
    """perms (S, P).  -> dict(r, r2 (T, P), mse (P,), ncomp (k, P) int, inner_mse (k + 1, n, P)): the null statistic of a
    permutation is the plain mean over the outer splits, each split at the c selected INSIDE that permutation; ncomp
    counts how many outer splits chose c (an undefined group counts nowhere)."""
    perms = np.asarray(perms)
    P, T, n = perms.shape[1], np.asarray(Y).shape[1], np.asarray(codes).shape[1]
    r, r2, mse = np.zeros((T, P)), np.zeros((T, P)), np.zeros(P)
    cnt, inner = np.zeros((k, P), dtype=np.int64), np.zeros((k + 1, n, P))
    for p in range(P):
        e = nested_expected(X, Y, codes, k, perm=perms[:, p])
        r[:, p], r2[:, p], mse[p] = split_mean(e['r']), split_mean(e['r2']), split_mean(e['mse'])
        inner[:, :, p] = e['inner_mse']
        for c in e['ncomp']:
            if c:
                cnt[c - 1, p] += 1
    return dict(r=r, r2=r2, mse=mse, ncomp=cnt, inner_mse=inner)


def pvals(obs, null, smaller=False):
    """(#{null > obs} + 1) / (P + 1) over the last axis of null (smaller: #{null < obs}); a NaN counts as neither."""
    obs, null = np.asarray(obs, dtype=float), np.asarray(null, dtype=float)
    with np.errstate(invalid='ignore'):
        hits = (null < obs[..., None]) if smaller else (null > obs[..., None])
    return (hits.sum(axis=-1) + 1) / (null.shape[-1] + 1)


def selection_gap(*inner_mses):
    """The smallest value, over all groups of a design including its permutations, of
    (runner-up - best) / max(1, best) over inner_mse[1 .. k].  Arguments: arrays (k + 1, n) or (k + 1, n, P)."""
    gap = np.inf
    for im in inner_mses:
        im = np.asarray(im, dtype=float)
        im = im.reshape(im.shape[0], -1)[1:]
        for g in range(im.shape[1]):
            v = np.sort(im[:, g])
            if len(v) > 1:
                gap = min(gap, (v[1] - v[0]) / max(1.0, v[0]))
    return float(gap)


def design(S, B, T, seed, sig):
    """randn X, Y = randn + sig X[:, :T] + 0.3 X[:, T:2T]."""
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + sig * X[:, :T] + 0.3 * X[:, T:2 * T]
    return X, Y


def rel_err(got, want):
    """max |got - want| / max(1, |want|), elementwise -- the form the tolerance takes on r^2, mse and inner_mse."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if want.size else 0.0


def abs_err(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want))) if want.size else 0.0
