"""Expected values of pls_da's cross-validated classification, written on the CPU oracle (oracle/cpu_ref.py: simpls,
get_mask) exactly as tests/regression_cv_expect.cv_expected forms its predictions.  Shared by
tests/test_discriminant_host.py, tests/test_gpu_discriminant.py and tests/golden/make_da_golden.py; not a test module.

The comparison these values serve is EXACT integer equality of confusion counts.  What keeps that honest is the
``margin``: the smallest gap between the two largest predicted indicators over every (split, c, counted row).  The
device's predictions agree with the oracle's to about 1e-10, so a margin of at least MARGIN = 1e-6 means no argmax can
differ; every test that compares counts asserts it for its own input."""
import numpy as np

from oracle import cpu_ref as ref

MARGIN = 1e-6


def one_hot(codes, G=None):
    codes = np.asarray(codes, dtype=int)
    G = int(codes.max()) + 1 if G is None else int(G)
    Y = np.zeros((len(codes), G))
    Y[np.arange(len(codes)), codes] = 1.0
    return Y


def da_expected(X, codes, masks, k, perm=None):
    """X (S, B), codes (S,) int class codes 0 .. G - 1, masks (S, n) bool with True = training row, perm (S,) a
    permutation of the rows of Y or None.  Returns dict(confusion (G, G, k, n) int64 -- [true, predicted, c - 1, split]
    over the usable test rows -- and margin).  Under ``perm`` the fit runs on (X, Y[perm]), the true class of position p
    is codes[perm[p]] and usability is get_mask(X, Y[perm]).  A row whose predictions contain a NaN is counted
    nowhere."""
    X, codes = np.asarray(X, dtype=float), np.asarray(codes, dtype=int)
    masks = np.asarray(masks, dtype=bool)
    G = int(codes.max()) + 1
    true = codes if perm is None else codes[np.asarray(perm)]
    Y = one_hot(true, G)
    ok = ref.get_mask(X, Y)
    n = masks.shape[1]
    conf = np.zeros((G, G, k, n), dtype=np.int64)
    margin = np.inf
    for s in range(n):
        tr, te = masks[:, s] & ok, ~masks[:, s] & ok
        fit = ref.simpls(X[tr], Y[tr], k)
        xm, ym = X[tr].mean(axis=0), Y[tr].mean(axis=0)
        scores = (X[te] - xm) @ fit['x_weights']                     # (n_te, k)
        Q = fit['y_loadings']                                        # (G, k)
        for c in range(1, k + 1):
            pred = ym + scores[:, :c] @ Q[:, :c].T
            counted = ~np.isnan(pred).any(axis=1)
            pred, t = pred[counted], true[te][counted]
            np.add.at(conf[:, :, c - 1, s], (t, np.argmax(pred, axis=1)), 1)
            if len(pred):
                top = np.sort(pred, axis=1)[:, -2:]
                margin = min(margin, float(np.min(top[:, 1] - top[:, 0])))
    return dict(confusion=conf, margin=margin)


def da_perm_expected(X, codes, masks, k, perms):
    """perms (S, P): per permutation the confusion summed over the splits, (G, G, k, P), and the smallest margin."""
    out = [da_expected(X, codes, masks, k, perm=perms[:, p]) for p in range(perms.shape[1])]
    return dict(confusion=np.stack([o['confusion'].sum(axis=-1) for o in out], axis=-1),
                margin=min(o['margin'] for o in out))


def stratified_expected(codes, sorted_masks):
    """The masks ``gen_splits(counts, 1, n, ...)`` drew on the rows in class-sorted order (sorted_masks (S, n)), scattered
    back to the caller's row order: row i of the result is the row of sorted_masks at the rank of i in a stable sort of
    the codes."""
    codes = np.asarray(codes)
    rank = np.empty(len(codes), dtype=int)
    pos = 0
    for g in np.unique(codes):
        for i in np.flatnonzero(codes == g):                          # ascending row order within a class: stable
            rank[i] = pos
            pos += 1
    return np.asarray(sorted_masks)[rank]
