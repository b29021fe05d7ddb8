"""
The out-of-sample score correlation of the latent variables in numpy, on the hooks of oracle.cpu_ref,
tests/crossval_expect.py and tests/behavioral_cv_perm_expect.py: the definition the device path
(plsx_crossval_lv_batch, plsx_crossval_perm_lv_batch, ``behavioral_pls(cv_lv=)``) is tested against
(tests/test_behavioral_cv_lv_host.py, tests/test_gpu_behavioral_cv_lv.py).

For one training mask, with R, V, d, live exactly as ``crossval_expect.single`` forms them (``U_live = R^T V_live /
d_live``) and test row p in cell j:

    x_score[p, l] = zmap(x_p; mean, std(ddof=1) of the training rows of cell j) . U_live[:, l]
                    (the z the prediction uses; in covariance mode too, as rescale_test does; 1/sd := 0 for a
                    cell-constant feature, the rule of behavioral_cv_perm_expect)
    y_score[p, l] = yt_p . V[jT:(j+1)T, l],   yt_p = y_p - training mean of cell j, in correlation mode also divided by
                    the training std (ddof=1) of cell j -- the normalisation R itself was built with
    lv_corr[l]    = Pearson r of x_score[:, l] and y_score[:, l] over ALL test rows of the split in row order, clamped
                    to [-1, 1]; NaN for a latent variable that is not live; NaN (0 / 0) where a side has no variance

Both scores flip with the sign of column l of V: no alignment.  LV l of a fit is its l-th largest singular value, also
under a permutation.  Under ``cv_perm`` ``perm_lv_corr[l, p]`` is the mean over the splits, in split order, of lv_corr of
(X, Y[perm_p]) (one NaN makes it NaN) and

    lv_corr_pvals[l] = (#{p : perm_lv_corr[l, p] > lv_corr[l, :].mean()} + 1) / (P + 1)

where a NaN null value compares false and a NaN observed mean gives NaN.

A single latent variable, unlike the prediction, needs a gap between singular values, and the device solves on the Gram
side: every value comes with ``relgap_l = min(d2_{l-1} - d2_l, d2_l - d2_{l+1}) / d2_1`` (d2 = d squared; a missing
neighbour is left out, except that with T' > B the T' x T' Gram matrix has zero eigenvalues below d2_L).  Measured on the
host (eigh of R R^T against the oracle SVD, every case below): |delta lv_corr| * relgap <= 8.1e-15.  ``compare`` states
the rule of the tests: a live entry is compared iff relgap >= RELGAP_MIN, within TOL * max(1, RELGAP_FULL / relgap)
absolute; at most CAP of the live entries of a case may be left out and never LV 0 (``check_cap``).
"""
import functools

import numpy as np

from oracle import cpu_ref as ref
import crossval_expect as cx
import behavioral_cv_perm_expect as bcp

RELGAP_MIN = 1e-6
RELGAP_FULL = 1e-4
CAP = 0.02


def decomposition(spec, X, Y, mask):
    """-> R (T', B), V (T', L), d (L,), live (L,) as crossval_expect.single forms them, and mu, inv [(B,)] per cell: the
    training mean and 1 / std (ddof=1) of the features (0 for a cell-constant feature; then R is built with that
    scale, as behavioral_cv_perm_expect does)."""
    dummy = spec.dummy.astype(bool)
    const = bcp.cell_constant(spec, X, mask)
    mu, inv, rows = [], [], []
    for j in range(dummy.shape[1]):
        Xt, Yt = X[dummy[:, j] & mask], Y[dummy[:, j] & mask]
        with np.errstate(divide='ignore', invalid='ignore'):
            iv = np.where(const[j], 0.0, 1.0 / Xt.std(axis=0, ddof=1))
        mu.append(Xt.mean(axis=0))
        inv.append(iv)
        if const.any():
            Xc, Yc = Xt - Xt.mean(axis=0), Yt - Yt.mean(axis=0)
            if not spec.covariance:
                Xc, Yc = Xc * iv, Yc / Yt.std(axis=0, ddof=1)
            rows.append((Yc.T @ Xc) / (len(Xt) - 1))
    R = np.vstack(rows) if const.any() else ref.gen_covcorr(spec, X[mask], Y[mask], dummy[mask])
    _, d, V = ref.svd(R)
    d = np.diag(d).copy()
    return R, V, d, d > ref.RANK_RTOL * d.max(), mu, inv


def relgap_of(d, Tp):
    """(L,) relative gap of every squared singular value to its neighbours (module docstring)."""
    d2 = np.asarray(d, dtype=float) ** 2
    if Tp > len(d2):
        d2 = np.append(d2, 0.0)                  # the Gram matrix's zero eigenvalues
    up = np.append(np.inf, d2[:-1] - d2[1:])
    down = np.append(d2[:-1] - d2[1:], np.inf)
    return (np.minimum(up, down) / d2[0])[:len(d)]


def pearson(x, y):
    """Pearson r of two vectors, clamped to [-1, 1]; NaN (0 / 0) where a side has no variance."""
    xc, yc = x - x.mean(), y - y.mean()
    with np.errstate(invalid='ignore', divide='ignore'):
        r = (xc * yc).sum() / np.sqrt((xc * xc).sum() * (yc * yc).sum())
    return r if np.isnan(r) else float(np.clip(r, -1.0, 1.0))


def scores(spec, X, Y, mask, V=None):
    """One split -> x_score, y_score (n_test, L) in row order (NaN columns for the LVs that are not live), and the
    decomposition they rest on (R, V, d, live).  ``V``: a replacement for the V of the training SVD (same d, live)."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    mask = np.asarray(mask, dtype=bool)
    T = Y.shape[1]
    dummy = spec.dummy.astype(bool)
    R, V0, d, live, mu, inv = decomposition(spec, X, Y, mask)
    V = V0 if V is None else V
    U = np.full((X.shape[1], len(d)), np.nan)
    U[:, live] = R.T @ V[:, live] / d[live]
    xs, ys = np.full((len(X), len(d)), np.nan), np.full((len(X), len(d)), np.nan)
    for j in range(dummy.shape[1]):
        tr, te = dummy[:, j] & mask, dummy[:, j] & ~mask
        if not te.any():
            continue
        xs[te] = ((X[te] - mu[j]) * inv[j]) @ U
        yt = Y[te] - Y[tr].mean(axis=0)
        if not spec.covariance:
            yt = yt / Y[tr].std(axis=0, ddof=1)
        ys[te] = yt @ V[j * T:(j + 1) * T]
        ys[np.ix_(te, ~live)] = np.nan
    return xs[~mask], ys[~mask], dict(R=R, V=V, d=d, live=live)


def single(spec, X, Y, mask, V=None):
    """One split -> lv_corr (L,), relgap (L,), live (L,)."""
    xs, ys, dec = scores(spec, X, Y, mask, V=V)
    live = dec['live']
    lv = np.full(len(live), np.nan)
    for l in np.flatnonzero(live):
        lv[l] = pearson(xs[:, l], ys[:, l])
    return lv, relgap_of(dec['d'], dec['R'].shape[0]), live


def crossval_lv(spec, X, Y, masks):
    """masks (S, n) -> lv_corr, relgap (L, n), live (L, n) bool."""
    out = [single(spec, X, Y, masks[:, i]) for i in range(masks.shape[1])]
    return tuple(np.stack([o[k] for o in out], -1) for k in range(3))


def null(spec, X, Y, perms, masks):
    """perms (S, P) index columns, masks (S, n) -> lv_corr, relgap, live (L, P, n) of (X, Y[perm_p]) under mask s."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    out = [crossval_lv(spec, X, Y[perms[:, p]], masks) for p in range(perms.shape[1])]
    return tuple(np.stack([o[k] for o in out], 1) for k in range(3))


def split_mean(a):
    """(L, P, n) -> (L, P): the mean over the splits in split order; one NaN makes the mean NaN."""
    return bcp.split_mean(a)


def pvals(perm_mean, observed):
    """perm_mean (L, P), observed (L, n splits) -> (L,): (#{null > observed mean} + 1) / (P + 1); a NaN null value
    compares false, a NaN observed mean gives NaN."""
    perm_mean, observed = np.asarray(perm_mean, dtype=float), np.asarray(observed, dtype=float)
    mean = observed.mean(axis=1)
    with np.errstate(invalid='ignore'):
        count = np.sum(perm_mean > mean[:, None], axis=1)
    return np.where(np.isnan(mean), np.nan, (count + 1) / (perm_mean.shape[1] + 1))


def tolerance(relgap):
    """Per entry: crossval_expect.TOL * max(1, RELGAP_FULL / relgap)."""
    with np.errstate(divide='ignore'):
        return cx.TOL * np.maximum(1.0, RELGAP_FULL / np.asarray(relgap, dtype=float))


def check_cap(relgap, live, what=''):
    """The condition on the EXPECTATION, asserted before the device is looked at: at most CAP of the live entries
    (LV axis first) have relgap < RELGAP_MIN, and never LV 0.  -> the number left out."""
    out = live & (relgap < RELGAP_MIN)
    n_out, n_live = int(out.sum()), int(live.sum())
    assert not out[0].any(), '{}: LV 0 would be left out of the comparison'.format(what)
    assert n_out <= CAP * n_live, '{}: {} of {} live entries have no gap: more than {:g}'.format(what, n_out, n_live, CAP)
    return n_out


def compare(got, want, relgap, live, what=''):
    """Every entry of ``got`` against the expectation: NaN exactly where the LV is not live, a live entry with
    relgap >= RELGAP_MIN within ``tolerance`` (absolute); prints and returns the largest error over its tolerance."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape == relgap.shape == live.shape, (got.shape, want.shape, relgap.shape, live.shape)
    check_cap(relgap, live, what)
    assert np.all(np.isnan(got[~live])), '{}: a latent variable that is not live has a value'.format(what)
    assert np.all(np.isfinite(want[live])), '{}: the expectation has a NaN in a live entry'.format(what)
    use = live & (relgap >= RELGAP_MIN)
    err = np.abs(got[use] - want[use])
    err[~np.isfinite(got[use])] = np.inf
    ratio = err / tolerance(relgap[use])
    worst = float(ratio.max()) if ratio.size else 0.0
    print('{}: {} entries, {} left out, max |d lv_corr| {:.2e}, max error / tolerance {:.2e}'
          .format(what, int(use.sum()), int((live & ~use).sum()), float(err.max()) if err.size else 0.0, worst))
    assert worst <= 1.0, '{}: lv_corr off by {:.3g} x its tolerance in one entry'.format(what, worst)
    return worst


def compare_mean(got, want_pairs, relgap, live, what=''):
    """Split means (L, P) against pairs (L, P, n): a mean is compared iff all its splits pass the gap rule, with the
    loosest tolerance among them; it is NaN where a split's LV is not live."""
    got = np.asarray(got, dtype=float)
    all_live = live.all(axis=-1)
    assert np.all(np.isnan(got[~all_live])), '{}: the mean over a NaN split has a value'.format(what)
    use = all_live & (relgap >= RELGAP_MIN).all(axis=-1)
    tol = tolerance(relgap).max(axis=-1)
    want = split_mean(want_pairs)
    err = np.abs(got[use] - want[use])
    err[~np.isfinite(got[use])] = np.inf
    worst = float((err / tol[use]).max()) if err.size else 0.0
    print('{}: {} means, max error / tolerance {:.2e}'.format(what, int(use.sum()), worst))
    assert worst <= 1.0, '{}: a split mean of lv_corr is off by {:.3g} x its tolerance'.format(what, worst)
    return worst


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> lv_corr, relgap, live (L, m) of a case of crossval_expect.CASES: computed once per session (read-only)."""
    spec, X, Y, masks = cx.problem(name)
    out = crossval_lv(spec, X, Y, masks)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def null_expected(name):
    """-> lv_corr, relgap, live (L, P, n) on the problem of behavioral_cv_perm_expect (its masks and permutations)."""
    spec, X, Y, masks, perms = bcp.problem(name)
    out = null(spec, X, Y, perms, masks)
    for a in out:
        a.setflags(write=False)
    return out
