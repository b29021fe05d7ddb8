"""
The permutation null of the behavioural cross-validation in numpy, on the hooks of oracle.cpu_ref and
tests/crossval_expect.py: the definition the device path (plsx_crossval_perm_batch, ``behavioral_pls(cv_perm=)``) is
tested against (tests/test_behavioral_cv_perm_host.py, tests/test_gpu_behavioral_cv_perm.py).

For permutation p (an index row over 0 .. S-1) and training mask s

    r[:, p, s], r2[:, p, s] = crossval_expect.single(spec, X, Y[perm_p], mask_s)

(the device's existing convention: live latent variables only, RANK_RTOL), ``perm_pearson_r[:, p]`` is the mean of
``r[:, p, :]`` over the splits, ``perm_r_squared`` the same mean of ``r2``, and

    pearson_r_pvals[t] = (#{p : perm_pearson_r[t, p] > pearson_r[t, :].mean()} + 1) / (P + 1)

(``r_squared_pvals`` likewise) -- the rule of ``pls_regression(cv_perm=)``.  A NaN score of one (permutation, split)
makes that permutation's mean NaN, and a NaN compares false, as in numpy.

Cell-constant features: a feature whose training rows of a cell all hold the same bits has
1/sd := 0 in that cell -- its column of the training cross-correlation is 0 in the cell's rows and the test rows of
the cell rescale to 0 -- where ``crossval_expect.single`` divides by zero.  ``single`` below states that rule and is
``crossval_expect.single`` itself on data without such a feature.
"""
import functools

import numpy as np

from oracle import cpu_ref as ref
import crossval_expect as cx

#: the cases of the GPU test and the edge each one reaches
CASES = ['E1', 'E2', 'E7', 'E3', 'E4', 'E6_65', 'E6_127', 'E5_64', 'E5_65', 'E8', 'E12', 'E13']
#: permutations per case (3 .. 6): fewer where one fit is expensive on the host
N_PERM = {'E1': 4, 'E3': 3, 'E5_64': 3, 'E5_65': 3}
N_PERM_DEFAULT = 6
#: splits per case: the first MAX_SPLITS masks of the case
MAX_SPLITS = 6
PERM_SEED = 5


def cell_constant(spec, X, mask):
    """(J, B) bool: feature b holds one bit pattern in every training row of cell j."""
    X = np.ascontiguousarray(X, dtype=float)
    mask = np.asarray(mask, dtype=bool)
    bits = X.view(np.int64)
    out = np.zeros((spec.dummy.shape[1], X.shape[1]), dtype=bool)
    for j, c in enumerate(spec.dummy.T.astype(bool)):
        rows = bits[c & mask]
        out[j] = (rows == rows[:1]).all(axis=0)
    return out


def _single_scale0(spec, X, Y, mask, const):
    """crossval_expect.single with 1/sd := 0 for the (cell, feature) pairs of ``const``."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    mask = np.asarray(mask, dtype=bool)
    T = Y.shape[1]
    dummy = spec.dummy.astype(bool)
    inv, mu, rows = [], [], []
    for j in range(dummy.shape[1]):
        tr = dummy[:, j] & mask
        Xt, Yt = X[tr], Y[tr]
        with np.errstate(divide='ignore', invalid='ignore'):
            iv = np.where(const[j], 0.0, 1.0 / Xt.std(axis=0, ddof=1))
        iv[const[j]] = 0.0
        Xc, Yc = Xt - Xt.mean(axis=0), Yt - Yt.mean(axis=0)
        if not spec.covariance:
            Xc, Yc = Xc * iv, Yc / Yt.std(axis=0, ddof=1)
        rows.append((Yc.T @ Xc) / (len(Xt) - 1))
        inv.append(iv)
        mu.append(Xt.mean(axis=0))
    R = np.vstack(rows)
    _, d, V = ref.svd(R)
    d = np.diag(d).copy()
    live = d > ref.RANK_RTOL * d.max()
    V_live, d_live = V[:, live], d[live]
    U_live = R.T @ V_live / d_live
    n_live = int(live.sum())
    info = dict(n_live=n_live, L=len(d), kappa=float(d_live.max() / d_live.min()),
                gap=float(d[n_live] / d[0]) if n_live < len(d) else 0.0)
    pred = np.full(Y.shape, np.nan)
    for j in range(dummy.shape[1]):
        tr, te = dummy[:, j] & mask, dummy[:, j] & ~mask
        if not te.any():
            continue
        pred[te] = ((X[te] - mu[j]) * inv[j]) @ U_live @ V_live[j * T:(j + 1) * T].T + Y[tr].mean(axis=0, keepdims=True)
    return ref.efficient_corr(Y[~mask], pred[~mask]), ref.r2_score_raw(Y[~mask], pred[~mask]), info


def single(spec, X, Y, mask):
    """One split -> r (T,), r2 (T,), info: crossval_expect.single, with scale 0 for cell-constant features."""
    const = cell_constant(spec, X, mask)
    if not const.any():
        return cx.single(spec, X, Y, mask)
    return _single_scale0(spec, X, Y, mask, const)


def null(spec, X, Y, perms, masks):
    """perms (S, P) index columns, masks (S, n) -> r, r2 (T, P, n) and the info of every (permutation, split)."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    P, n, T = perms.shape[1], masks.shape[1], Y.shape[1]
    r, r2, info = np.empty((T, P, n)), np.empty((T, P, n)), []
    for p in range(P):
        Yp = Y[perms[:, p]]
        for s in range(n):
            r[:, p, s], r2[:, p, s], i = single(spec, X, Yp, masks[:, s])
            info.append(i)
    return r, r2, info


def split_mean(a):
    """(T, P, n) -> (T, P): the mean over the splits in split order; one NaN makes the mean NaN."""
    out = np.zeros(a.shape[:2])
    for s in range(a.shape[2]):
        out = out + a[:, :, s]
    return out / a.shape[2]


def pvals(perm_mean, observed):
    """perm_mean (T, P), observed (T, n splits) -> (T,): (#{null > observed mean} + 1) / (P + 1); NaN compares false."""
    perm_mean, observed = np.asarray(perm_mean, dtype=float), np.asarray(observed, dtype=float)
    with np.errstate(invalid='ignore'):
        count = np.sum(perm_mean > observed.mean(axis=1)[:, None], axis=1)
    return (count + 1) / (perm_mean.shape[1] + 1)


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> spec, X, Y, masks (S, n <= MAX_SPLITS), perms (S, P) of one case, built once and shared (read-only)."""
    from pypyls_amd import resampling as rsmp
    spec, X, Y, masks = cx.problem(name)
    case = cx.CASES[name]
    masks = np.ascontiguousarray(masks[:, :MAX_SPLITS])
    perms = np.ascontiguousarray(rsmp.gen_permsamp(case['groups'], case['n_cond'], N_PERM.get(name, N_PERM_DEFAULT),
                                                   seed=PERM_SEED, verbose=False))
    masks.setflags(write=False)
    perms.setflags(write=False)
    return spec, X, Y, masks, perms


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> perm_pearson_r (T, P), perm_r_squared (T, P), r, r2 (T, P, n), [info]: computed once per session."""
    spec, X, Y, masks, perms = problem(name)
    r, r2, info = null(spec, X, Y, perms, masks)
    out = (split_mean(r), split_mean(r2), r, r2)
    for a in out:
        a.setflags(write=False)
    return out + (info,)
