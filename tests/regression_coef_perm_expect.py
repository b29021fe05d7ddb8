"""Expected values of pls_regression(coef_components=c, coef_perm=True), written on the CPU oracle (oracle/cpu_ref.py:
simpls, get_mask): the coefficients of the c-component model of every permutation, their exceedance counts, the maxima
of the standardised coefficients and both p-value arrays.  Shared by tests/test_regression_coef_perm_host.py,
tests/test_gpu_regression_coef_perm.py and tests/golden/make_coef_perm_golden.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref
from regression_coef_expect import _AGG, beta_of


def centred(X, Y, aggfunc='mean'):
    """(Xc, Yc): what pls_regression fits -- nan-mean centred X and aggregated Y."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    agg = _AGG.get(aggfunc, aggfunc)
    Y_agg = agg(Y, axis=-1) if Y.ndim == 3 else Y
    return X - np.nanmean(X, axis=0, keepdims=True), Y_agg - np.nanmean(Y_agg, axis=0, keepdims=True)


def feature_scale(Xc):
    """s_f (B,): sqrt(sum_s Xc[s, f]^2 / (n_x - 1)) over the n_x usable rows of X (rows that are not NaN throughout)."""
    okx = ~np.isnan(Xc).all(axis=1)
    return np.sqrt(np.sum(Xc[okx] ** 2, axis=0) / (okx.sum() - 1))


def coef_perms(Xc, Yc, permsamples, k, c):
    """(n_perm, B, T): beta of the c-component model fitted on (Xc, Yc[perm]) -- get_mask on the permuted pair."""
    out = []
    for i in range(permsamples.shape[1]):
        Yp = Yc[permsamples[:, i]]
        m = ref.get_mask(Xc, Yp)
        out.append(beta_of(ref.simpls(Xc[m], Yp[m], k), c))
    return np.stack(out)


def pvals_of(obs, perms, scale):
    """obs (B, T), perms (n, B, T), scale (B,) -> dict(count, coefs_pvals, coefs_max, coefs_pvals_fwe) exactly as
    pls_regression defines them: >= in both counts, the maximum over standardised magnitudes."""
    n = perms.shape[0]
    count = (np.abs(perms) >= np.abs(obs)[None]).sum(axis=0)
    std = scale[None, :, None] * np.abs(perms)
    cmax = np.ascontiguousarray(std.max(axis=1).T)                       # (T, n)
    sobs = scale[:, None] * np.abs(obs)
    fwe_count = (cmax.T[:, None, :] >= sobs[None]).sum(axis=0)            # (B, T)
    return dict(count=count, coefs_pvals=(count + 1) / (n + 1), coefs_max=cmax,
                coefs_pvals_fwe=(fwe_count + 1) / (n + 1))


def coef_perm_expected(X, Y, permsamples, k, c, aggfunc='mean'):
    Xc, Yc = centred(X, Y, aggfunc)
    m = ref.get_mask(Xc, Yc)
    obs = beta_of(ref.simpls(Xc[m], Yc[m], k), c)
    perms = coef_perms(Xc, Yc, permsamples, k, c)
    out = pvals_of(obs, perms, feature_scale(Xc))
    out.update(coefs=obs, perms=perms)
    return out


def min_rel_gap(obs, perms):
    """The smallest | |b_p| - |b| | / |b| over all (f, t, p) with b != 0: how far the counts are from a tie."""
    a = np.abs(obs)
    nz = a > 0
    return float((np.abs(np.abs(perms) - a[None])[:, nz] / a[nz][None]).min())


def stack_test(Xc, stack, obs, standardise):
    """numpy's answer to plsx_simpls_coef_perm_test: Xc (S, B) centred (no NaN), stack (n, T, S), obs (B, T) ->
    (count (B, T) int, max (n, T))."""
    coef = np.einsum('sf,nts->nft', Xc, stack, optimize=True)
    s = np.sqrt(np.sum(Xc ** 2, axis=0) / (Xc.shape[0] - 1)) if standardise else np.ones(Xc.shape[1])
    v = s[None, :, None] * np.abs(coef)
    count = (v >= (s[:, None] * np.abs(obs))[None]).sum(axis=0)
    return count, v.max(axis=1)
