"""Expected values of pls_regression(coef_components=c), written on the CPU oracle (oracle/cpu_ref.py: simpls,
get_mask, boot_rel).  Shared by tests/test_regression_coef_host.py, tests/test_gpu_regression_coef.py and
tests/golden/make_coef_golden.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref

_AGG = dict(mean=np.mean, median=np.median, sum=np.sum)
MAX_RATIO = 1e3          # the inputs must keep the oracle's own |coefs_normed| below this ...
MIN_SE_REL = 1e-8        # ... and every coefs_stderr above this fraction of the largest: boot_rel's variance
#                          sum b^2 - (sum b)^2 / n cancels where a coefficient hardly moves, in the oracle too


def beta_of(fit, c):
    """(B, T) coefficients of the first c components of an oracle simpls fit."""
    return fit['x_weights'][:, :c] @ fit['y_loadings'][:, :c].T


def coef_expected(X, Y, bootsamples, k, c, aggfunc='mean', third=None, weights=None):
    """X (S, B), Y (S, T) or (S, T, C), bootsamples (S, n) (3-D Y: with ``third`` (C, n), the resampled third axis).
    weights (n,): how often each bootstrap counts (the replication trick of the batch-geometry tests).  Returns
    dict(coefs, intercept, bsum, bsq, stderr, normed, n): per bootstrap ``simpls(Xi[mask], Yi[mask], k)``, beta from
    its x_weights / y_loadings, plain sums, ``ref.boot_rel`` with the original added back (n = n_boot + 1)."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    agg = _AGG.get(aggfunc, aggfunc)
    Y_agg = agg(Y, axis=-1) if Y.ndim == 3 else Y
    Xc = X - np.nanmean(X, axis=0, keepdims=True)
    Yc = Y_agg - np.nanmean(Y_agg, axis=0, keepdims=True)
    mask = ref.get_mask(Xc, Yc)
    coefs = beta_of(ref.simpls(Xc[mask], Yc[mask], k), c)
    out = dict(coefs=coefs, intercept=Y_agg[mask].mean(axis=0) - X[mask].mean(axis=0) @ coefs)
    if bootsamples is None:
        return out
    n = bootsamples.shape[1]
    weights = np.ones(n) if weights is None else np.asarray(weights, dtype=float)
    bsum, bsq = np.zeros_like(coefs), np.zeros_like(coefs)
    for i in range(n):
        # what the reference bootstraps: the centred X, the centred Y for 2-D input, the ORIGINAL Y aggregated over
        # the resampled third axis for 3-D input (regression.py:308-310, 395-397, 408)
        inds = bootsamples[:, i]
        Xi = Xc[inds]
        Yi = agg(Y[..., third[:, i]], axis=-1)[inds] if Y.ndim == 3 else Yc[inds]
        m = ref.get_mask(Xi, Yi)
        b = beta_of(ref.simpls(Xi[m], Yi[m], k), c)
        bsum += weights[i] * b
        bsq += weights[i] * b ** 2
    ntot = int(round(weights.sum()))
    normed, se = ref.boot_rel(coefs, bsum + coefs, bsq + coefs ** 2, ntot + 1)
    assert np.max(np.abs(normed)) < MAX_RATIO, 'inputs outside the tested range: max |coefs_normed| = {:.3g}'.format(
        np.max(np.abs(normed)))
    assert se.min() >= MIN_SE_REL * se.max(), 'inputs outside the tested range: min / max coefs_stderr = {:.3g}'.format(
        se.min() / se.max())
    out.update(bsum=bsum, bsq=bsq, stderr=se, normed=normed, n=ntot)
    return out


def packed_bootsamples(subj, third):
    """The (2, n_boot) object array pls_regression takes for 3-D Y."""
    n = subj.shape[1]
    packed = np.empty((2, n), dtype=object)
    for i in range(n):
        packed[0, i], packed[1, i] = subj[:, i], third[:, i]
    return packed


def max_rel(got, want):
    """max |got - want| / max |want|: the figure conftest.assert_close bounds."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
