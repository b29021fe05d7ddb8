"""Expected values of pls_regression(coef_components=c, coef_ci=True), written on the CPU oracle (oracle/cpu_ref.py:
simpls, get_mask): the per-bootstrap coefficient matrices ``coef_expected`` sums, kept, and numpy's percentiles of
them.  Shared by tests/test_regression_coef_ci_host.py, tests/test_gpu_regression_coef_ci.py and
tests/golden/make_coef_ci_golden.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref
from regression_coef_expect import _AGG, beta_of


def coef_boot(X, Y, bootsamples, k, c, aggfunc='mean', third=None):
    """(n, B, T): beta_b of every bootstrap, exactly the matrices whose sums regression_coef_expect.coef_expected
    builds ``coefs_stderr`` from (same rows, same masks, same fit)."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    agg = _AGG.get(aggfunc, aggfunc)
    Y_agg = agg(Y, axis=-1) if Y.ndim == 3 else Y
    Xc = X - np.nanmean(X, axis=0, keepdims=True)
    Yc = Y_agg - np.nanmean(Y_agg, axis=0, keepdims=True)
    out = []
    for i in range(bootsamples.shape[1]):
        inds = bootsamples[:, i]
        Xi = Xc[inds]
        Yi = agg(Y[..., third[:, i]], axis=-1)[inds] if Y.ndim == 3 else Yc[inds]
        m = ref.get_mask(Xi, Yi)
        out.append(beta_of(ref.simpls(Xi[m], Yi[m], k), c))
    return np.stack(out)


def ci_of(boot, ci=95, weights=None):
    """boot (n, B, T) -> (B, T, 2): np.percentile over the bootstraps, [..., 0] lower, [..., 1] upper (numpy's default
    linear interpolation; the original fit is not part of the series).  weights (n,) ints: how often each bootstrap
    counts (the replication trick of the batch-geometry tests): the series is the matrices repeated."""
    boot = np.asarray(boot, dtype=float)
    if weights is not None:
        boot = np.repeat(boot, np.asarray(weights, dtype=int), axis=0)
    low = (100 - ci) / 2
    lo, hi = np.percentile(boot, [low, 100 - low], axis=0)
    return np.stack([lo, hi], axis=-1)


def coef_ci_expected(X, Y, bootsamples, k, c, ci=95, aggfunc='mean', third=None, weights=None):
    return ci_of(coef_boot(X, Y, bootsamples, k, c, aggfunc=aggfunc, third=third), ci=ci, weights=weights)


def stack_ci(Xc, stack, ci=95):
    """numpy's answer to plsx_simpls_coef_ci: Xc (S, B) centred, stack (n, T, S) -> (B, T, 2)."""
    boot = np.einsum('sf,nts->nft', Xc, stack, optimize=True)
    return ci_of(boot, ci=ci)
