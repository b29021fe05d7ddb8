"""Expected values of pls_regression(vip_components=c), written on the CPU oracle (oracle/cpu_ref.py: simpls,
get_mask): the VIP scores of a fit (the formula of MATLAB's ``plsregress`` documentation with unit-norm x_scores), of
every bootstrap's fit -- the fits ``regression_coef_ci_expect.coef_boot`` takes its coefficients from --, numpy's
standard deviation and percentiles of them.  Shared by tests/test_regression_vip_host.py,
tests/test_gpu_regression_vip.py and tests/golden/make_vip_golden.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref
from regression_coef_expect import _AGG


def vip_formula(W, Q, c):
    """VIP (B,) from x_weights W (B, >= c) and simpls y_loadings Q (T, >= c).  0 / 0 gives NaN."""
    W, Q = np.asarray(W, dtype=float)[:, :c], np.asarray(Q, dtype=float)[:, :c]
    ssq = (Q ** 2).sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sqrt(W.shape[0] * ((W ** 2 / (W ** 2).sum(axis=0)) @ ssq) / ssq.sum())


def vip_of(fit, c):
    """(B,) VIP of the first c components of an oracle simpls fit (the models are nested)."""
    return vip_formula(fit['x_weights'], fit['y_loadings'], c)


def degenerate(fit, c):
    """True when the formula divides 0 by 0: no explained variance or a component of zero weight norm."""
    W, Q = np.asarray(fit['x_weights'])[:, :c], np.asarray(fit['y_loadings'])[:, :c]
    return bool((Q ** 2).sum() == 0 or np.any((W ** 2).sum(axis=0) == 0))


def _fits(X, Y, bootsamples, k, aggfunc, third, simpls, get_mask):
    """The original fit and one fit per bootstrap: the rows, masks and fit of coef_boot."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    agg = _AGG.get(aggfunc, aggfunc)
    Y_agg = agg(Y, axis=-1) if Y.ndim == 3 else Y
    Xc = X - np.nanmean(X, axis=0, keepdims=True)
    Yc = Y_agg - np.nanmean(Y_agg, axis=0, keepdims=True)
    mask = get_mask(Xc, Yc)
    yield simpls(Xc[mask], Yc[mask], k)
    for i in range(0 if bootsamples is None else bootsamples.shape[1]):
        inds = bootsamples[:, i]
        Xi = Xc[inds]
        Yi = agg(Y[..., third[:, i]], axis=-1)[inds] if Y.ndim == 3 else Yc[inds]
        m = get_mask(Xi, Yi)
        yield simpls(Xi[m], Yi[m], k)


def vip_boot(X, Y, bootsamples, k, c, aggfunc='mean', third=None):
    """(n, B): the VIP scores of every bootstrap's fit (same rows, same masks, same fit as coef_boot)."""
    fits = _fits(X, Y, bootsamples, k, aggfunc, third, ref.simpls, ref.get_mask)
    next(fits)
    return np.stack([vip_of(f, c) for f in fits])


def summary(boot, ci=95, weights=None):
    """boot (n, B) -> stderr (B,), np.std(ddof=1) (NaN for n = 1), and ci (B, 2), np.percentile over the bootstraps
    (numpy's default linear interpolation; the original fit is not part of the series).  weights (n,) ints: how often
    each bootstrap counts (the replication trick of the batch-geometry tests): the series is the rows repeated."""
    boot = np.asarray(boot, dtype=float)
    if weights is not None:
        boot = np.repeat(boot, np.asarray(weights, dtype=int), axis=0)
    low = (100 - ci) / 2
    lo, hi = np.percentile(boot, [low, 100 - low], axis=0)
    with np.errstate(divide='ignore', invalid='ignore'), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        sd = np.std(boot, ddof=1, axis=0)
    return sd, np.stack([lo, hi], axis=-1)


def vip_expected(X, Y, bootsamples, k, c, ci=95, aggfunc='mean', third=None, weights=None):
    """dict(vip, stderr, ci): the original fit's VIP and the summary of the bootstraps'."""
    fits = _fits(X, Y, None, k, aggfunc, third, ref.simpls, ref.get_mask)
    out = dict(vip=vip_of(next(fits), c))
    if bootsamples is not None:
        sd, iv = summary(vip_boot(X, Y, bootsamples, k, c, aggfunc=aggfunc, third=third), ci=ci, weights=weights)
        out.update(stderr=sd, ci=iv)
    return out


def stack_boot(Xc, stack):
    """Xc (S, B) centred, stack (n, c, S) -> (n, B): sqrt(B sum_a (Xc^T G_b[a])^2), the series of plsx_simpls_vip_ci."""
    proj = np.einsum('sf,nas->naf', Xc, stack, optimize=True)
    return np.sqrt(Xc.shape[1] * (proj ** 2).sum(axis=1))


def stack_vip(Xc, stack, ci=95):
    """numpy's answer to plsx_simpls_vip_ci: (stderr (B,), ci (B, 2))."""
    return summary(stack_boot(Xc, stack), ci=ci)
