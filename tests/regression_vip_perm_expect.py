"""Expected values of pls_regression(vip_components=c, vip_perm=True), written on the CPU oracle (oracle/cpu_ref.py:
simpls, get_mask): the VIP scores of the c-component model of every permutation -- the fits
``regression_coef_perm_expect.coef_perms`` takes its coefficients from --, their exceedance counts, the maxima over the
features and both p-value arrays.  Shared by tests/test_regression_vip_perm_host.py,
tests/test_gpu_regression_vip_perm.py and tests/golden/make_vip_perm_golden.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref
from regression_coef_perm_expect import centred
from regression_vip_expect import vip_of


def vip_perms(Xc, Yc, permsamples, k, c, simpls=ref.simpls, get_mask=ref.get_mask):
    """(n_perm, B): VIP of the c-component model fitted on (Xc, Yc[perm]) -- get_mask on the permuted pair."""
    out = []
    for i in range(permsamples.shape[1]):
        Yp = Yc[permsamples[:, i]]
        m = get_mask(Xc, Yp)
        out.append(vip_of(simpls(Xc[m], Yp[m], k), c))
    return np.stack(out)


def pvals_of(obs, perms):
    """obs (B,), perms (n, B) -> dict(count, vip_pvals, vip_max, fwe_count, vip_pvals_fwe) exactly as pls_regression
    defines them: one-sided, >= in both counts, the plain maximum over the features.  A degenerate permuted fit (a row
    of NaN) counts nowhere and has a NaN maximum; where the observed score is NaN both p-values are NaN."""
    obs, perms = np.asarray(obs, dtype=float), np.asarray(perms, dtype=float)
    n = perms.shape[0]
    with np.errstate(invalid='ignore'):
        count = (perms >= obs[None]).sum(axis=0)
        dead = np.isnan(perms).any(axis=1)
        vmax = np.where(dead, np.nan, np.where(np.isnan(perms), -np.inf, perms).max(axis=1))
        fwe_count = (vmax[:, None] >= obs[None]).sum(axis=0)
    nan = np.isnan(obs)
    return dict(count=count, fwe_count=fwe_count, vip_max=vmax,
                vip_pvals=np.where(nan, np.nan, (count + 1) / (n + 1)),
                vip_pvals_fwe=np.where(nan, np.nan, (fwe_count + 1) / (n + 1)))


def vip_perm_expected(X, Y, permsamples, k, c, aggfunc='mean'):
    Xc, Yc = centred(X, Y, aggfunc)
    m = ref.get_mask(Xc, Yc)
    obs = vip_of(ref.simpls(Xc[m], Yc[m], k), c)
    perms = vip_perms(Xc, Yc, permsamples, k, c)
    out = pvals_of(obs, perms)
    out.update(vip=obs, perms=perms)
    return out


def min_rel_gap(obs, perms):
    """(per-feature gap, gap against the maxima): the smallest |vip_p[f] - vip[f]| / vip[f] over all (f, p) and the
    smallest |max_f vip_p - vip[f]| / vip[f] over all (f, p), features with vip > 0: how far the two counts are from
    a tie."""
    obs, perms = np.asarray(obs, dtype=float), np.asarray(perms, dtype=float)
    nz = obs > 0
    own = np.abs(perms[:, nz] - obs[nz][None]) / obs[nz][None]
    top = np.abs(perms.max(axis=1)[:, None] - obs[nz][None]) / obs[nz][None]
    return float(own.min()), float(top.min())


def stack_series(Xc, stack):
    """Xc (S, B) centred, stack (n, c, S) -> (n, B): sqrt(B sum_a (Xc^T G_b[a])^2), the series k_vip_perm_prod tests."""
    proj = np.einsum('sf,nas->naf', Xc, stack, optimize=True)
    return np.sqrt(Xc.shape[1] * (proj ** 2).sum(axis=1))


def stack_test(Xc, stack, obs):
    """numpy's answer to plsx_simpls_vip_perm_test: Xc (S, B) centred (no NaN), stack (n, c, S), obs (B,) ->
    (count (B,) int, max (n,)).  A permutation whose scores are NaN counts nowhere and leaves maximum 0."""
    v = stack_series(Xc, stack)
    with np.errstate(invalid='ignore'):
        count = (v >= np.asarray(obs)[None]).sum(axis=0)
    return count, np.where(np.isnan(v), 0.0, v).max(axis=1)
