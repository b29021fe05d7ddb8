"""
Non-rotated PLS (``contrasts=``) in numpy, on the hooks of oracle.cpu_ref: the definition the device is tested
against (tests/test_nonrotated_host.py, tests/test_gpu_nonrotated.py).

With R(.) = gen_covcorr of an arrangement (T' x B, rows in the order of y_weights) and V = normalize(contrasts):
  original      Z = R(X, Y)^T V; singvals[l] = ||Z[:, l]||; x_weights = Z / singvals (0 where the norm is 0);
                y_weights = V (no svd_flip); varexp = singvals^2 / sum
  permutation   perm_singval[l, p] = ||R_p^T V[:, l]|| on make_permutation's arrangement; pvals = perm_sig
  bootstrap     U_b = R_b^T V summed (and squared); orig = x_weights . singvals; behavioural: the original is added
                back and n = n_boot + 1, mean-centred: n = n_boot; gen_distrib with x_weights
"""
import numpy as np

from oracle import cpu_ref as ref


def spec_of(method, groups, n_cond=1, covariance=False, mean_centering=0):
    return ref.Spec(method, list(groups), n_cond, covariance, mean_centering, True)


def original(spec, X, Y, contrasts):
    """-> x_weights (B, Lc), singvals (Lc,), y_weights (T', Lc)."""
    V = ref.normalize(np.asarray(contrasts, dtype=float))
    Z = ref.gen_covcorr(spec, X, Y, spec.dummy).T @ V
    sv = np.sqrt((Z ** 2).sum(axis=0))
    with np.errstate(divide='ignore', invalid='ignore'):
        U = np.where(sv > 0, Z / sv, 0.0)
    return U, sv, V


def perm_singvals(spec, X, Y, V, permsamples=None, ystack=None):
    """(Lc, P): index arrays (S, P), or pre-permuted Y matrices (P, S, T) for behavioural PLS."""
    out = []
    n = permsamples.shape[1] if permsamples is not None else len(ystack)
    for i in range(n):
        if permsamples is not None:
            Xp, Yp = ref.make_permutation(spec, X, Y, permsamples[:, i])
        else:
            Xp, Yp = X, ystack[i]
        Zp = ref.gen_covcorr(spec, Xp, Yp, spec.dummy).T @ V
        out.append(np.sqrt((Zp ** 2).sum(axis=0)))
    return np.stack(out, axis=-1)


def boot_sums(spec, X, Y, V, x_weights, bootsamples):
    """-> sum of U_b (B, Lc), sum of U_b^2, distrib (T', Lc, R)."""
    u_sum = np.zeros((X.shape[1], V.shape[1]))
    u_sq = np.zeros_like(u_sum)
    dist = []
    for i in range(bootsamples.shape[1]):
        inds = bootsamples[:, i]
        Ub = ref.gen_covcorr(spec, X[inds], Y[inds], spec.dummy).T @ V
        u_sum += Ub
        u_sq += Ub ** 2
        dist.append(ref.gen_distrib(spec, X[inds], Y[inds], x_weights, spec.dummy))
    return u_sum, u_sq, np.stack(dist, axis=-1)


def closest_tie(singvals, perm_singval):
    """min |s_p - s| / s over the live contrasts: exact p-value counts are a fair demand above ~1e-6."""
    s = np.asarray(singvals)[:, None]
    live = s[:, 0] > 1e-8 * s.max()
    return float(np.min(np.abs(perm_singval[live] - s[live]) / s[live])) if perm_singval.size else np.inf


def run_nonrotated(X, Y=None, *, contrasts, method='behavioral', groups=None, n_cond=1, covariance=False,
                   mean_centering=0, ci=95, permsamples=None, bootsamples=None, ystack=None):
    """The analysis with caller-supplied resampling arrays: a nested dict in the PLSResults key layout (the
    counterpart of oracle.cpu_ref.run_plsc)."""
    X = np.asarray(X, dtype=float)
    if groups is None:
        groups = [len(X) // n_cond]
    spec = spec_of(method, groups, n_cond, covariance, mean_centering)
    Y = spec.dummy if method == 'meancentered' else np.asarray(Y, dtype=float)
    res = dict(permres={}, bootres={})
    U, sv, V = original(spec, X, Y, contrasts)
    res.update(x_weights=U, y_weights=V, singvals=sv, x_scores=X @ U)
    with np.errstate(divide='ignore', invalid='ignore'):
        res['varexp'] = sv ** 2 / (sv ** 2).sum()
    if permsamples is not None or ystack is not None:
        d_perm = perm_singvals(spec, X, Y, V, permsamples, ystack)
        res['permres'] = dict(perm_singval=d_perm, pvals=ref.perm_sig(np.diag(sv), d_perm),
                              counts=np.sum(d_perm > sv[:, None], axis=1))
    if method == 'behavioral':
        cells = np.repeat(spec.groups, spec.n_cond)
        edges = np.cumsum(cells)[:-1]
        res['y_scores'] = np.vstack([y @ v for y, v in zip(np.split(Y, edges), np.split(V, len(cells)))])
        res['y_loadings'] = ref.gen_covcorr(spec, res['x_scores'], Y, spec.dummy)
    else:
        res['y_scores'] = Y @ V
        bs_dm = ref.get_mean_center(X, Y, n_cond, mean_centering, False) @ U
        contrast = np.vstack([bs_dm[c].mean(axis=0) for c in Y.T.astype(bool)])
    if bootsamples is not None:
        R = bootsamples.shape[1]
        u_sum, u_sq, distrib = boot_sums(spec, X, Y, V, U, bootsamples)
        res['u_sum'], res['u_sq'] = u_sum, u_sq
        bs = U * sv
        ci_arr = np.stack(ref.boot_ci(distrib, ci=ci), -1)
        if method == 'behavioral':
            bsr, se = ref.boot_rel(bs, u_sum + bs, u_sq + bs ** 2, R + 1)
            res['bootres'] = dict(x_weights_normed=bsr, x_weights_stderr=se, y_loadings=res['y_loadings'].copy(),
                                  y_loadings_boot=distrib, y_loadings_ci=ci_arr, bootsamples=bootsamples)
        else:
            bsr, se = ref.boot_rel(bs, u_sum, u_sq, R)
            res['bootres'] = dict(x_weights_normed=bsr, x_weights_stderr=se, contrast=contrast,
                                  contrast_boot=distrib, contrast_ci=ci_arr, bootsamples=bootsamples)
    return res
