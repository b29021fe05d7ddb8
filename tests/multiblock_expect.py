"""
Multiblock PLS in numpy, on the hooks of oracle.cpu_ref: the definition the device is tested against
(tests/test_multiblock_host.py, tests/test_gpu_multiblock.py).  pyls has no multiblock method; the definition follows
the Matlab PLS toolbox's method 4 in structure and is this project's own.

With G groups, C conditions, J = G C cells, T behaviours, ``sm`` the mean-centred Spec and ``sb`` the behavioural one
(same groups, n_cond, covariance, mean_centering):

  R_task  = gen_covcorr(sm, X_t, dummy, dummy)          (J, B)    cell means minus the reference mean
  R_behav = gen_covcorr(sb, X_b, Y_b, dummy)            (J T, B)  per-cell xcorr
  R_mb    = vstack([rownorm(R_task), rownorm(R_behav)]) T' = J + J T rows; rownorm(R)[t] = R[t] / ||R[t]|| (0 stays 0)

  original      svd(R_mb) with the oracle's svd_flip; y_scores from the behaviour rows of y_weights, cell by cell;
                y_loadings = the two gen_distrib outputs stacked, NOT normalised
  permutation   one index array pi: X_t = X[pi] in the task block, (X, Y[pi]) in the behaviour block; the statistic of
                single_perm (Procrustes of y_weights, or the plain singular values)
  bootstrap     X[inds], Y[inds] in both blocks; procrustes_live against x_weights, sums and squares; the behavioural
                convention (the original is added back, n = n_boot + 1); the stacked gen_distrib
"""
import numpy as np

from oracle import cpu_ref as ref


def specs_of(groups, n_cond=1, covariance=False, mean_centering=0, rotate=True):
    """-> (sm, sb): the mean-centred and the behavioural Spec of one design."""
    sm = ref.Spec('meancentered', list(groups), n_cond, covariance, mean_centering, rotate)
    sb = ref.Spec('behavioral', list(groups), n_cond, covariance, mean_centering, rotate)
    return sm, sb


def rownorm(R):
    return ref.normalize(R, axis=1)


def blocks(specs, X_t, X_b, Y_b):
    """The two blocks before normalisation: (J, B), (J T, B)."""
    sm, sb = specs
    return ref.gen_covcorr(sm, X_t, sm.dummy, sm.dummy), ref.gen_covcorr(sb, X_b, Y_b, sb.dummy)


def R_mb(specs, X, Y, perminds=None, bootinds=None):
    """The stacked, row-normalised cross-covariance matrix (T', B) of the identity, a permutation or a bootstrap."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    if perminds is not None:
        X_t, X_b, Y_b = X[perminds], X, Y[perminds]
    elif bootinds is not None:
        X_t, X_b, Y_b = X[bootinds], X[bootinds], Y[bootinds]
    else:
        X_t, X_b, Y_b = X, X, Y
    Rt, Rb = blocks(specs, X_t, X_b, Y_b)
    return np.vstack([rownorm(Rt), rownorm(Rb)])


def distrib(specs, X, Y, x_weights):
    """gen_distrib of both blocks stacked (T', L), not normalised: cell means of the mean-centred scores, then the
    per-cell xcorr of Y with the scores."""
    sm, sb = specs
    return np.vstack([ref.gen_distrib(sm, X, sm.dummy, x_weights, sm.dummy),
                      ref.gen_distrib(sb, X, Y, x_weights, sb.dummy)])


def original(specs, X, Y):
    """-> x_weights (B, L), singvals (L,), y_weights (T', L) with the oracle's sign rule."""
    U, d, V = ref.svd(R_mb(specs, X, Y))
    return U, np.diag(d).copy(), V


def perm_singvals(specs, X, Y, y_weights, permsamples, rotate=True):
    """(L, P): the statistic of single_perm on the stacked matrix."""
    out = []
    for i in range(permsamples.shape[1]):
        _, d, V = ref.svd(R_mb(specs, X, Y, perminds=permsamples[:, i]))
        if rotate:
            out.append(np.sqrt(np.sum(ref.procrustes(y_weights, V, d) ** 2, axis=0)))
        else:
            out.append(np.diag(d).copy())
    return np.stack(out, axis=-1)


def boot_sums(specs, X, Y, x_weights, singvals, bootsamples):
    """-> sum of U_b (B, L), sum of U_b^2, distrib (T', L, R): single_boot on the stacked matrix."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    u_sum, u_sq = np.zeros_like(x_weights), np.zeros_like(x_weights)
    live_o = ref.live_lvs(np.asarray(singvals))
    dist = []
    for i in range(bootsamples.shape[1]):
        inds = bootsamples[:, i]
        U, d, _ = ref.svd(R_mb(specs, X, Y, bootinds=inds))
        Ub = ref.procrustes_live(x_weights, U, d, live_o, ref.live_lvs(d))
        u_sum += Ub
        u_sq += Ub ** 2
        dist.append(distrib(specs, X[inds], Y[inds], x_weights))
    return u_sum, u_sq, np.stack(dist, axis=-1)


def closest_tie(singvals, perm_singval):
    """min |s_p - s| / s over the live LVs: exact p-value counts are a fair demand above ~1e-6."""
    s = np.asarray(singvals)[:, None]
    live = s[:, 0] > ref.RANK_RTOL * s.max()
    return float(np.min(np.abs(perm_singval[live] - s[live]) / s[live])) if perm_singval.size else np.inf


def run_multiblock(X, Y, *, groups=None, n_cond=1, covariance=False, mean_centering=0, rotate=True, ci=95,
                   permsamples=None, bootsamples=None):
    """The analysis with caller-supplied resampling arrays: a nested dict in the PLSResults key layout (the counterpart
    of oracle.cpu_ref.run_plsc)."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    if groups is None:
        groups = [len(X) // n_cond]
    specs = specs_of(groups, n_cond, covariance, mean_centering, rotate)
    sb = specs[1]
    J = sb.dummy.shape[1]
    res = dict(permres={}, bootres={})
    U, sv, V = original(specs, X, Y)
    res.update(x_weights=U, y_weights=V, singvals=sv, x_scores=X @ U, varexp=sv ** 2 / (sv ** 2).sum())
    cells = np.repeat(sb.groups, sb.n_cond)
    edges = np.cumsum(cells)[:-1]
    res['y_scores'] = np.vstack([y @ v for y, v in zip(np.split(Y, edges), np.split(V[J:], len(cells)))])
    res['y_loadings'] = distrib(specs, X, Y, U)
    if permsamples is not None:
        d_perm = perm_singvals(specs, X, Y, V, permsamples, rotate)
        res['permres'] = dict(perm_singval=d_perm, pvals=ref.perm_sig(np.diag(sv), d_perm),
                              counts=np.sum(d_perm > sv[:, None], axis=1), permsamples=permsamples)
    if bootsamples is not None:
        R = bootsamples.shape[1]
        u_sum, u_sq, dist = boot_sums(specs, X, Y, U, sv, bootsamples)
        res['u_sum'], res['u_sq'] = u_sum, u_sq
        bs = U * sv
        bsr, se = ref.boot_rel(bs, u_sum + bs, u_sq + bs ** 2, R + 1)
        res['bootres'] = dict(x_weights_normed=bsr, x_weights_stderr=se, y_loadings=res['y_loadings'].copy(),
                              y_loadings_boot=dist, y_loadings_ci=np.stack(ref.boot_ci(dist, ci=ci), -1),
                              bootsamples=bootsamples)
    return res
