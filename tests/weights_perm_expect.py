"""Expected values of behavioral_pls / meancentered_pls(weights_perm=m), written on the hooks of the CPU oracle
(oracle/cpu_ref.py: gen_covcorr, make_permutation, decompose): the null Z_p = R_p.T @ V0 of every permutation, the
observed Z = x_weights * singvals, the counts, maxima and both p-values, and how close the nearest comparison comes to a
tie (`closeness`), which every exact comparison of counts asserts first.  Shared by tests/test_weights_perm_host.py and
tests/test_gpu_weights_perm.py; not a test module."""
import numpy as np

from oracle import cpu_ref as ref

#: an exact comparison of counts needs every |Z_p| at least this far, relatively, from the |Z| it is compared with (the
#: rule of the coef_perm fixtures: device and oracle agree to ~1e-12, nine orders inside)
MIN_CLOSENESS = 1e-8


def spec_of(method, groups, n_cond=1, covariance=False, mean_centering=0):
    return ref.Spec(method, groups, n_cond, covariance, mean_centering)


def _y(spec, Y):
    return spec.dummy if spec.method == 'meancentered' else np.asarray(Y, dtype=float)


def observed(spec, X, Y=None, contrasts=None):
    """(Z (B, L), V0 (T', L)) of the original data: Z = x_weights @ diag(singvals), V0 = y_weights -- of the SVD, or,
    with ``contrasts`` (T', Lc), V0 = normalize(contrasts) and Z = R.T @ V0 (whose column norms are the singular values
    of non-rotated PLS and whose normalised columns its x_weights)."""
    X = np.asarray(X, dtype=float)
    if contrasts is not None:
        V = ref.normalize(np.asarray(contrasts, dtype=float))
        return ref.gen_covcorr(spec, X, _y(spec, Y), spec.dummy).T @ V, V
    U, d, V = ref.decompose(spec, X, _y(spec, Y))
    return U @ d, V


def null(spec, X, Y, perms, V0):
    """(B, m, n): Z_p = gen_covcorr(spec, *make_permutation(spec, X, Y, perms[:, p])).T @ V0 of every column of ``perms``
    (S, n); V0 (T', m)."""
    X = np.asarray(X, dtype=float)
    Yh = _y(spec, Y)
    out = []
    for p in range(perms.shape[1]):
        Xp, Yp = ref.make_permutation(spec, X, Yh, np.asarray(perms)[:, p])
        out.append(ref.gen_covcorr(spec, Xp, Yp, spec.dummy).T @ V0)
    return np.stack(out, axis=-1)


def feature_matrix(spec, X):
    """Xf (S, B) with Z_p = W_p @ Xf: the per-cell scaled X (ddof = 1; a feature constant in a cell: 0) in correlation-mode
    behavioral PLS, else the centred X."""
    X = np.asarray(X, dtype=float)
    Xc = X - X.mean(axis=0)
    if spec.method != 'behavioral' or spec.covariance:
        return Xc
    out = np.zeros_like(Xc)
    for c in spec.dummy.T.astype(bool):
        sd = Xc[c].std(axis=0, ddof=1)
        const = (X[c] == X[c][0]).all(axis=0)
        out[c] = Xc[c] * np.where(const | (sd == 0), 0.0, 1.0 / np.where(sd == 0, 1.0, sd))
    return out


def feature_scale(spec, X):
    """q_f (B,) = 1 / s_f: 1 in correlation-mode behavioral PLS; elsewhere s_f is the standard deviation (ddof = 1) of
    feature f over all rows about its grand mean, and q_f = 0 where the feature has no variance."""
    X = np.asarray(X, dtype=float)
    if spec.method == 'behavioral' and not spec.covariance:
        return np.ones(X.shape[1])
    sd = X.std(axis=0, ddof=1)
    flat = (X == X[0]).all(axis=0) | (sd == 0)
    return np.where(flat, 0.0, 1.0 / np.where(flat, 1.0, sd))


def statistics(Z, Zp, q):
    """Z (B, m) observed, Zp (B, m, n) null, q (B,) -> dict(count (B, m) int, max (m, n), pvals, pvals_fwe (B, m),
    closeness): count = #{p : |Zp| >= |Z|}; max = max_f q_f |Zp|; the maxT p-value compares max with q_f |Z|;
    closeness = the minimum over every comparison made of | |left| - |right| | / |right| (0 / 0, a feature without
    variance against itself, is a tie by definition and left out)."""
    Z, Zp, q = np.asarray(Z, dtype=float), np.asarray(Zp, dtype=float), np.asarray(q, dtype=float)
    n = Zp.shape[-1]
    aZ, aZp = np.abs(Z), np.abs(Zp)
    count = (aZp >= aZ[:, :, None]).sum(axis=-1)
    wmax = (q[:, None, None] * aZp).max(axis=0)                                 # (m, n)
    obs = q[:, None] * aZ                                                      # (B, m)
    fwe_count = (wmax[None, :, :] >= obs[:, :, None]).sum(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        c1 = np.abs(aZp - aZ[:, :, None]) / aZ[:, :, None]
        c2 = np.abs(wmax[None, :, :] - obs[:, :, None]) / obs[:, :, None]
    c1, c2 = c1[np.isfinite(c1)], c2[np.isfinite(c2)]
    return dict(count=count, max=wmax, pvals=(count + 1) / (n + 1), pvals_fwe=(fwe_count + 1) / (n + 1),
                closeness=min(float(c1.min()) if c1.size else np.inf, float(c2.min()) if c2.size else np.inf))


def expected(spec, X, Y, perms, m=None, contrasts=None):
    """What the public call adds to permres for the permutations ``perms`` (S, n) -> statistics(...) plus Z and Zp."""
    Z, V = observed(spec, X, Y, contrasts)
    m = Z.shape[1] if m is None else m
    Zp = null(spec, X, Y, perms, V[:, :m])
    out = statistics(Z[:, :m], Zp, feature_scale(spec, X))
    out.update(Z=Z[:, :m], Zp=Zp, V=V[:, :m])
    return out


def random_perms(S, n, rs, identity_at=None):
    """(S, n) permutations of 0 .. S-1, column ``identity_at`` the identity."""
    perms = np.stack([rs.permutation(S) for _ in range(n)], axis=1)
    if identity_at is not None:
        perms[:, identity_at] = np.arange(S)
    return perms
