"""behavioral_pls(cv_perm=P), the permutation null of the behavioural cross-validation: what can be checked without a
GPU -- a numpy restatement of the device's dual form (one S x S matrix per split, csrc/plsx_k_cvperm.h) against the
definition of tests/behavioral_cv_perm_expect.py on every case of the GPU test, the conditioning its tolerance rests
on, the p-value rule, validation before any engine exists, the C ABI declaration and the built library."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import cpu_ref as ref
import crossval_expect as cx
import behavioral_cv_perm_expect as px

ENTRY = 'plsx_crossval_perm_batch'


def dual_single(spec, X, Y, mask):
    """One (permutation, split) fit as the device forms it -> r, r2, kappa of the live spectrum.

        xc_i = x_i - mu_c(i);  z_i = xc_i / sigma_c(i)   (training moments of the cell, 1 / sigma := 0 when constant)
        M[i][t] = a_i xc_i . b_t xc_t:  correlation a = b = 1 / sigma; covariance b = 1, a = 1 (training i), 1 / sigma (test i)
        W' = A M^T;  G = W' A^T -> V, d;  pred(test p of cell j) = W'[:, p]^T V_live / d_live V_live[jT:(j+1)T]^T + ybar_j
    """
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    mask = np.asarray(mask, dtype=bool)
    S, T = Y.shape
    dummy = spec.dummy.astype(bool)
    J = dummy.shape[1]
    const = px.cell_constant(spec, X, mask)
    Xc, Z = np.zeros_like(X), np.zeros_like(X)
    A = np.zeros((J * T, S))
    ybar = np.zeros((J, T))
    for j in range(J):
        tr = dummy[:, j] & mask
        mu = X[tr].mean(axis=0)
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = np.where(const[j], 0.0, 1.0 / X[tr].std(axis=0, ddof=1))
        inv[const[j]] = 0.0
        Xc[dummy[:, j]] = X[dummy[:, j]] - mu
        Z[dummy[:, j]] = Xc[dummy[:, j]] * inv
        Yt = Y[tr]
        Yc = Yt - Yt.mean(axis=0)
        if not spec.covariance:
            Yc = Yc / Yt.std(axis=0, ddof=1)
        A[j * T:(j + 1) * T][:, tr] = Yc.T / (tr.sum() - 1)
        ybar[j] = Yt.mean(axis=0)
    if spec.covariance:
        rows = np.where(mask[:, None], Xc, Z)
        M = rows @ Xc.T
    else:
        M = Z @ Z.T
    W = A @ M.T
    G = W @ A.T
    lam, V = np.linalg.eigh((G + G.T) / 2)
    order = np.argsort(lam)[::-1][:min(J * T, X.shape[1])]
    d, V = np.sqrt(np.maximum(lam[order], 0.0)), V[:, order]
    live = d > ref.RANK_RTOL * d.max()
    Vl, dl = V[:, live], d[live]
    pred = np.full(Y.shape, np.nan)
    for j in range(J):
        te = dummy[:, j] & ~mask
        if te.any():
            pred[te] = (W[:, te].T @ Vl / dl) @ Vl[j * T:(j + 1) * T].T + ybar[j]
    return (ref.efficient_corr(Y[~mask], pred[~mask]), ref.r2_score_raw(Y[~mask], pred[~mask]),
            float(dl.max() / dl.min()))


@pytest.mark.parametrize('name', px.CASES)
def test_dual_form_agrees_with_the_definition(name):
    spec, X, Y, masks, perms = px.problem(name)
    _, _, want_r, want_r2, info = px.expected(name)
    P, n = perms.shape[1], masks.shape[1]
    assert 3 <= P <= 6 and 1 <= n <= px.MAX_SPLITS
    r, r2 = np.empty_like(want_r), np.empty_like(want_r2)
    kappa = 0.0
    for p in range(P):
        for s in range(n):
            r[:, p, s], r2[:, p, s], k = dual_single(spec, X, Y[perms[:, p]], masks[:, s])
            kappa = max(kappa, k)
    cx.assert_entrywise(r, r2, want_r, want_r2, what=name + ' dual form')
    # the condition the device tolerance rests on (crossval_expect.TOL: eps * kappa^2), of the definition's own fits
    kmax = max(i['kappa'] for i in info)
    print('{}: {} permutations x {} splits, largest kappa {:.1f} (dual form {:.1f})'.format(name, P, n, kmax, kappa))
    assert kmax <= cx.KAPPA_MAX and kappa <= cx.KAPPA_MAX
    assert np.isfinite(want_r).all() and np.isfinite(want_r2).all()
    if cx.CASES[name]['deficient']:
        assert all(i['n_live'] < i['L'] for i in info)


def test_identity_permutation_is_the_observed_cross_validation():
    spec, X, Y, masks, _ = px.problem('E2')
    ident = np.arange(len(X))[:, None]
    r, r2, _ = px.null(spec, X, Y, ident, masks)
    want_r, want_r2, _ = cx.expected('E2')
    assert np.array_equal(r[:, 0], want_r[:, :masks.shape[1]]) and np.array_equal(r2[:, 0], want_r2[:, :masks.shape[1]])


@pytest.mark.parametrize('name', ['E2', 'E4'])
def test_cell_constant_feature_has_scale_zero(name):
    """A feature made bit-constant in one training cell of one split (where the reference's arithmetic divides by a
    zero, or by the 1e-17 a rounded mean leaves): the definition stays finite and the dual form follows it."""
    spec, X, Y, masks, perms = px.problem(name)
    mask = masks[:, 0]
    cell = spec.dummy[:, 1].astype(bool)
    Xk = X.copy()
    Xk[cell & mask, 3] = Xk[cell & mask, 3][0]
    assert px.cell_constant(spec, Xk, mask)[1, 3] and px.cell_constant(spec, Xk, mask).sum() == 1
    assert not px.cell_constant(spec, Xk, masks[:, 1]).any() or masks.shape[1] < 2
    Yp = Y[perms[:, 0]]
    r, r2, _ = px.single(spec, Xk, Yp, mask)
    assert np.isfinite(r).all() and np.isfinite(r2).all()
    dr, dr2, _ = dual_single(spec, Xk, Yp, mask)
    cx.assert_entrywise(dr, dr2, r, r2, what=name + ' cell-constant, dual form')


def test_split_mean_and_pvalues_follow_the_rule():
    a = np.array([[[1.0, 2.0, 3.0], [1.0, np.nan, 3.0]]])          # (T = 1, P = 2, n = 3)
    m = px.split_mean(a)
    assert m[0, 0] == 2.0 and np.isnan(m[0, 1])                    # one NaN score makes the permutation's mean NaN
    observed = np.array([[0.4, 0.6], [0.0, 0.2]])                  # means 0.5, 0.1
    null = np.array([[0.5, 0.6, np.nan, 0.4], [0.1, 0.1, 0.1, np.nan]])
    p = px.pvals(null, observed)
    # a tie is not larger (strict '>'), a NaN compares false
    assert np.array_equal(p, np.array([(1 + 1) / 5, (0 + 1) / 5]))
    from pypyls_amd import hostmath
    with np.errstate(invalid='ignore'):
        assert np.array_equal(hostmath.perm_sig(observed.mean(axis=-1), null), p)


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def _data(S=40, B=30, T=3, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    return X, rs.randn(S, T) + 0.5 * X[:, :T], rs


KW = dict(n_perm=0, n_boot=0, verbose=False)


@pytest.mark.parametrize('bad', [-1, 2.5, True, '3', None])
def test_bad_cv_perm_raises(no_engine, bad):
    import pypyls_amd as pls
    X, Y, _ = _data()
    with pytest.raises(ValueError, match=r'`cv_perm` must be a non-negative integer'):
        pls.behavioral_pls(X, Y, test_split=4, cv_perm=bad, **KW)


def test_cv_perm_without_cross_validation_or_with_contrasts_raises(no_engine):
    import pypyls_amd as pls
    X, Y, _ = _data()
    with pytest.raises(ValueError, match=r'`cv_perm` needs cross-validation'):
        pls.behavioral_pls(X, Y, cv_perm=5, test_split=0, **KW)
    with pytest.raises(ValueError, match=r'`cv_perm` needs cross-validation'):
        pls.behavioral_pls(X, Y, cv_perm=5, test_split=4, test_size=0, **KW)
    with pytest.raises(ValueError, match=r'`cv_perm` is not available with `contrasts`'):
        pls.behavioral_pls(X, Y, cv_perm=5, test_split=4, contrasts=np.eye(3)[:, :2], **KW)


def test_cv_perm_belongs_to_behavioral_pls(no_engine):
    import pypyls_amd as pls
    X, Y, _ = _data()
    with pytest.raises(ValueError, match=r'`cv_perm` .* is not available for mean-centred PLS'):
        pls.meancentered_pls(X, groups=[20, 20], cv_perm=5, **KW)
    with pytest.raises(ValueError, match=r'`cv_perm` .* is not available for multiblock PLS'):
        pls.multiblock_pls(X, Y, groups=[20, 20], cv_perm=5, **KW)


def test_bad_cvpermsamples_raise(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    perms = np.stack([rs.permutation(40) for _ in range(5)], axis=1)
    kw = dict(test_split=4, **KW)
    with pytest.raises(ValueError, match=r'`cvpermsamples` must have shape \(S, cv_perm\) = \(40, 4\)'):
        pls.behavioral_pls(X, Y, cv_perm=4, cvpermsamples=perms, **kw)
    with pytest.raises(ValueError, match=r'`cvpermsamples` must have shape'):
        pls.behavioral_pls(X, Y, cv_perm=5, cvpermsamples=perms[:-1], **kw)
    with pytest.raises(ValueError, match=r'`cvpermsamples` must have shape'):
        pls.behavioral_pls(X, Y, cv_perm=5, cvpermsamples=perms.T, **kw)
    dup = perms.copy()
    dup[0, 2] = dup[1, 2]                                   # a row drawn twice: a bootstrap, not a permutation
    with pytest.raises(ValueError, match=r'one permutation of 0 \.\. 39 per column; column 2 is not one'):
        pls.behavioral_pls(X, Y, cv_perm=5, cvpermsamples=dup, **kw)
    out = perms.copy()
    out[3, 1] = 40
    with pytest.raises(IndexError, match=r'out of bounds'):                  # (engine.check_index_array, as permsamples)
        pls.behavioral_pls(X, Y, cv_perm=5, cvpermsamples=out, **kw)


def test_keys_are_allowed_in_the_records():
    from pypyls_amd.structures import PLSInputs, PLSCrossValidationResults
    assert 'cv_perm' in PLSInputs.allowed
    for key in ('perm_pearson_r', 'perm_r_squared', 'pearson_r_pvals', 'r_squared_pvals', 'cvpermsamples', 'cvsamples'):
        assert key in PLSCrossValidationResults.allowed, key


def test_header_engine_and_library_carry_the_entry():
    from pypyls_amd import engine, _build
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+' + ENTRY + r'\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*d_masks\s*,\s*int\s+n\s*,'
                     r'\s*const\s+int32_t\s*\*\s*d_perm_idx\s*,\s*int\s+m\s*,\s*double\s*\*\s*d_r\s*,\s*double\s*\*\s*d_r2\s*,'
                     r'\s*void\s*\*\s*stream\s*\)', header)
    defined = False
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            if re.search(r'\bint\s+' + ENTRY + r'\s*\([^;{]*\)\s*try\s*\{', f.read(), re.S):
                defined = True
    assert defined, 'the entry is a function-try-block in csrc/'
    assert ENTRY in engine.exported_symbols()
    assert hasattr(engine.Engine, 'crossval_perm')
    _build.build()
    lib = engine._load()
    assert hasattr(lib, ENTRY)
