"""pls_regression(confounds=Z): what can be checked without a GPU -- the algebra the device path rests on, the
host-side refusals (raised before any engine exists), the arithmetic of predict and the C ABI declarations."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from confound_expect import cv_expected_confound, cv_expected_global, design, residualise

ENTRIES = ['plsx_simpls_set_confounds', 'plsx_simpls_crossval_confound_batch',
           'plsx_simpls_crossval_confound_perm_batch']


def _design(S=60, B=40, T=3, q=2, n=4, seed=0):
    rs = np.random.RandomState(seed)
    Z = rs.randn(S, q)
    X = rs.randn(S, B) + Z @ rs.randn(q, B) * 2.0
    Y = rs.randn(S, T) + Z @ rs.randn(q, T) * 2.0 + 0.3 * X[:, :T]
    masks = np.ones((S, n), dtype=bool)
    for s in range(n):
        masks[rs.choice(S, S // 4, replace=False), s] = False
    return X, Y, Z, masks, rs


def _fold_ops(Zt, tr):
    """P_s = (Zt' D Zt)^-1 Zt' D and M_s = I - Zt P_s for the training indicator tr."""
    D = np.diag(tr.astype(float))
    P = np.linalg.solve(Zt.T @ D @ Zt, Zt.T @ D)
    return P, np.eye(len(Zt)) - Zt @ P


def test_fold_residuals_of_raw_and_of_residualised_data_agree():
    # identity 1: M_s Zt = 0, hence M_s M = M_s
    X, Y, Z, masks, _ = _design()
    S = len(X)
    allr = np.ones(S, dtype=bool)
    Zt = np.c_[np.ones(S), Z - Z.mean(axis=0)]
    _, M = _fold_ops(Zt, allr)
    Xr, Yr = residualise(X, Z, allr), residualise(Y, Z, allr)
    assert np.abs(M @ X - Xr).max() <= 1e-10 * np.abs(X).max()
    for s in range(masks.shape[1]):
        P, Ms = _fold_ops(Zt, masks[:, s])
        assert np.abs(Ms @ Zt).max() <= 1e-12
        assert np.abs(Ms @ M - Ms).max() <= 1e-12
        assert np.abs(residualise(X, Z, masks[:, s]) - residualise(Xr, Z, masks[:, s])).max() <= 1e-10 * np.abs(X).max()
        assert np.abs(residualise(Y, Z, masks[:, s]) - Ms @ Yr).max() <= 1e-10 * np.abs(Y).max()


def test_rank_update_of_K_and_zero_training_means():
    # identities 2 and 3: K_s = K_r - Zt F' - F Zt', and the training rows of M_s X have zero means
    X, Y, Z, masks, _ = _design()
    S = len(X)
    Zt = np.c_[np.ones(S), Z - Z.mean(axis=0)]
    Xr = residualise(X, Z, np.ones(S, dtype=bool))
    K = Xr @ Xr.T
    for s in range(masks.shape[1]):
        tr = masks[:, s]
        P, Ms = _fold_ops(Zt, tr)
        C = K @ P.T
        E = P @ C
        F = C - 0.5 * Zt @ E
        Ks = K - Zt @ F.T - F @ Zt.T
        Xs = residualise(X, Z, tr)
        assert np.abs(Ks - Xs @ Xs.T).max() <= 1e-12 * np.abs(K).max()
        assert np.abs(Xs[tr].mean(axis=0)).max() <= 1e-12 * np.abs(X).max()
        assert np.abs(residualise(Y, Z, tr)[tr].mean(axis=0)).max() <= 1e-12 * np.abs(Y).max()


def test_freedman_lane_collapses_under_the_fold_regression():
    # identity 4: M_s ((I - M) Y + Y_r[perm]) = M_s (Y_r[perm])
    X, Y, Z, masks, rs = _design()
    S = len(X)
    Zt = np.c_[np.ones(S), Z - Z.mean(axis=0)]
    _, M = _fold_ops(Zt, np.ones(S, dtype=bool))
    Yr = M @ Y
    perm = rs.permutation(S)
    for s in range(masks.shape[1]):
        _, Ms = _fold_ops(Zt, masks[:, s])
        assert np.abs(Ms @ ((np.eye(S) - M) @ Y + Yr[perm]) - Ms @ Yr[perm]).max() <= 1e-11 * np.abs(Y).max()


def test_fold_identity_holds_with_masked_rows():
    # M_s M = M_s over the usable rows: Zt is zero on the masked rows, D never selects them
    X, Y, Z, masks, _ = _design()
    S = len(X)
    ok = np.ones(S, dtype=bool)
    ok[[3, 17, 40]] = False
    Zt = np.where(ok[:, None], np.c_[np.ones(S), Z - Z[ok].mean(axis=0)], 0.0)
    G = np.linalg.solve(Zt.T @ Zt, Zt.T)
    M = np.diag(ok.astype(float)) - Zt @ G
    for s in range(masks.shape[1]):
        tr = masks[:, s] & ok
        P, _ = _fold_ops(Zt, tr)
        Ms = np.diag(ok.astype(float)) - Zt @ P
        assert np.abs(Ms @ M - Ms).max() <= 1e-12
        want = residualise(np.where(ok[:, None], X, 0.0), np.where(ok[:, None], Z, 0.0), tr)[ok]
        assert np.abs((Ms @ (M @ np.where(ok[:, None], X, 0.0)))[ok] - want).max() <= 1e-10 * np.abs(X).max()


def test_foldwise_and_whole_cohort_expectations_differ():
    X, Y, Z, masks, _ = _design(S=130, B=300)
    a, g = cv_expected_confound(X, Y, Z, masks, 3), cv_expected_global(X, Y, Z, masks, 3)
    assert np.abs(a['r'] - g['r']).max() > 1e-3


def test_design_rows():
    Z = np.arange(6.0).reshape(3, 2)
    D = design(Z, rows=[True, False, True])
    assert D.shape == (3, 3) and np.all(D[1] == 0) and np.all(D[:, 0] == [1, 0, 1])


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def _call(X, Y, **kw):
    import pypyls_amd as pls
    kw.setdefault('n_components', 3)
    kw.setdefault('n_perm', 0)
    kw.setdefault('n_boot', 0)
    return pls.pls_regression(X, Y, verbose=False, **kw)


def test_wrong_shape_raises(no_engine):
    X, Y, Z, masks, _ = _design()
    for bad in (Z[:-1], Z[:, :, None], np.zeros((len(X), 0))):
        with pytest.raises(ValueError, match=r'`confounds` must be numeric with shape \(S, q\) or \(S,\)'):
            _call(X, Y, confounds=bad)


def test_too_many_columns_raises(no_engine):
    X, Y, Z, masks, rs = _design()
    with pytest.raises(ValueError, match=r'at most 15 columns; got 16'):
        _call(X, Y, confounds=rs.randn(len(X), 16))


def test_non_finite_on_a_usable_row_raises(no_engine):
    X, Y, Z, masks, _ = _design()
    for bad in (np.inf, np.nan):
        Zb = Z.copy()
        Zb[7, 1] = bad                                     # (row 7 stays usable: it is not NaN throughout)
        with pytest.raises(ValueError, match=r'finite on every usable row.*row 7 is not'):
            _call(X, Y, confounds=Zb)


def test_rank_deficiency_raises(no_engine):
    X, Y, Z, masks, _ = _design()
    with pytest.raises(ValueError, match=r'rank deficient together with the intercept on the 60 usable rows'):
        _call(X, Y, confounds=np.c_[Z, Z[:, 0] - 2.0 * Z[:, 1]])
    with pytest.raises(ValueError, match=r'rank deficient together with the intercept'):
        _call(X, Y, confounds=np.full(len(X), 3.0))        # a constant: collinear with the intercept


def test_rank_deficiency_on_a_split_raises_and_names_it(no_engine):
    X, Y, Z, masks, _ = _design()
    ind = np.zeros(len(X))
    ind[~masks[:, 2]] = 1.0
    ind[np.flatnonzero(masks[:, 2])[0]] = 0.0
    ind[np.flatnonzero(~masks[:, 2])[:3]] = 1.0            # varies over the cohort, constant on the training rows of split 2
    assert np.ptp(ind[masks[:, 2]]) == 0 and np.ptp(ind) > 0
    with pytest.raises(ValueError, match=r'training rows of split 2'):
        _call(X, Y, confounds=np.c_[Z, ind], test_split=4, cvsamples=masks)


def test_3d_y_raises(no_engine):
    X, Y, Z, masks, rs = _design()
    with pytest.raises(ValueError, match=r'`confounds` needs a 2-D Y'):
        _call(X, np.stack([Y, Y + 0.1 * rs.randn(*Y.shape)], axis=-1), confounds=Z)


def test_coef_perm_raises(no_engine):
    X, Y, Z, masks, _ = _design()
    with pytest.raises(ValueError, match=r'`confounds` cannot be combined with `coef_perm=True`'):
        _call(X, Y, confounds=Z, n_perm=5, coef_components=2, coef_perm=True)


def test_cv_perm_with_masked_rows_raises(no_engine):
    X, Y, Z, masks, _ = _design()
    for which in range(3):
        Xn, Yn, Zn = X.copy(), Y.copy(), Z.copy()
        (Xn, Yn, Zn)[which][5] = np.nan
        with pytest.raises(ValueError, match=r'`confounds` with `cv_perm` needs complete data: 1 rows'):
            _call(Xn, Yn, confounds=Zn, test_split=4, cvsamples=masks, cv_perm=3)


def test_pls_da_raises(no_engine):
    import pypyls_amd as pls
    X, Y, Z, masks, rs = _design()
    labels = rs.randint(0, 3, len(X))
    with pytest.raises(ValueError, match=r'`confounds` is not supported by pls_da'):
        pls.pls_da(X, labels, n_components=2, n_perm=0, n_boot=0, verbose=False, confounds=Z)


def test_predict_arithmetic_on_a_hand_built_result():
    import pypyls_amd as pls
    from pypyls_amd.structures import PLSResults
    rs = np.random.RandomState(3)
    S, B, T, q, k = 12, 5, 2, 2, 2
    X, Y, Z = rs.randn(S, B), rs.randn(S, T), rs.randn(S, q)
    W, Q = rs.randn(B, k), rs.randn(T, k)
    gx, gy, zm = rs.randn(q, B), rs.randn(q, T), Z.mean(axis=0)
    res = PLSResults(x_weights=W, y_loadings=Q, x_scores=rs.randn(S, k), confound_mean=zm, confound_x=gx, confound_y=gy,
                     inputs=dict(X=X, Y=Y, n_components=k, confounds=Z))
    X_new, Z_new = rs.randn(4, B), rs.randn(4, q)
    coefs = W @ Q.T
    want = Y.mean(axis=0) - X.mean(axis=0) @ coefs + X_new @ coefs + (Z_new - zm) @ (gy - gx @ coefs)
    got = pls.predict(res, X_new, confounds=Z_new)
    assert np.abs(got - want).max() <= 1e-12
    one = pls.predict(res, X_new, n_components=1, confounds=Z_new)
    c1 = W[:, :1] @ Q[:, :1].T
    assert np.abs(one - (Y.mean(axis=0) - X.mean(axis=0) @ c1 + X_new @ c1 + (Z_new - zm) @ (gy - gx @ c1))).max() <= 1e-12
    with pytest.raises(ValueError, match=r'fitted with confounds: predict needs `confounds=Z_new`'):
        pls.predict(res, X_new)
    with pytest.raises(ValueError, match=r'`confounds` must have shape \(S_new, q\) = \(4, 2\)'):
        pls.predict(res, X_new, confounds=Z_new[:, :1])
    plain = PLSResults(x_weights=W, y_loadings=Q, x_scores=rs.randn(S, k), inputs=dict(X=X, Y=Y, n_components=k))
    with pytest.raises(ValueError, match=r'fitted without confounds: predict takes none'):
        pls.predict(plain, X_new, confounds=Z_new)
    assert np.abs(pls.predict(plain, X_new) - (Y.mean(axis=0) - X.mean(axis=0) @ coefs + X_new @ coefs)).max() <= 1e-12


def test_result_containers_know_the_new_keys():
    from pypyls_amd.structures import PLSInputs, PLSResults
    assert 'confounds' in PLSInputs.allowed
    for key in ('confound_mean', 'confound_x', 'confound_y'):
        assert key in PLSResults.allowed


def test_header_declares_and_a_unit_defines_the_entries():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        eng = f.read()
    sources = []
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            sources.append(f.read())
    for entry in ENTRIES:
        assert re.search(r'\bint\s+' + entry + r'\s*\(\s*plsx_ctx\s*\*', header), entry
        assert any(re.search(r'\bint\s+' + entry + r'\s*\([^;{]*\)\s*try\s*\{', src, re.S) for src in sources), entry
        assert eng.count("'" + entry + "'") >= 2, entry        # the ctypes signature and the required-symbol list
    from pypyls_amd import _build
    assert 'plsx_confound' in _build.UNITS and os.path.exists(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_confound.hip'))
