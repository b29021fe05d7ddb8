"""pls_regression split-half reliability (``n_split``): what can be checked without a GPU -- the fixtures against the
oracle-based expectation, the dual-space identities the device relies on against the direct feature-space form, the C
ABI declaration and host-side validation (raised before any engine exists)."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import cpu_ref as ref
from regression_split_expect import split_expected, split_null, pvals_of, corr_err

TAGS = ['a', 'nan', 'y3d']


def _agg(Y):
    return Y if Y.ndim == 2 else np.mean(Y, axis=-1)


@pytest.mark.parametrize('tag', TAGS)
def test_oracle_helper_reproduces_the_reference_fixture(tag):
    g = load_golden('simpls_split_' + tag)
    k, Y = int(g['n_components']), _agg(g['Y'])
    uc, vc = split_expected(g['X'], Y, g['splitsamples'], k)
    puc, pvc = split_null(g['X'], Y, g['perm_splitsamples'], g['permsamples'], k)
    assert corr_err(uc, g['ref_ucorr']) <= 1e-10 and corr_err(vc, g['ref_vcorr']) <= 1e-10
    assert corr_err(puc, g['ref_perm_ucorr']) <= 1e-10 and corr_err(pvc, g['ref_perm_vcorr']) <= 1e-10
    # the pinned means and p-values follow from the pinned per-split values; no permuted mean is near the observed one
    assert np.array_equal(g['ref_ucorr_mean'], g['ref_ucorr'].mean(axis=-1))
    assert np.array_equal(g['ref_perm_vcorr_mean'], g['ref_perm_vcorr'].mean(axis=-1).T)
    assert np.array_equal(g['ref_ucorr_pvals'], pvals_of(g['ref_ucorr_mean'], g['ref_perm_ucorr_mean']))
    assert np.array_equal(g['ref_vcorr_pvals'], pvals_of(g['ref_vcorr_mean'], g['ref_perm_vcorr_mean']))
    assert np.abs(g['ref_perm_ucorr_mean'] - g['ref_ucorr_mean'][:, None]).min() > 1e-6
    assert np.abs(g['ref_perm_vcorr_mean'] - g['ref_vcorr_mean'][:, None]).min() > 1e-6


def test_fixture_designs():
    g = {t: load_golden('simpls_split_' + t) for t in TAGS}
    assert g['a']['X'].shape == (90, 400) and g['a']['Y'].shape == (90, 7) and int(g['a']['n_components']) == 6
    assert g['nan']['X'].shape == (80, 200) and g['nan']['Y'].shape == (80, 5)
    assert g['y3d']['X'].shape == (60, 150) and g['y3d']['Y'].shape == (60, 4, 3)
    for t in TAGS:
        S, P = g[t]['permsamples'].shape
        assert 6 <= P <= 8 and g[t]['splitsamples'].shape == (S, 5) and g[t]['perm_splitsamples'].shape == (P, S, 5)
    n = g['nan']
    assert int(np.isnan(n['X']).all(axis=1).sum()) == 3 and int(np.isnan(n['Y']).all(axis=1).sum()) == 2
    # a permutation that moves the masked rows of Y: the usable rows differ from the observed arrangement's
    bad_y = np.flatnonzero(np.isnan(n['Y']).all(axis=1))
    assert any(set(np.flatnonzero(np.isin(n['permsamples'][:, p], bad_y))) != set(bad_y) for p in range(7))


def dual_split(X, Y, masks, k, perm=None):
    """What the device computes, in numpy: nothing B-long but K = Xc Xc^T and r = Xc 1_B of the bound data (Xc centred
    over whatever rows the binding centres it over -- here all that are not NaN; the half means make it irrelevant)."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    if perm is not None:
        Y = Y[perm]
    ok = ref.get_mask(X, Y)
    Xc = np.nan_to_num(X - np.nanmean(X, axis=0))
    K, r, B = Xc @ Xc.T, Xc.sum(axis=1), X.shape[1]
    fit = ref.simpls(X[ok], Y[ok], k)
    t = np.zeros((len(X), k))
    t[ok] = fit['x_scores'] + 3.0                       # (the solver's scores carry a constant: it must drop out)
    Y0 = np.zeros_like(Y)
    Y0[ok] = Y[ok] - Y[ok].mean(axis=0)
    Q = Y0.T @ t                                        # = y_loadings: Y0 sums to zero
    yq = Y0 @ Q                                         # (S, k)
    n = masks.shape[1]
    uc, vc = np.zeros((k, n)), np.zeros((k, n))
    for s in range(n):
        h = [masks[:, s] & ok, ~masks[:, s] & ok]
        for c in range(k):
            g = [np.where(m, yq[:, c] - yq[m, c].mean(), 0.0) for m in h]
            kg = [K @ v for v in g]
            rr = [v @ r for v in g]
            v11, v22 = g[0] @ kg[0] - rr[0] ** 2 / B, g[1] @ kg[1] - rr[1] ** 2 / B
            uc[c, s] = (g[0] @ kg[1] - rr[0] * rr[1] / B) / np.sqrt(v11 * v22)
            d = [Y0[m].T @ (t[m, c] - t[m, c].mean()) for m in h]
            d = [v - v.mean() for v in d]
            with np.errstate(divide='ignore', invalid='ignore'):
                vc[c, s] = (d[0] @ d[1]) / np.sqrt((d[0] @ d[0]) * (d[1] @ d[1]))
    return uc, vc


@pytest.mark.parametrize('S,B,T,k,nan', [(61, 130, 5, 6, False), (90, 33, 3, 4, True), (40, 400, 1, 1, False)])
def test_dual_identities_against_the_direct_form(S, B, T, k, nan):
    """g1^T K g2 - (g1^T r)(g2^T r) / B and the T-vectors from the scores against D_h^T Q and D_h W in feature space, on
    a design whose rows share a common mode of 50 sigma over the features.  The rank-one term is then about
    1 + 50^2 = 2501 times the variance it is subtracted from: 2501 eps times the growth of an S-long dot product, about
    1e-11; the bound leaves two digits.  Measured: at most 4.5e-11 over the three designs."""
    rs = np.random.RandomState(S + B)
    X = rs.randn(S, B) + 50.0 * rs.randn(S, 1)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    perm = rs.permutation(S)
    if nan:
        X[[3, 17]] = np.nan
        Y[[5, 40, 41]] = np.nan
    masks = np.stack([rs.permutation(S) < (S + s) // 2 for s in range(4)], axis=1)
    for p in (None, perm):
        want = split_expected(X, Y, masks, k, perm=p)
        got = dual_split(X, Y, masks, k, perm=p)
        assert corr_err(got[0], want[0]) <= 1e-9 and corr_err(got[1], want[1]) <= 1e-9
    if T == 1:
        assert np.isnan(want[1]).all() and not np.isnan(want[0]).any()


def test_header_declares_and_a_unit_defines_the_entry():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+plsx_simpls_split_half_batch\s*\(\s*plsx_ctx\s*\*', header)
    defined = False
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            if re.search(r'\bint\s+plsx_simpls_split_half_batch\s*\([^;{]*\)\s*try\s*\{', f.read(), re.S):
                defined = True
    assert defined


def _data(S=40, B=30, T=3, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    return X, rs.randn(S, T) + 0.5 * X[:, :T], rs


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


@pytest.mark.parametrize('bad', [-1, 2.5, True, 'many'])
def test_bad_n_split_raises(no_engine, bad):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r'`n_split` must be a non-negative integer'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, n_split=bad, verbose=False)


def test_hook_shapes_raise(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r'`_splitsamples` must have shape \(S, n_split\) = \(40, 4\)'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, n_split=4, verbose=False,
                           _splitsamples=np.ones((40, 5), dtype=bool))
    with pytest.raises(ValueError, match=r'`_perm_splitsamples` must have shape \(n_perm, S, n_split\) = \(6, 40, 4\)'):
        pls.pls_regression(X, Y, n_components=3, n_perm=6, n_boot=0, n_split=4, verbose=False,
                           _perm_splitsamples=np.ones((6, 4, 40), dtype=bool))


def test_half_with_one_usable_row_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    masks = np.zeros((40, 3), dtype=bool)
    masks[:20] = True
    masks[:, 2] = False
    masks[[7, 8], 2] = True                                # a first half of two rows ...
    Xn = X.copy()
    Xn[8] = np.nan                                         # ... of which one is NaN throughout
    with pytest.raises(ValueError, match=r'at least 2 usable rows; split 2 leaves 1 \(1 of 40 rows'):
        pls.pls_regression(Xn, Y, n_components=3, n_perm=0, n_boot=0, n_split=3, _splitsamples=masks, verbose=False)


def test_drawn_halves_count_masked_rows_before_any_engine(no_engine):
    """Drawn masks keep floor(S / 2) rows at least in a half; the rows that are NaN throughout may all fall into it --
    under a permutation those of X and those of Y."""
    import pypyls_amd as pls
    rs = np.random.RandomState(3)
    X, Y = rs.randn(8, 5), rs.randn(8, 2)
    X[[0, 1]] = np.nan
    Y[1] = np.nan                                          # observed: 2 unusable rows; permuted: up to 3
    with pytest.raises(ValueError, match=r'at least 2 usable rows; a split can leave 1 of 8 \(3 rows'):
        pls.pls_regression(X, Y, n_components=1, n_perm=4, n_boot=0, n_split=3, verbose=False)
    X[2] = np.nan
    with pytest.raises(ValueError, match=r'at least 2 usable rows; a split can leave 1 of 8 \(3 rows'):
        pls.pls_regression(X, Y, n_components=1, n_perm=0, n_boot=0, n_split=3, verbose=False)


def test_splitres_keys():
    from pypyls_amd.structures import PLSResults
    keys = ('ucorr', 'vcorr', 'ucorr_pvals', 'vcorr_pvals', 'ucorr_lolim', 'ucorr_uplim', 'vcorr_lolim', 'vcorr_uplim')
    res = PLSResults(splitres=dict({key: np.zeros(3) for key in keys}, bogus=1))
    assert set(res.splitres.keys()) == set(keys)
