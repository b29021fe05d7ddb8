"""pls_regression cross-validation per component count: what can be checked without a GPU -- the fixtures against
the oracle-based expectation, the C ABI declaration, host-side validation (raised before any engine exists) and the
result container."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from regression_cv_expect import cv_expected, abs_err, rel_err

TAGS = ['a', 'b', 'nan']


@pytest.mark.parametrize('tag', TAGS)
def test_oracle_helper_reproduces_the_reference_fixture(tag):
    g = load_golden('simpls_cv_' + tag)
    want = cv_expected(g['X'], g['Y'], g['cvsamples'], int(g['n_components']))
    assert abs_err(want['r'], g['ref_r']) <= 1e-10
    assert rel_err(want['r2'], g['ref_r2']) <= 1e-10
    assert rel_err(want['sse'], g['ref_sse']) <= 1e-10
    assert rel_err(want['mse'], g['ref_mse']) <= 1e-10


def test_fixture_designs():
    shapes = {t: load_golden('simpls_cv_' + t) for t in TAGS}
    assert shapes['a']['X'].shape == (90, 400) and shapes['a']['Y'].shape == (90, 7) and int(shapes['a']['n_components']) == 6
    assert shapes['b']['X'].shape == (60, 150) and shapes['b']['Y'].shape == (60, 3) and int(shapes['b']['n_components']) == 8
    assert shapes['nan']['X'].shape == (80, 200) and shapes['nan']['Y'].shape == (80, 5)
    assert shapes['a']['cvsamples'].shape == (90, 8) and shapes['b']['cvsamples'].shape == (60, 8)
    g = shapes['nan']
    assert int(np.isnan(g['X']).all(axis=1).sum()) == 3 and int(np.isnan(g['Y']).all(axis=1).sum()) == 1


def test_header_declares_and_a_unit_defines_the_entry():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+plsx_simpls_crossval_batch\s*\(\s*plsx_ctx\s*\*', header)
    defined = False
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            if re.search(r'\bint\s+plsx_simpls_crossval_batch\s*\([^;{]*\)\s*try\s*\{', f.read(), re.S):
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


def test_wrong_cvsamples_shape_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    masks = np.ones((40, 5), dtype=bool)
    masks[:10] = False
    with pytest.raises(ValueError, match=r'`cvsamples` must have shape \(S, test_split\) = \(40, 4\)'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=4, cvsamples=masks, verbose=False)
    with pytest.raises(ValueError, match=r'`cvsamples` must have shape'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=5, cvsamples=masks[:-1], verbose=False)


def test_split_with_one_test_row_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    masks = np.ones((40, 3), dtype=bool)
    masks[:10, 0] = False
    masks[5:15, 1] = False
    masks[7, 2] = False                                   # one test row
    with pytest.raises(ValueError, match=r'at least 2 usable test rows; split 2 has 1'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=3, cvsamples=masks, verbose=False)
    # a masked (all-NaN) row is on neither side: two test rows of which one is NaN throughout leave one
    masks[8, 2] = False
    Xn = X.copy()
    Xn[8] = np.nan
    with pytest.raises(ValueError, match=r'at least 2 usable test rows; split 2 has 1'):
        pls.pls_regression(Xn, Y, n_components=3, n_perm=0, n_boot=0, test_split=3, cvsamples=masks, verbose=False)


def test_n_components_too_large_for_the_training_rows_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    masks = np.ones((40, 2), dtype=bool)
    masks[:10, 0] = False                                 # 30 training rows
    masks[:28, 1] = False                                 # 12 training rows: at most 11 components
    with pytest.raises(ValueError, match=r'`n_components` cannot be greater than 11 '):
        pls.pls_regression(X, Y, n_components=12, n_perm=0, n_boot=0, test_split=2, cvsamples=masks, verbose=False)
    # drawn splits: floor(40 * 0.5) = 20 training rows at least -> at most 19 components
    with pytest.raises(ValueError, match=r'`n_components` cannot be greater than 19 '):
        pls.pls_regression(X, Y, n_components=25, n_perm=0, n_boot=0, test_split=4, test_size=0.5, verbose=False)


def test_drawn_splits_count_masked_rows_before_any_engine(no_engine):
    """Drawn masks: rows that are NaN throughout may fall on either side, so the worst case is checked up front."""
    import pypyls_amd as pls
    X, Y, rs = _data()
    X[[2, 9, 30]] = np.nan
    # 40 - ceil(40 * 0.9) = 4 test rows, of which 3 may be masked
    with pytest.raises(ValueError, match=r'at least 2 usable test rows; test_size = 0.1 can leave 1 of 40 \(3 rows'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=4, test_size=0.1, verbose=False)
    # floor(40 * 0.5) - 3 = 17 usable training rows at least -> at most 16 components
    with pytest.raises(ValueError, match=r'`n_components` cannot be greater than 16 '):
        pls.pls_regression(X, Y, n_components=17, n_perm=0, n_boot=0, test_split=4, test_size=0.5, verbose=False)
    with pytest.raises(ValueError, match=r'test_size must be in \[0, 1\)'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=4, test_size=1.5, verbose=False)


def test_cvres_keys():
    from pypyls_amd.structures import PLSCrossValidationResults, PLSResults
    new = dict(pearson_r_ncomp=np.zeros((3, 2, 4)), r_squared_ncomp=np.ones((3, 2, 4)), mse=np.ones((3, 4)),
               cvsamples=np.ones((10, 4), dtype=bool))
    rec = PLSCrossValidationResults(pearson_r=np.zeros((3, 4)), r_squared=np.zeros((3, 4)), unknown_key=1, **new)
    assert set(rec.keys()) == {'pearson_r', 'r_squared'} | set(new)
    assert 'unknown_key' not in rec
    res = PLSResults(cvres=dict(new, bogus=2))
    assert set(res.cvres.keys()) == set(new)
    assert res.cvres.cvsamples.dtype == bool
