"""pls_regression(cv_perm=P), the permutation test of the cross-validated prediction: what can be checked without a GPU
-- the oracle helper against the fixtures the reference wrote (tests/golden/make_cv_perm_golden.py), the conditions
those fixtures must meet, validation before any engine exists, the C ABI declaration, the built library and the records."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from regression_cv_perm_expect import cv_perm_expected, gaps, abs_err, rel_err

TAGS = ['a', 'b', 'nan']
PIN = 1e-10            # helper vs reference fixtures (the generator measured 1.9e-14 at worst)
GAP = 1e-4             # no observed split-mean this close to a null value: a device error of 1e-5 cannot flip a p-value
ENTRY = 'plsx_simpls_crossval_perm_batch'
KEYS = ('perm_pearson_r', 'perm_r_squared', 'perm_mse', 'pearson_r_pvals', 'r_squared_pvals', 'mse_pvals', 'cvpermsamples')


def _expected(tag):
    g, f = load_golden('simpls_cv_' + tag), load_golden('simpls_cv_perm_' + tag)
    return g, f, cv_perm_expected(g['X'], g['Y'], g['cvsamples'], f['cvpermsamples'], int(g['n_components']))


@pytest.mark.parametrize('tag', TAGS)
def test_helper_reproduces_the_reference_fixtures(tag):
    g, f, want = _expected(tag)
    k, T, P = int(g['n_components']), g['Y'].shape[1], f['cvpermsamples'].shape[1]
    assert P == 12 and f['ref_perm_r'].shape == (T, k, P) and f['ref_perm_r2'].shape == (T, k, P)
    assert f['ref_perm_mse'].shape == (k + 1, P)
    errs = dict(obs_r=abs_err(want['obs']['r'], f['ref_obs_r']), obs_r2=rel_err(want['obs']['r2'], f['ref_obs_r2']),
                obs_mse=rel_err(want['obs']['mse'], f['ref_obs_mse']),
                null_r=abs_err(want['null']['r'], f['ref_perm_r']), null_r2=rel_err(want['null']['r2'], f['ref_perm_r2']),
                null_mse=rel_err(want['null']['mse'], f['ref_perm_mse']))
    print('simpls_cv_perm_{}: oracle vs reference {}'.format(tag, errs))
    assert max(errs.values()) <= PIN, (tag, errs)
    # the observed split-means are those of the cross-validation fixture itself
    assert abs_err(f['ref_obs_r'], g['ref_r'].mean(axis=-1)) <= 1e-14
    for key in ('r', 'r2', 'mse'):
        assert np.array_equal(want['pvals'][key], f['pvals_' + key]), (tag, key)


@pytest.mark.parametrize('tag', TAGS)
def test_fixture_conditions(tag):
    g, f, want = _expected(tag)
    S, P = f['cvpermsamples'].shape
    assert S == len(g['X']) and np.issubdtype(f['cvpermsamples'].dtype, np.integer)
    assert np.array_equal(np.sort(f['cvpermsamples'], axis=0), np.broadcast_to(np.arange(S)[:, None], (S, P)))
    assert len({tuple(c) for c in f['cvpermsamples'].T}) == P
    for key in ('ref_obs_r', 'ref_obs_r2', 'ref_obs_mse', 'ref_perm_r', 'ref_perm_r2', 'ref_perm_mse'):
        assert np.isfinite(f[key]).all(), key
    gap = gaps(dict(r=f['ref_obs_r'], r2=f['ref_obs_r2'], mse=f['ref_obs_mse']),
               dict(r=f['ref_perm_r'], r2=f['ref_perm_r2'], mse=f['ref_perm_mse']))
    print('simpls_cv_perm_{}: smallest gap between an observed and a null value {}'.format(tag, gap))
    assert min(gap.values()) > GAP, (tag, gap)
    for key in ('pvals_r', 'pvals_r2', 'pvals_mse'):
        assert f[key].min() >= 1 / (P + 1) - 1e-15 and f[key].max() <= 1.0
        assert np.allclose(f[key] * (P + 1), np.round(f[key] * (P + 1)), atol=1e-12)


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


def test_cv_perm_without_cross_validation_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    kw = dict(n_components=3, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match=r'`cv_perm` needs cross-validation'):
        pls.pls_regression(X, Y, cv_perm=5, **kw)
    with pytest.raises(ValueError, match=r'`cv_perm` needs cross-validation'):
        pls.pls_regression(X, Y, cv_perm=5, test_split=4, test_size=0, **kw)
    masks = np.ones((40, 4), dtype=bool)
    masks[:10] = False
    with pytest.raises(ValueError, match=r'`cv_perm` needs cross-validation'):
        pls.pls_regression(X, Y, cv_perm=5, cvsamples=masks, **kw)         # (cvsamples alone: test_split is 0)


@pytest.mark.parametrize('bad', [-1, 2.5, True, '3', None])
def test_bad_cv_perm_raises(no_engine, bad):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r'`cv_perm` must be a non-negative integer'):
        pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=4, cv_perm=bad, verbose=False)


def test_wrong_cvpermsamples_shape_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    perms = np.stack([rs.permutation(40) for _ in range(5)], axis=1)
    kw = dict(n_components=3, n_perm=0, n_boot=0, test_split=4, verbose=False)
    with pytest.raises(ValueError, match=r'`cvpermsamples` must have shape \(S, cv_perm\) = \(40, 4\)'):
        pls.pls_regression(X, Y, cv_perm=4, cvpermsamples=perms, **kw)
    with pytest.raises(ValueError, match=r'`cvpermsamples` must have shape'):
        pls.pls_regression(X, Y, cv_perm=5, cvpermsamples=perms[:-1], **kw)
    with pytest.raises(ValueError, match=r'`cvpermsamples` must have shape'):
        pls.pls_regression(X, Y, cv_perm=5, cvpermsamples=perms.T, **kw)


def test_columns_that_are_not_permutations_raise(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    perms = np.stack([rs.permutation(40) for _ in range(3)], axis=1)
    kw = dict(n_components=3, n_perm=0, n_boot=0, test_split=4, cv_perm=3, verbose=False)
    dup = perms.copy()
    dup[0, 2] = dup[1, 2]                                   # a row drawn twice: a bootstrap, not a permutation
    with pytest.raises(ValueError, match=r'one permutation of 0 \.\. 39 per column; column 2 is not one'):
        pls.pls_regression(X, Y, cvpermsamples=dup, **kw)
    out = perms.copy()
    out[3, 1] = 40
    with pytest.raises(IndexError, match=r'out of bounds'):                  # (engine.check_index_array, as permsamples)
        pls.pls_regression(X, Y, cvpermsamples=out, **kw)
    with pytest.raises(IndexError, match=r'integer row indices'):
        pls.pls_regression(X, Y, cvpermsamples=perms.astype(float), **kw)


def test_header_engine_and_library_carry_the_entry():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+' + ENTRY + r'\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*d_masks\s*,\s*int\s+n\s*,'
                     r'\s*const\s+int32_t\s*\*\s*d_perm_idx\s*,\s*int\s+m\s*,', header)
    defined = False
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            if re.search(r'\bint\s+' + ENTRY + r'\s*\([^;{]*\)\s*try\s*\{', f.read(), re.S):
                defined = True
    assert defined
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        src = f.read()
    assert src.count("'" + ENTRY + "'") >= 2                 # the ctypes signature and the required-symbol list
    from pypyls_amd import _build, engine
    _build.build()
    assert ENTRY in set(engine.exported_symbols())
    assert callable(getattr(engine.Engine, 'simpls_crossval_perm_into'))


def test_records_declare_the_new_surface():
    import inspect
    import pypyls_amd as pls
    from pypyls_amd import structures as st
    assert set(KEYS) <= set(st.PLSCrossValidationResults.allowed) and 'cv_perm' in st.PLSInputs.allowed
    rec = st.PLSCrossValidationResults(perm_mse=np.zeros((3, 4)), mse_pvals=np.ones(3), bogus=1)
    assert set(rec.keys()) == {'perm_mse', 'mse_pvals'}
    # a record that was not given the keyword holds no trace of it, and a cross-validation without it none of the keys
    assert 'cv_perm' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1, test_split=3)
    assert st.PLSInputs(X=np.zeros((2, 2)), n_components=1, test_split=3, cv_perm=7).cv_perm == 7
    res = st.PLSResults(cvres=dict(pearson_r=np.zeros((3, 4)), mse=np.ones((2, 4))))
    assert not set(KEYS) & set(res.cvres.keys())
    sig = inspect.signature(pls.pls_regression).parameters
    assert sig['cv_perm'].default == 0 and sig['cvpermsamples'].default is None


def test_save_load_round_trip_of_the_keys(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g, f, want = _expected('b')
    k = int(g['n_components'])
    res = PLSResults(x_weights=np.zeros((g['X'].shape[1], k)),
                     inputs=dict(X=g['X'], Y=g['Y'], n_components=k, test_split=8, test_size=0.25, cv_perm=12))
    new = dict(perm_pearson_r=want['null']['r'], perm_r_squared=want['null']['r2'], perm_mse=want['null']['mse'],
               pearson_r_pvals=want['pvals']['r'], r_squared_pvals=want['pvals']['r2'], mse_pvals=want['pvals']['mse'],
               cvpermsamples=f['cvpermsamples'])
    res['cvres'].update(new)
    back = pls.load_results(pls.save_results(str(tmp_path / 'cv_perm'), res))
    assert int(back.inputs.cv_perm) == 12
    for key, val in new.items():
        assert np.array_equal(back.cvres[key], val) and back.cvres[key].shape == val.shape, key
    assert np.issubdtype(back.cvres.cvpermsamples.dtype, np.integer)
