"""pls_regression(inner_split=ni), the nested cross-validation of n_components: what can be checked without a GPU -- the
expectation (tests/regression_nested_expect.py) against a hand-computed two-split case, the draw of the inner folds,
validation before any engine exists, the C ABI declaration, the ctypes signatures, the Engine methods, the records and
the documents."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import regression_nested_expect as ne

ENTRIES = ('plsx_simpls_crossval_nested_batch', 'plsx_simpls_crossval_nested_perm_batch')
KEYS = ('nested_ncomp', 'nested_pearson_r', 'nested_r_squared', 'nested_mse', 'inner_mse', 'innersamples')
PERM_KEYS = ('perm_nested_pearson_r', 'perm_nested_r_squared', 'perm_nested_mse', 'perm_nested_ncomp',
             'nested_pearson_r_pvals', 'nested_r_squared_pvals', 'nested_mse_pvals')


# ---- the expectation ---------------------------------------------------------------------------------------------

def _by_hand(X, y, tr, te):
    """B = 2, T = 1, k = 2, written out: -> mse of c = 0, 1, 2 over the test rows, and r, r2 of c = 1, 2.
    c = 1: PLS1's first weight is X_c' y_c, the prediction ybar + t (t'y_c) / (t't); c = 2 = B: ordinary least squares."""
    Xc, yc = X[tr] - X[tr].mean(axis=0), y[tr] - y[tr].mean()
    w = Xc.T @ yc
    t = Xc @ w
    slope = (t @ yc) / (t @ t)
    p1 = y[tr].mean() + ((X[te] - X[tr].mean(axis=0)) @ w) * slope
    beta = np.linalg.lstsq(Xc, yc, rcond=None)[0]
    p2 = y[tr].mean() + (X[te] - X[tr].mean(axis=0)) @ beta
    p0 = np.full(te.sum(), y[tr].mean())
    mse = [float(np.sum((y[te] - p) ** 2) / te.sum()) for p in (p0, p1, p2)]
    r = [float(np.corrcoef(y[te], p)[0, 1]) for p in (p1, p2)]
    r2 = [float(1 - np.sum((y[te] - p) ** 2) / np.sum((y[te] - y[te].mean()) ** 2)) for p in (p1, p2)]
    return np.array(mse), r, r2


def _two_split_case():
    rs = np.random.RandomState(7)
    S = 16
    X = rs.randn(S, 2)
    y = X @ np.array([1.0, -2.0]) + 0.3 * rs.randn(S)
    codes = np.zeros((S, 2, 3), dtype=np.uint8)
    outer_test = [np.arange(0, 4), np.arange(10, 16)]
    for s in range(2):
        codes[:, s, 0] = 1
        codes[outer_test[s], s, 0] = 0
        tr = np.flatnonzero(codes[:, s, 0] == 1)
        for j in range(2):
            codes[:, s, 1 + j] = 2
            codes[tr, s, 1 + j] = 1
            codes[tr[j::3], s, 1 + j] = 0
    return X, y, codes


def test_expectation_against_a_hand_computed_two_split_case():
    X, y, codes = _two_split_case()
    got = ne.nested_expected(X, y[:, None], codes, 2)
    assert got['inner_mse'].shape == (3, 2) and got['ncomp'].shape == (2,) and got['r'].shape == (1, 2)
    for s in range(2):
        folds = [_by_hand(X, y, codes[:, s, j] == 1, codes[:, s, j] == 0)[0] for j in (1, 2)]
        inner = (folds[0] + folds[1]) / 2
        best = 1 if not inner[2] < inner[1] else 2
        mse, r, r2 = _by_hand(X, y, codes[:, s, 0] == 1, codes[:, s, 0] == 0)
        print('split {}: inner_mse {} -> c = {}; outer mse {:.6f} r {:.6f} r2 {:.6f}'
              .format(s, inner, best, mse[best], r[best - 1], r2[best - 1]))
        assert np.allclose(got['inner_mse'][:, s], inner, rtol=1e-10, atol=0)
        assert got['ncomp'][s] == best
        assert np.isclose(got['mse'][s], mse[best], rtol=1e-10)
        assert np.isclose(got['r'][0, s], r[best - 1], atol=1e-10) and np.isclose(got['r2'][0, s], r2[best - 1], rtol=1e-10)
    # the signal lives in both features: the full model wins everywhere
    assert list(got['ncomp']) == [2, 2]
    # under a permutation the selection is repeated inside it, and the identity permutation is the observed data
    same = ne.nested_perm_expected(X, y[:, None], codes, 2, np.arange(16)[:, None])
    assert np.array_equal(same['ncomp'][:, 0], [0, 2])
    assert np.isclose(same['mse'][0], got['mse'].mean(), rtol=1e-14) and np.allclose(same['r'][:, 0], got['r'].mean(axis=1))


def test_selection_rule_first_minimum_nan_and_undefined():
    nan, inf = np.nan, np.inf
    assert ne.select(np.array([0.1, 3.0, 2.0, 2.0, 2.5])) == 2           # the first minimum wins
    assert ne.select(np.array([0.0, 1.0, 1.0, 1.0])) == 1                # c = 0 is not a candidate
    assert ne.select(np.array([0.0, 3.0, nan, 2.0])) == 3                # a NaN is never smaller
    assert ne.select(np.array([0.0, nan, 1.0, 0.5])) == 0                # ... and nothing is smaller than a NaN: undefined
    assert ne.select(np.array([0.0, inf, inf])) == 0
    assert ne.select(np.array([5.0, 2.0])) == 1


def test_selection_gap_and_pvals():
    a = np.array([[9.0, 9.0], [1.0, 4.0], [1.5, 2.0], [3.0, 2.5]])          # (k + 1, n): row 0 does not count
    assert np.isclose(ne.selection_gap(a), min(0.5 / 1.0, 0.5 / 2.0))
    b = np.stack([a, a + 0.0], axis=-1)
    b[2, 1, 1] = 2.4                                                       # a permutation's group: (2.5 - 2.4) / 2.4
    assert np.isclose(ne.selection_gap(a, b), 0.1 / 2.4)
    null = np.array([[0.1, 0.5, np.nan, 0.3]])
    assert np.array_equal(ne.pvals(np.array([0.3]), null), [2 / 5])         # a NaN is not larger
    assert np.array_equal(ne.pvals(np.array([0.3]), null, smaller=True), [2 / 5])


# ---- the draw of the inner folds ---------------------------------------------------------------------------------

@pytest.mark.parametrize('S, n, ni, test_size', [(41, 3, 4, 0.25), (30, 2, 3, 0.4)])
def test_inner_draw(S, n, ni, test_size):
    from pypyls_amd import resampling
    from pypyls_amd.regression import _draw_inner_codes, nested_codes
    masks = resampling.gen_splits([S], 1, n, seed=5, test_size=test_size)
    codes = _draw_inner_codes(masks, ni, np.random.RandomState(99), test_size)
    assert codes.shape == (S, n, ni) and codes.dtype == np.uint8 and set(np.unique(codes)) <= {0, 1, 2}
    # 2 exactly on the outer test rows
    assert np.array_equal(codes == 2, np.broadcast_to(~masks[:, :, None], codes.shape))
    # ceil or floor of n_tr (1 - test_size) inner training rows
    n_tr = masks.sum(axis=0)
    for s in range(n):
        kept = (codes[:, s] == 1).sum(axis=0)
        print('split {}: {} training rows, inner training rows {}'.format(s, n_tr[s], kept))
        assert all(v in (int(np.floor(n_tr[s] * (1 - test_size))), int(np.ceil(n_tr[s] * (1 - test_size)))) for v in kept)
        assert ((codes[:, s] == 0).sum(axis=0) == n_tr[s] - kept).all()
    # the sequence of generator calls, from a fresh RandomState: split by split, on the training rows in ascending order
    rs = np.random.RandomState(99)
    for s in range(n):
        rows = np.flatnonzero(masks[:, s])
        want = resampling.gen_splits([len(rows)], 1, ni, seed=rs, test_size=test_size)
        assert np.array_equal(codes[rows, s, :] == 1, want), s
    full = nested_codes(masks, codes)
    assert full.shape == (S, n, 1 + ni) and np.array_equal(full[:, :, 0], masks) and np.array_equal(full[:, :, 1:], codes)


# ---- validation before any engine ---------------------------------------------------------------------------------

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


KW = dict(n_components=3, n_perm=0, n_boot=0, verbose=False)


def _given(S=40, n=2, ni=2):
    masks = np.ones((S, n), dtype=bool)
    for s in range(n):
        masks[s * 10:(s + 1) * 10, s] = False
    inner = np.full((S, n, ni), 2, dtype=np.uint8)
    for s in range(n):
        tr = np.flatnonzero(masks[:, s])
        for j in range(ni):
            inner[tr, s, j] = 1
            inner[tr[j::4], s, j] = 0
    return masks, inner


def test_inner_split_without_cross_validation_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r'`inner_split` needs cross-validation'):
        pls.pls_regression(X, Y, inner_split=3, **KW)
    with pytest.raises(ValueError, match=r'`inner_split` needs cross-validation'):
        pls.pls_regression(X, Y, inner_split=3, test_split=4, test_size=0, **KW)


@pytest.mark.parametrize('bad', [-1, 2.5, True, '3', None])
def test_bad_inner_split_raises(no_engine, bad):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r'`inner_split` must be a non-negative integer'):
        pls.pls_regression(X, Y, test_split=4, inner_split=bad, **KW)


def test_wrong_innersamples_raise(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    masks, inner = _given()
    kw = dict(test_split=2, cvsamples=masks, inner_split=2, **KW)
    with pytest.raises(ValueError, match=r'`innersamples` must have shape \(S, test_split, inner_split\) = \(40, 2, 2\)'):
        pls.pls_regression(X, Y, innersamples=inner[:, :, :1], **kw)
    with pytest.raises(ValueError, match=r'`innersamples` must have shape'):
        pls.pls_regression(X, Y, innersamples=inner.transpose(1, 0, 2), **kw)
    with pytest.raises(ValueError, match=r'`innersamples` needs `inner_split`'):
        pls.pls_regression(X, Y, test_split=2, cvsamples=masks, innersamples=inner, **KW)
    with pytest.raises(ValueError, match=r'`innersamples` needs `cvsamples`'):
        pls.pls_regression(X, Y, test_split=2, inner_split=2, innersamples=inner, **KW)
    bad = inner.copy()
    bad[0, 1, 0] = 3
    with pytest.raises(ValueError, match=r'codes 0 \(test row\), 1 \(training row\) and 2'):
        pls.pls_regression(X, Y, innersamples=bad, **kw)
    leak = inner.copy()
    leak[3, 0, 1] = 0                                        # an outer test row of split 0 on the test side of a fold
    with pytest.raises(ValueError, match=r'2 exactly on the outer test rows.*row 3 of inner fold 1 of split 0'):
        pls.pls_regression(X, Y, innersamples=leak, **kw)
    out = inner.copy()
    out[25, 0, 0] = 2                                        # an outer training row on neither side
    with pytest.raises(ValueError, match=r'2 exactly on the outer test rows'):
        pls.pls_regression(X, Y, innersamples=out, **kw)
    few = inner.copy()
    tr = np.flatnonzero(masks[:, 1])
    few[tr, 1, 0] = 1
    few[tr[0], 1, 0] = 0                                     # one test row
    with pytest.raises(ValueError, match=r'Every inner fold needs at least 2 usable test rows'):
        pls.pls_regression(X, Y, innersamples=few, **kw)
    small = inner.copy()
    small[tr, 1, 1] = 0
    small[tr[:3], 1, 1] = 1                                  # three training rows: at most 2 components
    with pytest.raises(ValueError, match=r'`n_components` cannot be greater than 2 with `inner_split`'):
        pls.pls_regression(X, Y, innersamples=small, **kw)


def test_drawn_folds_worst_case_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data(S=20)
    # 20 rows -> 15 training rows (5 test rows) -> 11 or 12 inner training rows, 3 or 4 inner test rows; two masked rows
    # leave the outer splits their 3 usable test rows but can leave an inner fold 1
    Y[[0, 1]] = np.nan
    with pytest.raises(ValueError, match=r'Every inner fold needs at least 2 usable test rows'):
        pls.pls_regression(X, Y, test_split=3, inner_split=2, **KW)
    X, Y, rs = _data(S=20)
    with pytest.raises(ValueError, match=r'`n_components` cannot be greater than 10 with `inner_split`'):
        pls.pls_regression(X, Y, test_split=3, inner_split=2, **dict(KW, n_components=11))


def test_confounds_and_pls_da_refuse(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r'`inner_split` cannot be combined with `confounds`'):
        pls.pls_regression(X, Y, test_split=4, inner_split=2, confounds=rs.randn(40, 2), **KW)
    labels = np.arange(40) % 2
    with pytest.raises(ValueError, match=r'`inner_split` is not available for pls_da'):
        pls.pls_da(X, labels, test_split=4, inner_split=2, **KW)


# ---- the C ABI, the ctypes signatures, the Engine methods -------------------------------------------------------

def _header():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        return f.read()


def test_header_prototypes_and_comment():
    header = _header()
    ws = r'\s*'
    assert re.search(r'\bint\s+plsx_simpls_crossval_nested_batch' + ws + r'\(' + ws + r'plsx_ctx\s*\*\s*ctx\s*,' + ws +
                     r'const\s+uint8_t\s*\*\s*d_codes\s*,\s*int\s+n\s*,\s*int\s+ni\s*,\s*double\s*\*\s*d_r\s*,\s*double\s*\*'
                     r'\s*d_r2\s*,\s*double\s*\*\s*d_mse\s*,\s*int32_t\s*\*\s*d_ncomp\s*,\s*double\s*\*\s*d_inner_mse\s*,'
                     r'\s*void\s*\*\s*stream\s*\)\s*;', header)
    assert re.search(r'\bint\s+plsx_simpls_crossval_nested_perm_batch' + ws + r'\(' + ws + r'plsx_ctx\s*\*\s*ctx\s*,' + ws +
                     r'const\s+uint8_t\s*\*\s*d_codes\s*,\s*int\s+n\s*,\s*int\s+ni\s*,\s*const\s+int32_t\s*\*\s*d_perm_idx\s*,'
                     r'\s*int\s+m\s*,\s*double\s*\*\s*d_r\s*,\s*double\s*\*\s*d_r2\s*,\s*double\s*\*\s*d_mse\s*,\s*int32_t'
                     r'\s*\*\s*d_ncomp_count\s*,\s*void\s*\*\s*stream\s*\)\s*;', header)
    # the SIMPLS comment block documents both, the codes, the kernels and the refusals
    block = header[header.index(' *   plsx_simpls_crossval_nested_batch'):header.index(' *   plsx_simpls_set_confounds')]
    flat = re.sub(r'\s*\n \*\s*', ' ', block)
    for word in ('plsx_simpls_crossval_nested_perm_batch', '(n, 1 + ni, S)', '1 = training row, 0 = test row, 2 = on neither side',
                 'k_sd_cvn_expand', 'k_sd_cvn_select', 'k_sd_cvn_reduce', 'first minimum', 'PLSX_ERR_STATE', 'PLSX_ERR_ARG',
                 'PLSX_ERR_UNSUPPORTED', 'd_ncomp_count (m, k)', 'd_inner_mse (n, k + 1)'):
        assert word in flat, word


def test_entries_defined_declared_to_ctypes_and_exported():
    for entry in ENTRIES:
        defined = False
        for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
            with open(path) as f:
                if re.search(r'\bint\s+' + entry + r'\s*\([^;{]*\)\s*try\s*\{', f.read(), re.S):
                    defined = True
        assert defined, entry
    with open(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_simpls.h')) as f:
        kernels = f.read()
    for name in ('k_sd_cvn_expand', 'k_sd_cvn_select', 'k_sd_cvn_reduce'):
        assert re.search(r'__global__[^;{]*\bvoid\s+' + name + r'\s*\(', kernels, re.S), name
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        src = f.read()
    for entry in ENTRIES:
        assert src.count("'" + entry + "'") >= 2, entry           # the ctypes signature and the required-symbol list
    from pypyls_amd import _build, engine
    _build.build()
    assert set(ENTRIES) <= set(engine.exported_symbols())
    lib = engine._load()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert list(lib.plsx_simpls_crossval_nested_batch.argtypes) == [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    assert list(lib.plsx_simpls_crossval_nested_perm_batch.argtypes) == [vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    assert lib.plsx_simpls_crossval_nested_batch.restype is i32
    for name in ('simpls_crossval_nested_into', 'simpls_crossval_nested_perm_into', 'simpls_crossval_nested',
                 'simpls_crossval_nested_perm'):
        assert callable(getattr(engine.Engine, name)), name


def test_records_declare_the_new_surface():
    import inspect
    import pypyls_amd as pls
    from pypyls_amd import structures as st
    assert set(KEYS + PERM_KEYS) <= set(st.PLSCrossValidationResults.allowed) and 'inner_split' in st.PLSInputs.allowed
    assert 'inner_split' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1, test_split=3)
    assert st.PLSInputs(X=np.zeros((2, 2)), n_components=1, test_split=3, inner_split=4).inner_split == 4
    res = st.PLSResults(cvres=dict(pearson_r=np.zeros((3, 4)), mse=np.ones((2, 4))))
    assert not set(KEYS + PERM_KEYS) & set(res.cvres.keys())
    sig = inspect.signature(pls.pls_regression).parameters
    assert sig['inner_split'].default == 0 and sig['innersamples'].default is None


def test_documents_name_the_new_surface():
    for doc, words in (('DESIGN.md', ENTRIES + ('k_sd_cvn_expand', 'k_sd_cvn_select', 'k_sd_cvn_reduce', 'inner_split',
                                                'Nested cross-validation')),
                       ('INTEGRATION.md', ENTRIES + ('d_codes', 'd_ncomp_count')),
                       ('README.md', ('inner_split', 'nested_ncomp')), ('CHANGELOG.md', ('inner_split',))):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        for word in words:
            assert word in text, (doc, word)


def test_save_load_round_trip_of_the_keys(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    X, y, codes = _two_split_case()
    obs = ne.nested_expected(X, y[:, None], codes, 2)
    perms = np.stack([np.random.RandomState(i).permutation(16) for i in range(3)], axis=1)
    nul = ne.nested_perm_expected(X, y[:, None], codes, 2, perms)
    res = PLSResults(x_weights=np.zeros((2, 2)),
                     inputs=dict(X=X, Y=y[:, None], n_components=2, test_split=2, test_size=0.25, inner_split=2, cv_perm=3))
    new = dict(nested_ncomp=obs['ncomp'], nested_pearson_r=obs['r'], nested_r_squared=obs['r2'], nested_mse=obs['mse'],
               inner_mse=obs['inner_mse'], innersamples=codes[:, :, 1:].copy(), perm_nested_pearson_r=nul['r'],
               perm_nested_r_squared=nul['r2'], perm_nested_mse=nul['mse'], perm_nested_ncomp=nul['ncomp'],
               nested_pearson_r_pvals=ne.pvals(obs['r'].mean(axis=1), nul['r']),
               nested_r_squared_pvals=ne.pvals(obs['r2'].mean(axis=1), nul['r2']))
    res['cvres'].update(new)
    res['cvres']['nested_mse_pvals'] = float(ne.pvals(obs['mse'].mean(), nul['mse'], smaller=True))
    back = pls.load_results(pls.save_results(str(tmp_path / 'nested'), res))
    assert int(back.inputs.inner_split) == 2
    for key, val in new.items():
        assert np.array_equal(back.cvres[key], val) and back.cvres[key].shape == val.shape, key
    assert np.issubdtype(back.cvres.nested_ncomp.dtype, np.integer) and back.cvres.innersamples.dtype == np.uint8
    assert float(back.cvres.nested_mse_pvals) == res.cvres.nested_mse_pvals
