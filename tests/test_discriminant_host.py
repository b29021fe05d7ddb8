"""pls_da, PLS discriminant analysis with cross-validated accuracy: what can be checked without a GPU -- the oracle helper
against the fixtures the reference wrote (tests/golden/make_da_golden.py) with their margins, the stratified split draw,
every refusal before any engine exists, the scores and p-values from hand-made confusion matrices, predict_class, the C
ABI declarations, the built library, the records and their persistence."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from discriminant_expect import MARGIN, da_expected, one_hot, stratified_expected

TAGS = ['a', 'b', 'nan']
ENTRIES = ('plsx_simpls_set_classes', 'plsx_simpls_cv_class_begin', 'plsx_simpls_cv_class_end')
CV_KEYS = ('confusion', 'accuracy', 'balanced_accuracy', 'perm_confusion', 'perm_accuracy', 'perm_balanced_accuracy',
           'accuracy_pvals', 'balanced_accuracy_pvals')


@pytest.mark.parametrize('tag', TAGS)
def test_helper_reproduces_the_reference_fixtures(tag):
    g = load_golden('simpls_da_' + tag)
    k, G, n = int(g['n_components']), int(g['y'].max()) + 1, g['cvsamples'].shape[1]
    want = da_expected(g['X'], g['y'], g['cvsamples'], k)
    print('simpls_da_{}: margin oracle {:.3e} reference {:.3e}'.format(tag, want['margin'], float(g['ref_margin'])))
    assert want['margin'] >= MARGIN and float(g['ref_margin']) >= MARGIN
    assert g['ref_confusion'].shape == (G, G, k, n) and np.issubdtype(g['ref_confusion'].dtype, np.integer)
    assert np.array_equal(want['confusion'], g['ref_confusion'])
    # every usable test row is counted once per component count, and the fixture is neither perfect nor at chance
    usable = ~np.isnan(g['X']).all(axis=1)
    n_te = (~g['cvsamples'] & usable[:, None]).sum(axis=0)
    assert np.array_equal(g['ref_confusion'].sum(axis=(0, 1)), np.broadcast_to(n_te, (k, n)))
    import pypyls_amd as pls
    acc, bal = pls.scores_from_confusion(g['ref_confusion'].sum(axis=-1))
    print('simpls_da_{}: pooled accuracy {} balanced {}'.format(tag, np.round(acc, 3).tolist(), np.round(bal, 3).tolist()))
    assert acc.max() < 1.0 and bal.max() > 1.2 / G


def test_fixture_nan_design():
    g = load_golden('simpls_da_nan')
    assert np.bincount(g['y']).tolist() == [30, 20, 12, 8]
    nan = np.isnan(g['X'])
    assert nan.all(axis=1).sum() == 3 and not (nan.any(axis=1) & ~nan.all(axis=1)).any()


# ---- stratified splits

def _labels(sizes, seed):
    rs = np.random.RandomState(seed)
    return rs.permutation(np.repeat(np.arange(len(sizes)), sizes))


@pytest.mark.parametrize('test_size', [0.25, 0.4])
def test_stratified_masks(test_size):
    from pypyls_amd import resampling as rsmp
    sizes = (30, 21, 13, 7)
    y = _labels(sizes, 5)
    masks = rsmp.gen_stratified_splits(y, 12, seed=77, test_size=test_size)
    assert masks.shape == (71, 12) and masks.dtype == bool
    for g, n_g in enumerate(sizes):
        kept = masks[y == g].sum(axis=0)
        want = n_g * (1 - test_size)
        assert set(kept.tolist()) <= {int(np.floor(want)), int(np.ceil(want))}, (g, kept)
    assert np.array_equal(masks, rsmp.gen_stratified_splits(y, 12, seed=77, test_size=test_size))    # a seeded draw repeats
    assert not np.array_equal(masks, rsmp.gen_stratified_splits(y, 12, seed=78, test_size=test_size))
    sorted_masks = rsmp.gen_splits(list(sizes), 1, 12, seed=77, test_size=test_size)
    assert np.array_equal(masks, stratified_expected(y, sorted_masks))
    ys = np.sort(y)                                        # already sorted: gen_splits(counts, 1, ...) itself
    assert np.array_equal(rsmp.gen_stratified_splits(ys, 12, seed=77, test_size=test_size), sorted_masks)


# ---- refusals: all on the host, before any engine

@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def _data(S=40, B=30, sizes=(16, 14, 10), seed=0):
    rs = np.random.RandomState(seed)
    y = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    X = rs.randn(S, B)
    X[:, :len(sizes)] += one_hot(y)
    return X, y, rs


KW = dict(n_components=3, n_perm=0, n_boot=0, verbose=False)


def test_bad_label_arrays_raise(no_engine):
    import pypyls_amd as pls
    X, y, rs = _data()
    with pytest.raises(ValueError, match=r'`y` must be a 1-D array'):
        pls.pls_da(X, one_hot(y), **KW)
    with pytest.raises(ValueError, match=r'`y` must be a 1-D array'):
        pls.pls_da(X, y[:-1], **KW)
    with pytest.raises(ValueError, match=r'NaN label'):
        pls.pls_da(X, np.where(np.arange(40) == 3, np.nan, y.astype(float)), **KW)
    obj = y.astype(object)
    obj[7] = None
    with pytest.raises(ValueError, match=r'None or NaN label'):
        pls.pls_da(X, obj, **KW)
    obj[7] = float('nan')
    with pytest.raises(ValueError, match=r'None or NaN label'):
        pls.pls_da(X, obj, **KW)


def test_class_count_bounds_raise(no_engine):
    import pypyls_amd as pls
    rs = np.random.RandomState(1)
    X = rs.randn(99, 20)
    with pytest.raises(ValueError, match=r'at least 2 classes'):
        pls.pls_da(X, np.zeros(99, dtype=int), **KW)
    with pytest.raises(ValueError, match=r'at most 32 classes.*k_sd_cv_class'):
        pls.pls_da(X, np.arange(99) % 33, **KW)


def test_small_classes_raise(no_engine):
    import pypyls_amd as pls
    X, y, rs = _data()
    y1 = y.copy()
    y1[np.flatnonzero(y == 2)[1:]] = 0                     # class 2 keeps one row
    with pytest.raises(ValueError, match=r'at least 2 usable rows; class 2 has 1'):
        pls.pls_da(X, y1, **KW)
    Xn = X.copy()
    Xn[np.flatnonzero(y == 2)[1:]] = np.nan                # ten rows, nine of them NaN throughout
    with pytest.raises(ValueError, match=r'at least 2 usable rows; class 2 has 1 \(9 of its 10 rows'):
        pls.pls_da(Xn, y, **KW)


def test_test_size_that_can_empty_a_class_raises(no_engine):
    import pypyls_amd as pls
    X, y, rs = _data(sizes=(20, 17, 3))
    # floor(3 * 0.2) = 0 training rows of class 2
    with pytest.raises(ValueError, match=r'usable training row of every class; test_size = 0.8 can leave class 2'):
        pls.pls_da(X, y, test_split=4, test_size=0.8, **KW)
    # the worst case counts the masked rows: floor(3 * 0.5) = 1 training row, which may be the row that is NaN throughout
    Xn = X.copy()
    Xn[np.flatnonzero(y == 2)[0]] = np.nan
    with pytest.raises(ValueError, match=r'can leave class 2 \(3 rows, 1 of them NaN throughout\)'):
        pls.pls_da(Xn, y, test_split=4, test_size=0.5, n_components=2, n_perm=0, n_boot=0, verbose=False)


def test_cvsamples_without_a_class_on_the_training_side_raise(no_engine):
    import pypyls_amd as pls
    X, y, rs = _data()
    masks = np.ones((40, 3), dtype=bool)
    masks[:8] = False
    masks[np.flatnonzero(y == 1), 2] = False               # split 2 trains on no row of class 1
    with pytest.raises(ValueError, match=r'split 2 of `cvsamples` has none of class 1'):
        pls.pls_da(X, y, test_split=3, cvsamples=masks, **KW)
    # ... and a usable one is what counts
    masks = np.ones((40, 3), dtype=bool)
    masks[:8] = False
    rows = np.flatnonzero(y == 2)
    masks[rows[1:], 1] = False
    Xn = X.copy()
    Xn[rows[0]] = np.nan
    with pytest.raises(ValueError, match=r'split 1 of `cvsamples` has none of class 2'):
        pls.pls_da(Xn, y, test_split=3, cvsamples=masks, **KW)


@pytest.mark.parametrize('kw', [dict(n_split=5), dict(n_split=0), dict(aggfunc='mean'), dict(rotate=True)])
def test_keywords_pls_da_does_not_take_raise(no_engine, kw):
    import pypyls_amd as pls
    X, y, rs = _data()
    with pytest.raises(ValueError, match=r'`pls_da` takes no `{}`'.format(list(kw)[0])):
        pls.pls_da(X, y, **KW, **kw)


def test_the_checks_of_pls_regression_apply(no_engine):
    import pypyls_amd as pls
    X, y, rs = _data()
    with pytest.raises(ValueError, match=r'Expected 2D array for `X`'):
        pls.pls_da(X[:, 0], y, **KW)
    with pytest.raises(ValueError, match=r'`n_components` cannot be greater than'):
        pls.pls_da(X, y, n_components=31, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match=r'`cv_perm` needs cross-validation'):
        pls.pls_da(X, y, cv_perm=5, **KW)
    with pytest.raises(ValueError, match=r'`cvsamples` must have shape'):
        pls.pls_da(X, y, test_split=3, cvsamples=np.ones((40, 4), dtype=bool), **KW)
    with pytest.raises(ValueError, match=r'`coef_components` must be an integer in 1'):
        pls.pls_da(X, y, coef_components=4, **KW)
    # stratified worst case of the component count: floor(16 .5) + floor(14 .5) + floor(10 .5) = 20 training rows
    with pytest.raises(ValueError, match=r'`n_components` cannot be greater than 19 when cross-validating'):
        pls.pls_da(X, y, test_split=3, test_size=0.5, n_components=20, n_perm=0, n_boot=0, verbose=False)


def test_a_valid_call_passes_the_checks_and_only_then_asks_for_an_engine(monkeypatch):
    import pypyls_amd as pls
    from pypyls_amd import engine

    class Asked(Exception):
        pass

    def asked(*a, **k):
        raise Asked()
    monkeypatch.setattr(engine, 'default_engine', asked)
    monkeypatch.setattr(engine.Engine, '__init__', asked)
    X, y, rs = _data()
    names = np.array(['ctl', 'pat', 'sib'])[y]
    for labels in (y, names, y == 0):
        with pytest.raises(Asked):
            pls.pls_da(X, labels, test_split=4, cv_perm=3, coef_components=2, vip_components=2, **KW)


# ---- scores and p-values

def test_scores_from_confusion_on_hand_made_matrices():
    import pypyls_amd as pls
    conf = np.array([[5, 1, 0], [2, 2, 0], [0, 1, 3]])
    acc, bal = pls.scores_from_confusion(conf)
    assert acc.shape == () and bal.shape == ()
    assert acc == 10 / 14 and bal == (5 / 6 + 2 / 4 + 3 / 4) / 3
    # a class absent from the test side is left out of the mean, not counted as a recall of zero
    absent = np.array([[4, 1, 0], [0, 0, 0], [1, 0, 2]])
    acc, bal = pls.scores_from_confusion(absent)
    assert acc == 6 / 8 and bal == (4 / 5 + 2 / 3) / 2
    # trailing axes pass through
    both = np.stack([conf, absent], axis=-1)[..., None, :].repeat(2, axis=2)          # (3, 3, 2, 2)
    acc, bal = pls.scores_from_confusion(both)
    assert acc.shape == (2, 2) and np.array_equal(acc, [[10 / 14, 6 / 8]] * 2)
    assert np.array_equal(bal, [[(5 / 6 + 2 / 4 + 3 / 4) / 3, (4 / 5 + 2 / 3) / 2]] * 2)
    acc, bal = pls.scores_from_confusion(np.zeros((2, 2), dtype=int))
    assert np.isnan(acc) and np.isnan(bal)
    with pytest.raises(ValueError):
        pls.scores_from_confusion(np.zeros((2, 3)))


def test_pvalue_rule_counts_ties():
    from pypyls_amd.discriminant import confusion_results
    # one split, k = 1, G = 2: observed accuracy 6 / 8; nulls 5 / 8, 6 / 8 (a tie), 7 / 8
    obs = np.array([[[[3, 1], [1, 3]]]], dtype=float)                                  # (n = 1, k = 1, G, G)
    null = np.array([[[[3, 1], [2, 2]]], [[[3, 1], [1, 3]]], [[[4, 0], [1, 3]]]], dtype=float)
    out = confusion_results(obs, null)
    assert out['confusion'].shape == (2, 2, 1, 1) and out['confusion'].dtype == np.int64
    assert out['perm_confusion'].shape == (2, 2, 1, 3)
    assert np.array_equal(out['perm_accuracy'], [[5 / 8, 6 / 8, 7 / 8]])
    assert np.array_equal(out['accuracy_pvals'], [(2 + 1) / (3 + 1)])                 # with > it would be 2 / 4
    assert np.array_equal(out['balanced_accuracy_pvals'], [(2 + 1) / (3 + 1)])
    assert set(out) == set(CV_KEYS)
    assert set(confusion_results(obs)) == {'confusion', 'accuracy', 'balanced_accuracy'}


def test_pvalues_compare_the_pooled_observed_statistic():
    from pypyls_amd.discriminant import confusion_results
    # two splits of unequal size: the pooled accuracy (2 + 6) / (4 + 8) differs from the mean of 2 / 4 and 6 / 8
    obs = np.array([[[[1, 1], [1, 1]]], [[[3, 1], [1, 3]]]], dtype=float)
    null = np.array([[[[4, 2], [2, 4]]]], dtype=float)                                 # 8 / 12: ties the pooled value
    out = confusion_results(obs, null)
    assert np.array_equal(out['accuracy'], [[2 / 4, 6 / 8]])
    assert np.array_equal(out['accuracy_pvals'], [1.0])


def _hand_made_result(labels):
    from pypyls_amd.structures import PLSResults
    rs = np.random.RandomState(3)
    X = rs.randn(12, 5)
    codes = np.arange(12) % 3
    W = np.linalg.qr(rs.randn(5, 3))[0]
    Yc = one_hot(codes) - one_hot(codes).mean(axis=0)
    res = PLSResults(x_weights=W, y_loadings=Yc.T @ ((X - X.mean(axis=0)) @ W), x_scores=(X - X.mean(axis=0)) @ W,
                     inputs=dict(X=X, Y=one_hot(codes), n_components=3, coef_components=2))
    res['classes'] = np.asarray(labels)
    return res, rs


def test_predict_class_on_a_hand_made_result():
    import pypyls_amd as pls
    res, rs = _hand_made_result(['ctl', 'pat', 'sib'])
    X_new = rs.randn(7, 5)
    for c in (None, 1, 3):
        got = pls.predict_class(res, X_new, n_components=c)
        assert got.shape == (7,)
        assert np.array_equal(got, res.classes[np.argmax(pls.predict(res, X_new, n_components=c), axis=1)])
    assert len(set(pls.predict_class(res, rs.randn(60, 5)).tolist())) > 1
    del res['classes']
    with pytest.raises(ValueError, match=r'not a pls_da result'):
        pls.predict_class(res, X_new)
    with pytest.raises(ValueError, match=r'not a pls_da result'):
        pls.predict_class(dict(x_weights=1), X_new)


# ---- declarations, library, records

def test_header_engine_and_library_carry_the_entries():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+plsx_simpls_set_classes\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*d_class\s*,'
                     r'\s*int\s+G\s*,\s*void\s*\*\s*stream\s*\)\s*;', header)
    assert re.search(r'\bint\s+plsx_simpls_cv_class_begin\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*int32_t\s*\*\s*d_conf\s*,'
                     r'\s*long\s+long\s+capacity\s*\)\s*;', header)
    assert re.search(r'\bint\s+plsx_simpls_cv_class_end\s*\(\s*plsx_ctx\s*\*\s*ctx\s*\)\s*;', header)
    sources = ''
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            sources += f.read()
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        src = f.read()
    for entry in ENTRIES:
        assert re.search(r'\bint\s+' + entry + r'\s*\([^;{]*\)\s*try\s*\{', sources, re.S), entry
        assert src.count("'" + entry + "'") >= 2, entry     # the ctypes signature and the required-symbol list
    assert '"k_sd_cv_class"' in sources                     # the kernel-timing class
    from pypyls_amd import _build, engine
    _build.build()
    assert set(ENTRIES) <= set(engine.exported_symbols())
    lib = engine._load()
    names, i = [], 0
    while lib.plsx_kernel_class_name(i):
        names.append(lib.plsx_kernel_class_name(i).decode())
        i += 1
    assert 'k_sd_cv_class' in names and 'k_sd_cv_score' in names
    import ctypes
    assert lib.plsx_simpls_set_classes.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    assert lib.plsx_simpls_cv_class_begin.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    assert lib.plsx_simpls_cv_class_end.argtypes == [ctypes.c_void_p]
    for method in ('simpls_set_classes', 'simpls_cv_class_begin', 'simpls_cv_class_end'):
        assert callable(getattr(engine.Engine, method))


def test_records_and_exports_declare_the_new_surface():
    import inspect
    import pypyls_amd as pls
    from pypyls_amd import structures as st
    assert set(CV_KEYS) <= set(st.PLSCrossValidationResults.allowed)
    assert 'classes' in st.PLSResults.allowed
    allowed = list(st.PLSInputs.allowed)
    assert '_classes' in allowed and '_splitsamples' in allowed
    res = st.PLSResults(cvres=dict(pearson_r=np.zeros((3, 4))))
    assert not set(CV_KEYS) & set(res.cvres.keys()) and 'classes' not in res
    for name in ('pls_da', 'predict_class', 'scores_from_confusion'):
        assert callable(getattr(pls, name))
    sig = inspect.signature(pls.pls_da).parameters
    shared = ('n_components', 'n_perm', 'n_boot', 'ci', 'permsamples', 'bootsamples', 'seed', 'verbose', 'n_proc',
              'test_split', 'test_size', 'cvsamples', 'cv_perm', 'cvpermsamples', 'coef_components', 'coef_ci',
              'coef_perm', 'vip_components')
    ref = inspect.signature(pls.pls_regression).parameters
    for name in shared:
        assert sig[name].default == ref[name].default or (sig[name].default is None and ref[name].default is None), name
    for name in ('rotate', 'aggfunc', 'n_split'):
        assert name not in sig


def test_save_load_round_trip_of_the_keys(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.discriminant import confusion_results
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g = load_golden('simpls_da_b')
    k = int(g['n_components'])
    res, rs = _hand_made_result([3, 5, 8])
    blocks = g['ref_confusion'].transpose(3, 2, 0, 1).astype(float)
    new = confusion_results(blocks, blocks[::-1][:5])
    res['cvres'].update(new)
    back = pls.load_results(pls.save_results(str(tmp_path / 'da'), res))
    assert np.array_equal(back.classes, [3, 5, 8]) and np.issubdtype(back.classes.dtype, np.integer)
    for key, val in new.items():
        assert np.array_equal(back.cvres[key], val) and back.cvres[key].shape == val.shape, key
    assert np.issubdtype(back.cvres.confusion.dtype, np.integer) and back.cvres.confusion.shape == (2, 2, k, 8)
    X_new = rs.randn(6, 5)
    assert np.array_equal(pls.predict_class(back, X_new), pls.predict_class(res, X_new))
