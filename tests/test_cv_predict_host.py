"""``cv_predict=`` (the out-of-fold predictions of pls_regression, pls_da and behavioral_pls): what can be checked without
a GPU -- the expectation module (tests/cv_predict_expect.py) against the oracles it stands beside, every ValueError before
any engine exists, ``roc_curve`` on hand-made inputs with ties, the I/O round trip, the C ABI declaration, the ctypes
signatures, the Engine methods, the records and the documents."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import cv_predict_expect as pe
from regression_cv_expect import cv_expected

ENTRIES = ('plsx_simpls_cv_pred_begin', 'plsx_simpls_cv_pred_end', 'plsx_crossval_pred_begin', 'plsx_crossval_pred_end')
KEYS = ('y_pred', 'y_pred_ncomp', 'y_true', 'predicted')
KW = dict(n_components=3, n_perm=0, n_boot=0, verbose=False)


def _data(S=40, B=12, T=2, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    return X, rs.randn(S, T) + 0.5 * X[:, :T], rs


# ---- the expectation ---------------------------------------------------------------------------------------------

def test_scores_recomputed_from_the_expected_predictions_are_cv_expected():
    """The module's y_pred is what regression_cv_expect.cv_expected reduces to r / r2 / mse and discards: rows that are
    NaN throughout on both sides of the masks, c on either side of the full model."""
    S, B, T, k = 70, 40, 3, 5
    X, Y, rs = _data(S, B, T, 3)
    X[4] = np.nan
    Y[9] = np.nan
    masks = np.ones((S, 4), dtype=bool)
    for s in range(4):
        masks[rs.choice(S, 18, replace=False), s] = False
    masks[[4, 9], 0] = [False, True]
    want = cv_expected(X, Y, masks, k)
    for c in (1, 4, 5):
        y_pred = pe.pred_expected(X, Y, masks, c)
        assert np.array_equal(~np.isnan(y_pred[:, 0, :]), pe.usable_test_rows(X, Y, masks))
        sc = pe.scores_from_pred(y_pred, Y)
        errs = (np.abs(sc['r'] - want['r'][:, c - 1]).max(), np.abs(sc['r2'] - want['r2'][:, c - 1]).max(),
                np.abs(sc['mse'] - want['mse'][c]).max(), np.abs(sc['sse'] - want['sse'][:, c]).max())
        print('c = {}: r {:.2e}  r2 {:.2e}  mse {:.2e}  sse {:.2e}'.format(c, *errs))
        assert max(errs) <= 1e-12 and np.array_equal(sc['n_test'], want['n_test'])
    # one count per split, 0 = an undefined split
    mixed = pe.pred_expected(X, Y, masks, [2, 0, 5, 1])
    assert np.isnan(mixed[:, :, 1]).all()
    assert np.array_equal(mixed[:, :, 2], pe.pred_expected(X, Y, masks, 5)[:, :, 2], equal_nan=True)


def test_behavioural_expectation_is_the_prediction_crossval_expect_scores():
    import crossval_expect as cx
    import behavioral_confound_expect as bx
    spec, X, Y, masks = cx.problem('E2')
    r, r2, _ = cx.expected('E2')
    y_pred = pe.behav_pred_expected(spec, X, Y, masks[:, :6])
    assert np.array_equal(np.isnan(y_pred[:, 0, :]), masks[:, :6])
    sc = pe.scores_from_pred(y_pred, Y)
    assert np.abs(sc['r'] - r[:, :6]).max() <= 1e-12 and np.abs(sc['r2'] - r2[:, :6]).max() <= 1e-12
    spec, X, Y, Z, masks = bx.problem('C2')
    exp = bx.expected('C2')
    y_pred, y_true = pe.behav_fold_expected(spec, X, Y, Z, masks)
    assert np.array_equal(np.isnan(y_pred), np.isnan(y_true))
    sc = pe.scores_from_pred(y_pred, y_true)
    assert np.abs(sc['r'] - exp['r']).max() <= 1e-12 and np.abs(sc['r2'] - exp['r2']).max() <= 1e-11


def test_class_expectation_recounts_the_confusion_of_discriminant_expect():
    from discriminant_expect import da_expected
    rs = np.random.RandomState(5)
    y = rs.permutation(np.repeat(np.arange(3), 20))
    X = rs.randn(60, 15)
    X[:, :3] += rs.randn(3, 3)[y]
    masks = np.ones((60, 3), dtype=bool)
    for s in range(3):
        masks[rs.choice(60, 15, replace=False), s] = False
    want = da_expected(X, y, masks, 4)
    for c in (1, 4):
        y_pred, predicted = pe.da_pred_expected(X, y, masks, c)
        assert np.array_equal(pe.confusion_from_predicted(predicted, y, 3), want['confusion'][:, :, c - 1, :])


# ---- validation, before any engine exists ------------------------------------------------------------------------

@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def test_cv_predict_without_cross_validation_raises(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    for kw in (dict(), dict(test_split=4, test_size=0)):
        with pytest.raises(ValueError, match=r'`cv_predict` needs cross-validation'):
            pls.pls_regression(X, Y, cv_predict=True, **dict(KW, **kw))
        with pytest.raises(ValueError, match=r'`cv_predict` needs cross-validation'):
            pls.pls_da(X, np.arange(40) % 2, cv_predict=2, **dict(KW, **kw))
        with pytest.raises(ValueError, match=r'`cv_predict` needs cross-validation'):
            pls.behavioral_pls(X, Y, cv_predict=True, n_perm=0, n_boot=0, verbose=False, **dict(dict(test_split=0), **kw))


@pytest.mark.parametrize('bad', [0, 4, -1, 2.0, 'all', 'Nested', [1, 2]])
def test_bad_cv_predict_raises(no_engine, bad):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r'`cv_predict` must be True, an integer in 1 \.\. n_components = 3'):
        pls.pls_regression(X, Y, test_split=4, cv_predict=bad, **KW)
    with pytest.raises(ValueError, match=r'`cv_predict` must be True, an integer in 1 \.\. n_components = 3; got'):
        pls.pls_da(X, np.arange(40) % 2, test_split=4, cv_predict=bad, **KW)
    with pytest.raises(ValueError, match=r'`cv_predict` must be True or False for behavioral_pls'):
        pls.behavioral_pls(X, Y, test_split=4, cv_predict=bad, n_perm=0, n_boot=0, verbose=False)


def test_nested_needs_inner_split_and_pls_da_refuses_it(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    with pytest.raises(ValueError, match=r"`cv_predict='nested'` needs `inner_split` > 0"):
        pls.pls_regression(X, Y, test_split=4, cv_predict='nested', **KW)
    with pytest.raises(ValueError, match=r"`cv_predict='nested'` is not available for pls_da"):
        pls.pls_da(X, np.arange(40) % 2, test_split=4, cv_predict='nested', **KW)


def test_plsc_refusals(no_engine):
    import pypyls_amd as pls
    X, Y, rs = _data()
    contrasts = np.linalg.qr(rs.randn(2, 2))[0]
    with pytest.raises(ValueError, match=r'`cv_predict` is not available with `contrasts`'):
        pls.behavioral_pls(X, Y, test_split=4, cv_predict=True, contrasts=contrasts, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match=r'`cv_predict` \(the out-of-fold predictions\) is not available for mean-centred PLS'):
        pls.meancentered_pls(X, groups=[20, 20], cv_predict=True, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match=r'`cv_predict` \(the out-of-fold predictions\) is not available for multiblock PLS'):
        pls.multiblock_pls(X, Y, groups=[20, 20], cv_predict=True, n_perm=0, n_boot=0, verbose=False)


# ---- roc_curve ---------------------------------------------------------------------------------------------------

def test_roc_points_by_hand_with_ties():
    from pypyls_amd.discriminant import roc_points
    scores = np.array([0.9, 0.8, 0.8, 0.8, 0.4, 0.4, 0.1, np.nan])
    positive = np.array([1, 1, 0, 1, 0, 1, 0, 1], dtype=bool)
    fpr, tpr, thr = roc_points(scores, positive)
    # 4 positives and 3 negatives are left; thresholds inf, 0.9, 0.8 (three rows at once), 0.4 (two), 0.1
    assert np.array_equal(thr, [np.inf, 0.9, 0.8, 0.4, 0.1])
    assert np.array_equal(tpr, [0, 1 / 4, 3 / 4, 1, 1])
    assert np.array_equal(fpr, [0, 0, 1 / 3, 2 / 3, 1])
    area = pe.trapezoid(fpr, tpr)
    assert abs(area - pe.auc_mann_whitney(scores[:7], positive[:7])) <= 1e-15
    assert abs(area - (2 * 8 + 3) / 24.0) <= 1e-15           # u2 by hand: 8 of the 12 pairs in order, 3 tied
    # all tied: the diagonal; one side empty: NaN on that axis
    fpr, tpr, thr = roc_points(np.ones(5), np.array([1, 0, 1, 0, 0], dtype=bool))
    assert np.array_equal(fpr, [0, 1]) and np.array_equal(tpr, [0, 1]) and pe.trapezoid(fpr, tpr) == 0.5
    fpr, tpr, thr = roc_points(np.array([0.3, 0.2]), np.array([True, True]))
    assert np.isnan(fpr).all() and np.array_equal(tpr, [0, 0.5, 1])
    with pytest.raises(ValueError):
        roc_points(np.zeros((2, 2)), np.zeros((2, 2), dtype=bool))


def test_roc_curve_reads_a_result_record():
    import pypyls_amd as pls
    from pypyls_amd.structures import PLSResults
    codes = np.array([0, 1, 2, 0, 1, 2, 0, 1])
    y_pred = np.full((8, 3, 2), np.nan)
    y_pred[[0, 1, 4, 6], :, 1] = [[0.7, 0.2, 0.1], [0.7, 0.2, 0.1], [0.1, 0.6, 0.3], [0.2, 0.5, 0.3]]
    onehot = np.zeros((8, 3))
    onehot[np.arange(8), codes] = 1.0
    res = PLSResults(inputs=dict(X=np.zeros((8, 2)), Y=onehot, _classes=codes), classes=np.array(['a', 'b', 'c']),
                     cvres=dict(y_pred=y_pred, y_pred_ncomp=np.array([2, 2], dtype=np.int32)))
    fpr, tpr, thr = pls.roc_curve(res, 'a', 1)
    # class a on the test rows 0 (a), 1 (b), 4 (b), 6 (a): scores 0.7, 0.7, 0.1, 0.2 -- the tie of rows 0 and 1 is one point
    assert np.array_equal(thr, [np.inf, 0.7, 0.2, 0.1])
    assert np.array_equal(tpr, [0, 0.5, 1, 1]) and np.array_equal(fpr, [0, 0.5, 0.5, 1])
    for bad in (dict(cls='z', split=1), dict(cls='a', split=2), dict(cls='a', split=1.5)):
        with pytest.raises(ValueError):
            pls.roc_curve(res, **bad)
    with pytest.raises(ValueError, match=r'no out-of-fold predictions'):
        pls.roc_curve(PLSResults(inputs=dict(X=np.zeros((8, 2)), Y=onehot), classes=np.array(['a', 'b', 'c'])), 'a', 0)


# ---- the C ABI, the ctypes signatures, the Engine methods, the records, the documents ---------------------------

def test_header_prototypes_and_comment():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+plsx_simpls_cv_pred_begin\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*int\s+c\s*,\s*int32_t\s*\*\s*d_ncomp\s*,'
                     r'\s*double\s*\*\s*d_pred\s*,\s*double\s*\*\s*d_true\s*,\s*long\s+long\s+capacity\s*\)\s*;', header)
    assert re.search(r'\bint\s+plsx_simpls_cv_pred_end\s*\(\s*plsx_ctx\s*\*\s*ctx\s*\)\s*;', header)
    assert re.search(r'\bint\s+plsx_crossval_pred_begin\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*d_pred\s*,\s*double\s*\*'
                     r'\s*d_true\s*,\s*long\s+long\s+capacity\s*\)\s*;', header)
    assert re.search(r'\bint\s+plsx_crossval_pred_end\s*\(\s*plsx_ctx\s*\*\s*ctx\s*\)\s*;', header)
    flat = re.sub(r'\s*\n \*\s*', ' ', header)
    for word in ('k_sd_cv_pred', 'k_cv_pred_export', 'plsx_simpls_crossval_confound_batch of m splits appends m slots',
                 'an all-NaN slot', 'The permutation entries append nothing', 'PLSX_ERR_UNSUPPORTED (context still usable',
                 'k_sd_cv_pred / k_cv_pred_export of an open'):
        assert word in flat, word


def test_entries_defined_declared_to_ctypes_and_exported():
    for entry in ENTRIES:
        defined = False
        for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
            with open(path) as f:
                if re.search(r'\bint\s+' + entry + r'\s*\([^;{]*\)\s*try\s*\{', f.read(), re.S):
                    defined = True
        assert defined, entry
    for fname, name in (('plsx_simpls.h', 'k_sd_cv_pred'), ('plsx_k_finish.h', 'k_cv_pred_export')):
        with open(os.path.join(ROOT, 'pypyls_amd', 'csrc', fname)) as f:
            assert re.search(r'__global__[^;{]*\bvoid\s+' + name + r'\s*\(', f.read(), re.S), name
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        src = f.read()
    for entry in ENTRIES:
        assert src.count("'" + entry + "'") >= 2, entry           # the ctypes signature and the required-symbol list
    from pypyls_amd import _build, engine
    _build.build()
    assert set(ENTRIES) <= set(engine.exported_symbols())
    lib = engine._load()
    vp, i32, ll = ctypes.c_void_p, ctypes.c_int32, ctypes.c_longlong
    assert list(lib.plsx_simpls_cv_pred_begin.argtypes) == [vp, i32, vp, vp, vp, ll]
    assert list(lib.plsx_crossval_pred_begin.argtypes) == [vp, vp, vp, ll]
    assert list(lib.plsx_simpls_cv_pred_end.argtypes) == [vp] == list(lib.plsx_crossval_pred_end.argtypes)
    for name in ('simpls_cv_pred_begin', 'simpls_cv_pred_end', 'crossval_pred_begin', 'crossval_pred_end'):
        assert callable(getattr(engine.Engine, name)), name


def test_records_and_signatures_declare_the_new_surface():
    import inspect
    import pypyls_amd as pls
    from pypyls_amd import structures as st
    assert set(KEYS) <= set(st.PLSCrossValidationResults.allowed) and 'cv_predict' in st.PLSInputs.allowed
    assert 'cv_predict' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1, test_split=3)
    assert st.PLSInputs(X=np.zeros((2, 2)), n_components=1, test_split=3, cv_predict='nested').cv_predict == 'nested'
    res = st.PLSResults(cvres=dict(pearson_r=np.zeros((3, 4))))
    assert not set(KEYS) & set(res.cvres.keys())
    for fn in (pls.pls_regression, pls.pls_da, pls.behavioral_pls):
        assert inspect.signature(fn).parameters['cv_predict'].default is False, fn
    assert callable(pls.roc_curve)


def test_documents_name_the_new_surface():
    for doc, words in (('DESIGN.md', ENTRIES + ('k_sd_cv_pred', 'k_cv_pred_export', 'cv_predict', 'Out-of-fold predictions')),
                       ('README.md', ('cv_predict', 'y_pred', 'roc_curve', 'cvsamples')),
                       ('CHANGELOG.md', ('cv_predict', 'k_sd_cv_pred', 'k_cv_pred_export'))):
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
    X, Y, rs = _data(S=30, T=2)
    masks = np.ones((30, 3), dtype=bool)
    for s in range(3):
        masks[s * 8:(s + 1) * 8, s] = False
    new = dict(y_pred=pe.pred_expected(X, Y, masks, [1, 2, 3]), y_pred_ncomp=np.array([1, 2, 3], dtype=np.int32),
               y_true=np.where(masks[:, None, :], np.nan, Y[:, :, None]),
               predicted=np.where(masks, -1, 1).astype(np.int32))
    for value in (True, 2, 'nested'):
        res = PLSResults(x_weights=np.zeros((12, 3)),
                         inputs=dict(X=X, Y=Y, n_components=3, test_split=3, test_size=0.25, cv_predict=value))
        res['cvres'].update(new)
        back = pls.load_results(pls.save_results(str(tmp_path / 'pred_{}'.format(value)), res))
        assert back.inputs.cv_predict == value
        for key, val in new.items():
            assert np.array_equal(back.cvres[key], val, equal_nan=True) and back.cvres[key].shape == val.shape, key
            assert back.cvres[key].dtype == val.dtype, key
