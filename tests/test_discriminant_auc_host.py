"""pls_da(auc=True), cross-validated one-vs-rest AUC with its permutation test: what can be checked without a GPU -- the
oracle helper against scikit-learn's roc_auc_score and against hand-made scores with ties and NaNs, auc_from_counts, the
p-value rule, every refusal before any engine exists, the C ABI declarations, the built library, the records and their
persistence."""
import glob
import os
import re
import warnings

import numpy as np
import pytest

from conftest import ROOT, load_golden
from discriminant_auc_expect import PAIR_MARGIN, auc_expected, auc_of, auc_perm_expected, pair_counts
from discriminant_expect import one_hot

ENTRIES = ('plsx_simpls_cv_auc_begin', 'plsx_simpls_cv_auc_end')
AUC_KEYS = ('auc_counts', 'auc', 'auc_macro', 'perm_auc_counts', 'perm_auc', 'perm_auc_macro', 'auc_pvals',
            'auc_macro_pvals')


# ---- the oracle helper

def _one_split_predictions(g, s):
    """The helper's own predictions of split s, formed a second time on the oracle: (pred_c for c = 1 .. k, true, te)."""
    from oracle import cpu_ref as ref
    X, y, k = g['X'], g['y'], int(g['n_components'])
    Y = one_hot(y)
    ok = ref.get_mask(X, Y)
    tr, te = g['cvsamples'][:, s] & ok, ~g['cvsamples'][:, s] & ok
    fit = ref.simpls(X[tr], Y[tr], k)
    scores = (X[te] - X[tr].mean(axis=0)) @ fit['x_weights']
    return [Y[tr].mean(axis=0) + scores[:, :c] @ fit['y_loadings'][:, :c].T for c in range(1, k + 1)], y[te], te


@pytest.mark.parametrize('tag', ['a', 'b', 'nan'])
def test_helper_agrees_with_sklearn_on_continuous_scores(tag):
    metrics = pytest.importorskip('sklearn.metrics')
    g = load_golden('simpls_da_' + tag)
    k, G = int(g['n_components']), int(g['y'].max()) + 1
    want = auc_expected(g['X'], g['y'], g['cvsamples'][:, :1], k)
    print('simpls_da_{}: pair margin of split 0 {:.3e}'.format(tag, want['margin']))
    assert want['margin'] >= PAIR_MARGIN and want['counts'].shape == (G, 2, k, 1)
    auc, macro = auc_of(want['counts'])
    import pypyls_amd as pls
    got_auc, got_macro = pls.auc_from_counts(want['counts'])          # the public function, against scikit-learn too
    assert np.array_equal(got_auc, auc) and np.allclose(got_macro, macro, rtol=0, atol=1e-15)
    preds, true, te = _one_split_predictions(g, 0)
    for c in range(k):
        for cls in range(G):
            n_pos = int((true == cls).sum())
            assert want['counts'][cls, 1, c, 0] == n_pos * (len(true) - n_pos) > 0
            sk = metrics.roc_auc_score(true == cls, preds[c][:, cls])
            assert abs(auc[cls, c, 0] - sk) < 1e-12, (c, cls, auc[cls, c, 0], sk)
        assert abs(macro[c, 0] - np.mean(auc[:, c, 0])) < 1e-15
    # neither perfect nor at chance
    assert 0.55 < np.nanmax(macro) < 1.0


def test_pair_counts_on_hand_made_scores_with_ties_and_nans():
    metrics = pytest.importorskip('sklearn.metrics')
    v = np.array([0.5, 0.5, 0.2, 0.9, 0.5, 0.1, 0.9])
    member = np.array([1, 0, 1, 0, 0, 1, 1], dtype=bool)
    # members 0.5, 0.2, 0.1, 0.9 against others 0.5, 0.9, 0.5:  0.5 -> ties 2;  0.2 -> 0;  0.1 -> 0;  0.9 -> wins 2, tie 1
    u2, pairs, margin = pair_counts(v, member)
    assert (u2, pairs) == (2 + 2 * 2 + 1, 12) and abs(margin - 0.3) < 1e-15
    assert abs(u2 / (2 * pairs) - metrics.roc_auc_score(member, v)) < 1e-15
    import pypyls_amd as pls
    u2_rest, pairs_rest, _ = pair_counts(v, ~member)                  # the other class of a two-class problem, scored by v
    auc, macro = pls.auc_from_counts([[u2, pairs], [u2_rest, pairs_rest]])
    assert auc[0] == u2 / (2 * pairs) and abs(auc[1] - metrics.roc_auc_score(~member, v)) < 1e-15
    assert abs(auc[0] + auc[1] - 1.0) < 1e-15 and macro == 0.5
    # a tolerance turns near-ties into ties and takes them out of the margin
    w = v.copy()
    w[1] += 1e-13
    assert pair_counts(w, member)[0] == u2 - 1 and pair_counts(w, member)[2] < 1e-12
    assert pair_counts(w, member, tie_tol=1e-12)[0] == u2 and abs(pair_counts(w, member, tie_tol=1e-12)[2] - 0.3) < 1e-12
    # a NaN compares false both ways: its pairs stay in `pairs` and add nothing
    n = v.copy()
    n[3] = np.nan                                                      # an other: the tie with the member at 0.9 goes
    assert pair_counts(n, member)[:2] == (u2 - 1, 12)
    n[0] = np.nan                                                      # a member: its two ties go too
    assert pair_counts(n, member)[:2] == (u2 - 3, 12)
    assert pair_counts(v, np.ones(7, dtype=bool)) == (0, 0, np.inf) and pair_counts(v, np.zeros(7, dtype=bool))[1] == 0


def test_helper_under_a_permutation_and_without_a_class():
    g = load_golden('simpls_da_a')
    k = int(g['n_components'])
    rs = np.random.RandomState(71)
    perms = np.stack([rs.permutation(len(g['y'])) for _ in range(2)], axis=1)
    masks = g['cvsamples'][:, :3]
    want = auc_perm_expected(g['X'], g['y'], masks, k, perms)
    one = auc_expected(g['X'], g['y'], masks, k, perm=perms[:, 1])
    assert want['counts'].shape == (3, 2, k, 2) and np.array_equal(want['counts'][..., 1], one['counts'].sum(axis=-1))
    assert want['margin'] >= PAIR_MARGIN
    # the pairs of a split depend on the classes of the permuted labels on its test side only
    true = g['y'][perms[:, 1]]
    for s in range(3):
        te = ~masks[:, s]
        for cls in range(3):
            n_pos = int((true[te] == cls).sum())
            assert np.all(one['counts'][cls, 1, :, s] == n_pos * (int(te.sum()) - n_pos))
    # a test side without class 0: no pair, NaN, and the macro mean is over the others
    masks0 = masks.copy()
    masks0[g['y'] == 0, 0] = True
    w0 = auc_expected(g['X'], g['y'], masks0, k)
    auc, macro = auc_of(w0['counts'])
    import pypyls_amd as pls
    assert np.array_equal(pls.auc_from_counts(w0['counts'])[0], auc, equal_nan=True)
    assert np.all(w0['counts'][0, :, :, 0] == 0) and np.isnan(auc[0, :, 0]).all() and not np.isnan(auc[1:, :, 0]).any()
    assert np.allclose(macro[:, 0], auc[1:, :, 0].mean(axis=0), rtol=0, atol=1e-15)


# ---- auc_from_counts, the p-value rule

def test_auc_from_counts_shapes_nan_rules_and_macro_mean():
    import pypyls_amd as pls
    counts = np.zeros((3, 2, 2, 4), dtype=np.int64)
    counts[:, 1] = 12
    counts[0, 0], counts[1, 0], counts[2, 0] = 24, 12, 6
    counts[2, :, 1, 3] = 0                                             # class 2 has no pair in one cell
    counts[:, :, 0, 0] = 0                                             # no class has one in another
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        auc, macro = pls.auc_from_counts(counts)
    assert auc.shape == (3, 2, 4) and macro.shape == (2, 4)
    assert np.array_equal(auc[:, 1, 1], [1.0, 0.5, 0.25]) and macro[1, 1] == (1.0 + 0.5 + 0.25) / 3
    assert np.isnan(auc[2, 1, 3]) and macro[1, 3] == 0.75
    assert np.isnan(auc[:, 0, 0]).all() and np.isnan(macro[0, 0])
    want_auc, want_macro = auc_of(counts)
    assert np.array_equal(auc, want_auc, equal_nan=True) and np.allclose(macro, want_macro, rtol=0, atol=1e-15, equal_nan=True)
    # no trailing axes; a list; integers beyond 2^31
    auc, macro = pls.auc_from_counts([[3, 2], [2 ** 40, 2 ** 40]])
    assert np.array_equal(auc, [0.75, 0.5]) and macro == 0.625
    for bad in (np.zeros(4), np.zeros((3, 3)), np.zeros((2, 3, 2))):
        with pytest.raises(ValueError, match=r'\(G, 2, \.\.\.\)'):
            pls.auc_from_counts(bad)


def test_pvalue_rule_counts_ties_pools_the_observed_and_keeps_nan():
    import pypyls_amd as pls
    from pypyls_amd.discriminant import auc_results
    # n = 2 splits of unequal size, k = 1, G = 2 -- blocks (n, k, G, 2).  Pooled observed AUC of class 0:
    # (4 + 20) / (2 * (4 + 16)) = 0.6, not the mean of 0.5 and 0.625
    obs = np.array([[[[4, 4], [4, 4]]], [[[20, 16], [12, 16]]]], dtype=float)
    null = np.array([[[[22, 20], [18, 20]]], [[[24, 20], [16, 20]]], [[[26, 20], [14, 20]]]], dtype=float)   # 0.55 0.6 0.65
    out = auc_results(obs, null)
    assert set(out) == set(AUC_KEYS) and set(auc_results(obs)) == {'auc_counts', 'auc', 'auc_macro'}
    assert out['auc_counts'].shape == (2, 2, 1, 2) and out['auc_counts'].dtype == np.int64
    assert out['perm_auc_counts'].shape == (2, 2, 1, 3) and out['perm_auc_counts'].dtype == np.int64
    assert np.array_equal(out['auc'][0], [[0.5, 0.625]]) and np.array_equal(out['auc_macro'], [[0.5, 0.5]])
    assert np.array_equal(out['perm_auc'][0], [[0.55, 0.6, 0.65]])
    assert np.array_equal(out['auc_pvals'][0], [(2 + 1) / (3 + 1)])    # the tie counts: with > it would be 2 / 4
    assert np.array_equal(out['auc_pvals'][1], [(2 + 1) / (3 + 1)])    # class 1: observed 0.4 against 0.45 0.4 0.35
    omacro = pls.auc_from_counts(out['auc_counts'].sum(axis=-1))[1]
    assert out['auc_macro_pvals'].shape == (1,)
    assert np.array_equal(out['auc_macro_pvals'], (np.sum(out['perm_auc_macro'] >= omacro[:, None], axis=1) + 1) / 4)
    # a class without a pair in the observed data: NaN, not 1 / (P + 1); NaN nulls are not >= anything
    obs0 = obs.copy()
    obs0[:, :, 1, :] = 0
    null0 = null.copy()
    null0[0, :, 0, :] = 0
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        out = auc_results(obs0, null0)
    assert np.isnan(out['auc_pvals'][1, 0]) and out['auc_pvals'][0, 0] == (2 + 1) / (3 + 1)
    # the macro means: observed 0.6 (class 0 alone) against 0.45 (class 1 alone), 0.5, 0.5
    assert np.isnan(out['perm_auc'][0, 0, 0]) and out['auc_macro_pvals'][0] == (0 + 1) / (3 + 1)


# ---- refusals before any engine exists

@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def test_auc_without_cross_validation_raises(no_engine):
    import pypyls_amd as pls
    rs = np.random.RandomState(0)
    y = rs.permutation(np.repeat(np.arange(3), (16, 14, 10)))
    X = rs.randn(40, 30)
    kw = dict(n_components=3, n_perm=0, n_boot=0, verbose=False, auc=True)
    with pytest.raises(ValueError, match=r'`auc=True` needs a cross-validation'):
        pls.pls_da(X, y, **kw)
    with pytest.raises(ValueError, match=r'`auc=True` needs a cross-validation'):
        pls.pls_da(X, y, test_split=0, **kw)
    with pytest.raises(ValueError, match=r'`auc=True` needs a cross-validation'):
        pls.pls_da(X, y, test_split=5, test_size=0, **kw)
    # ... and what pls_da refuses anyway, it still refuses first-hand with auc=True
    with pytest.raises(ValueError, match=r'at least 2 classes'):
        pls.pls_da(X, np.zeros(40, dtype=int), test_split=5, **kw)


# ---- declarations, library, records

def test_header_engine_and_library_carry_the_entries():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+plsx_simpls_cv_auc_begin\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*d_auc\s*,'
                     r'\s*long\s+long\s+capacity\s*\)\s*;', header)
    assert re.search(r'\bint\s+plsx_simpls_cv_auc_end\s*\(\s*plsx_ctx\s*\*\s*ctx\s*\)\s*;', header)
    assert re.search(r'\*\s+plsx_simpls_cv_auc_begin / plsx_simpls_cv_auc_end\n', header)      # the header comment
    assert re.search(r'16 k_sd_cv_auc\b', header)                                               # ... and the timing list
    sources = ''
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            sources += f.read()
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        src = f.read()
    for entry in ENTRIES:
        assert re.search(r'\bint\s+' + entry + r'\s*\([^;{]*\)\s*try\s*\{', sources, re.S), entry
        assert src.count("'" + entry + "'") >= 2, entry     # the ctypes signature and the required-symbol list
    assert '"k_sd_cv_auc"' in sources                       # the kernel-timing class
    with open(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_simpls.h')) as f:
        kernels = f.read()
    assert re.search(r'template\s*<\s*int\s+GB\s*,\s*bool\s+PERM\s*>[^;{]*\bvoid\s+k_sd_cv_auc\s*\(\s*SdArgs\s+a\s*\)', kernels)
    from pypyls_amd import _build, engine
    _build.build()
    assert set(ENTRIES) <= set(engine.exported_symbols())
    lib = engine._load()
    names, i = [], 0
    while lib.plsx_kernel_class_name(i):
        names.append(lib.plsx_kernel_class_name(i).decode())
        i += 1
    assert names.index('k_sd_cv_auc') == names.index('k_sd_cv_class') + 1 == 16
    import ctypes
    assert lib.plsx_simpls_cv_auc_begin.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    assert lib.plsx_simpls_cv_auc_end.argtypes == [ctypes.c_void_p]
    for method in ('simpls_cv_auc_begin', 'simpls_cv_auc_end'):
        assert callable(getattr(engine.Engine, method))


def test_records_and_exports_declare_the_new_surface():
    import inspect
    import pypyls_amd as pls
    from pypyls_amd import structures as st
    assert set(AUC_KEYS) <= set(st.PLSCrossValidationResults.allowed)
    assert '_auc' in st.PLSInputs.allowed and '_classes' in st.PLSInputs.allowed
    res = st.PLSResults(cvres=dict(pearson_r=np.zeros((3, 4))))
    assert not set(AUC_KEYS) & set(res.cvres.keys())
    assert callable(pls.auc_from_counts)
    sig = inspect.signature(pls.pls_da).parameters
    assert sig['auc'].default is False and sig['auc'].kind is inspect.Parameter.KEYWORD_ONLY
    assert 'auc' not in inspect.signature(pls.pls_regression).parameters


def test_documents_record_the_feature():
    def read(*parts):
        with open(os.path.join(ROOT, *parts)) as f:
            return f.read()
    readme, design, integ, changes = read('README.md'), read('DESIGN.md'), read('INTEGRATION.md'), read('CHANGELOG.md')
    assert 'auc=True' in readme and 'auc_from_counts' in readme
    offered = re.findall(r'Not offered:[^.]*\.', readme, re.S)        # (the sentence of the PLS-DA paragraph)
    assert any('stratified bootstraps' in sent for sent in offered) and not any('AUC' in sent for sent in offered)
    assert 'k_sd_cv_auc' in design and 'plsx_simpls_cv_auc_begin' in design
    assert 'plsx_simpls_cv_auc_begin' in integ and 'plsx_simpls_cv_auc_end' in integ
    assert 'auc=True' in changes and 'k_sd_cv_auc' in changes
    assert "'--auc'" in read('tools', 'da_profile.py')


def test_save_load_round_trip_of_the_keys(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.discriminant import auc_results
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g = load_golden('simpls_da_b')
    k = int(g['n_components'])
    masks = g['cvsamples'][:, :3]
    counts = auc_expected(g['X'], g['y'], masks, k)['counts']                    # (G, 2, k, 3)
    blocks = counts.transpose(3, 2, 0, 1).astype(float)
    pblocks = blocks[::-1][:2].copy()
    pblocks[0, :, 1, :] = 0                                                         # (a NaN in the null survives too)
    new = auc_results(blocks, pblocks)
    rs = np.random.RandomState(3)
    X, codes = rs.randn(12, 5), np.arange(12) % 2
    W = np.linalg.qr(rs.randn(5, 3))[0]
    Yc = one_hot(codes) - one_hot(codes).mean(axis=0)
    res = PLSResults(x_weights=W, y_loadings=Yc.T @ ((X - X.mean(axis=0)) @ W), x_scores=(X - X.mean(axis=0)) @ W,
                     inputs=dict(X=X, Y=one_hot(codes), n_components=3, _auc=True))
    res['classes'] = np.array([0, 1])
    res['cvres'].update(new)
    back = pls.load_results(pls.save_results(str(tmp_path / 'da_auc'), res))
    for key, val in new.items():
        assert np.array_equal(back.cvres[key], val, equal_nan=True) and back.cvres[key].shape == val.shape, key
    assert np.issubdtype(back.cvres.auc_counts.dtype, np.integer) and back.cvres.auc_counts.shape == (2, 2, k, 3)
    assert np.issubdtype(back.cvres.perm_auc_counts.dtype, np.integer)
