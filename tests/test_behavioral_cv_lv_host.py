"""behavioral_pls(cv_lv=), the out-of-sample score correlation of the latent variables: what can be checked without a
GPU -- the definition of tests/behavioral_cv_lv_expect.py tied to the existing one of the prediction, its invariances,
the gap rule the device tolerance rests on (a Gram-side solve against the oracle SVD), the p-value rule, validation
before any engine exists, the C ABI declarations, the result records and their round trip."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import cpu_ref as ref
import crossval_expect as cx
import behavioral_cv_perm_expect as px
import behavioral_cv_lv_expect as lx

ENTRIES = ('plsx_crossval_lv_batch', 'plsx_crossval_perm_lv_batch')
TIE_CASES = ['E2', 'E4', 'E7', 'E8', 'E12', 'E13']


@pytest.mark.parametrize('name', TIE_CASES)
def test_scores_tie_to_the_prediction(name):
    """pred - ybar_train = x_score_live @ V_live[jT:(j+1)T]^T: the x_score IS the z of crossval_expect.single; the
    scores of every test row are finite in the live columns."""
    spec, X, Y, masks = cx.problem(name)
    T = Y.shape[1]
    dummy = spec.dummy.astype(bool)
    for s in range(min(masks.shape[1], 4)):
        mask = masks[:, s]
        xs, ys, dec = lx.scores(spec, X, Y, mask)
        live, V = dec['live'], dec['V']
        assert np.isfinite(xs[:, live]).all() and np.isfinite(ys[:, live]).all()
        assert np.isnan(xs[:, ~live]).all() and np.isnan(ys[:, ~live]).all()
        pred = np.full(Y.shape, np.nan)
        rows = np.flatnonzero(~mask)
        for j in range(dummy.shape[1]):
            tr, te = dummy[:, j] & mask, dummy[:, j] & ~mask
            if te.any():
                sel = np.isin(rows, np.flatnonzero(te))
                pred[te] = xs[sel][:, live] @ V[j * T:(j + 1) * T][:, live].T + Y[tr].mean(axis=0, keepdims=True)
        r, r2 = ref.efficient_corr(Y[~mask], pred[~mask]), ref.r2_score_raw(Y[~mask], pred[~mask])
        want_r, want_r2, _ = cx.single(spec, X, Y, mask)
        assert np.max(np.abs(r - want_r)) <= 1e-12 and np.max(np.abs(r2 - want_r2) / np.maximum(1, np.abs(want_r2))) <= 1e-12


def test_sign_of_V_does_not_matter():
    spec, X, Y, masks = cx.problem('E2')
    mask = masks[:, 0]
    _, _, dec = lx.scores(spec, X, Y, mask)
    flip = np.where(np.arange(dec['V'].shape[1]) % 2 == 0, -1.0, 1.0)
    a, _, _ = lx.single(spec, X, Y, mask)
    b, _, _ = lx.single(spec, X, Y, mask, V=dec['V'] * flip)
    assert np.isfinite(a).all() and np.max(np.abs(a - b)) <= 1e-14


@pytest.mark.parametrize('name', cx.DEFICIENT)
def test_dead_latent_variables_are_nan(name):
    lv, relgap, live = lx.expected(name)
    _, _, info = cx.expected(name)
    for s, i in enumerate(info):
        assert int(live[:, s].sum()) == i['n_live'] < i['L'] == lv.shape[0]
        assert np.isnan(lv[~live[:, s], s]).all() and np.isfinite(lv[live[:, s], s]).all()
        assert live[:i['n_live'], s].all()                       # the live LVs are the leading ones


def test_values_are_correlations_and_signal_shows():
    """The statistic is O(1): on data with signal the first LV generalises (what makes a wrong row, cell or LV show)."""
    lv, relgap, live = lx.expected('E1')
    assert np.all(np.abs(lv[live]) <= 1.0)
    from pypyls_amd import resampling
    X, Y = cx.data(80, 20, 2, seed=1, signal=2.0)
    masks = resampling.gen_splits([80], 1, 10, seed=3, test_size=cx.TEST_SIZE)
    strong, _, _ = lx.crossval_lv(ref.Spec('behavioral', [80], 1, False), X, Y, masks)
    assert strong[0].mean() > 0.8


def gram_side(spec, X, Y, mask):
    """lv_corr with V, d from eigh of R R^T (the side the device solves on) instead of the oracle SVD."""
    R, _, _, _, _, _ = lx.decomposition(spec, X, Y, mask)
    lam, V = np.linalg.eigh(R @ R.T)
    order = np.argsort(lam)[::-1][:min(R.shape)]
    return lx.single(spec, X, Y, mask, V=V[:, order])[0]


@pytest.mark.parametrize('name', list(cx.CASES))
def test_gap_rule_and_cap_on_every_case(name):
    """The cap of the GPU test on the expectation (at most 2 % of the live entries without a gap, never LV 0), and the
    measurement its tolerance rests on: a Gram-side solve on the host stays a factor 1000 inside the tolerance."""
    spec, X, Y, masks = cx.problem(name)
    lv, relgap, live = lx.expected(name)
    n_out = lx.check_cap(relgap, live, name)
    n = min(masks.shape[1], 3)
    got = np.stack([gram_side(spec, X, Y, masks[:, s]) for s in range(n)], -1)
    use = live[:, :n] & (relgap[:, :n] >= lx.RELGAP_MIN)
    err = np.abs(got - lv[:, :n])[use]
    worst = float((err / lx.tolerance(relgap[:, :n][use])).max())
    scaled = float((err * relgap[:, :n][use]).max())
    print('{}: {} of {} live entries left out; Gram side: max error / tolerance {:.2e}, max |d| * relgap {:.2e}'
          .format(name, n_out, int(live.sum()), worst, scaled))
    assert worst <= 1e-3


@pytest.mark.parametrize('name', ['E2', 'E12'])
def test_null_cases_pass_the_cap(name):
    lv, relgap, live = lx.null_expected(name)
    spec, X, Y, masks, perms = px.problem(name)
    assert lv.shape == (live.shape[0], perms.shape[1], masks.shape[1])
    assert lx.check_cap(relgap.reshape(len(lv), -1), live.reshape(len(lv), -1), name + ' null') == 0


def test_identity_permutation_is_the_observed_value():
    spec, X, Y, masks, _ = px.problem('E2')
    ident = np.arange(len(X))[:, None]
    lv, _, _ = lx.null(spec, X, Y, ident, masks)
    want, _, _ = lx.expected('E2')
    assert np.array_equal(lv[:, 0], want[:, :masks.shape[1]])


def test_cell_constant_feature_has_scale_zero():
    spec, X, Y, masks, perms = px.problem('E2')
    mask = masks[:, 0]
    cell = spec.dummy[:, 1].astype(bool)
    Xk = X.copy()
    Xk[cell & mask, 3] = Xk[cell & mask, 3][0]
    assert px.cell_constant(spec, Xk, mask)[1, 3]
    lv, relgap, live = lx.single(spec, Xk, Y[perms[:, 0]], mask)
    assert live.all() and np.isfinite(lv).all()


def test_split_mean_and_pvalues_follow_the_rule():
    a = np.array([[[0.1, 0.2, 0.3], [0.1, np.nan, 0.3]]])          # (L = 1, P = 2, n = 3)
    m = lx.split_mean(a)
    assert abs(m[0, 0] - 0.2) < 1e-15 and np.isnan(m[0, 1])
    observed = np.array([[0.4, 0.6], [0.0, 0.2], [np.nan, 0.3]])   # means 0.5, 0.1, NaN
    null = np.array([[0.5, 0.6, np.nan, 0.4], [0.1, 0.1, 0.1, np.nan], [0.9, 0.9, 0.9, 0.9]])
    p = lx.pvals(null, observed)
    # a tie is not larger (strict '>'), a NaN null value compares false, a NaN observed mean gives NaN -- not 1 / (P + 1)
    assert np.array_equal(p[:2], np.array([(1 + 1) / 5, (0 + 1) / 5])) and np.isnan(p[2])
    from pypyls_amd import plsc
    got = plsc._lv_corr_pvals(observed, null)
    assert np.array_equal(got[:2], p[:2]) and np.isnan(got[2])


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
    return X, rs.randn(S, T) + 0.5 * X[:, :T]


KW = dict(n_perm=0, n_boot=0, verbose=False)


def test_keyword_is_validated_before_any_engine(no_engine):
    import pypyls_amd as pls
    X, Y = _data()
    with pytest.raises(ValueError, match=r'`cv_lv` needs cross-validation'):
        pls.behavioral_pls(X, Y, cv_lv=True, test_split=0, **KW)
    with pytest.raises(ValueError, match=r'`cv_lv` needs cross-validation'):
        pls.behavioral_pls(X, Y, cv_lv=2, test_split=4, test_size=0, **KW)
    with pytest.raises(ValueError, match=r'`cv_lv` is not available with `contrasts`'):
        pls.behavioral_pls(X, Y, cv_lv=True, test_split=4, contrasts=np.eye(3)[:, :2], **KW)


@pytest.mark.parametrize('bad', [0, -1, 4, 2.0, '2', np.True_])
def test_bad_cv_lv_raises(no_engine, bad):
    """L = min(T', B) = 3 here; two groups make it 6."""
    import pypyls_amd as pls
    X, Y = _data()
    with pytest.raises(ValueError, match=r'`cv_lv` must be True or a number of latent variables in 1 \.\. 3'):
        pls.behavioral_pls(X, Y, cv_lv=bad, test_split=4, **KW)
    with pytest.raises(ValueError, match=r'in 1 \.\. 6; got 7'):
        pls.behavioral_pls(X, Y, groups=[20, 20], cv_lv=7, test_split=4, **KW)


def test_cv_lv_belongs_to_behavioral_pls(no_engine):
    import pypyls_amd as pls
    X, Y = _data()
    with pytest.raises(ValueError, match=r'`cv_lv` .* is not available for mean-centred PLS'):
        pls.meancentered_pls(X, groups=[20, 20], cv_lv=True, **KW)
    with pytest.raises(ValueError, match=r'`cv_lv` .* is not available for multiblock PLS'):
        pls.multiblock_pls(X, Y, groups=[20, 20], cv_lv=2, **KW)


def test_keys_are_allowed_in_the_records():
    from pypyls_amd.structures import PLSInputs, PLSCrossValidationResults
    assert 'cv_lv' in PLSInputs.allowed
    for key in ('lv_corr', 'perm_lv_corr', 'lv_corr_pvals'):
        assert key in PLSCrossValidationResults.allowed, key


def test_results_round_trip(tmp_path):
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    rs = np.random.RandomState(3)
    lv = rs.rand(2, 5)
    lv[1, 3] = np.nan
    res = PLSResults(x_weights=rs.randn(6, 2), singvals=np.array([2.0, 1.0]),
                     cvres=dict(pearson_r=rs.rand(3, 5), r_squared=rs.rand(3, 5), lv_corr=lv,
                                perm_lv_corr=rs.rand(2, 7), lv_corr_pvals=np.array([0.125, np.nan])),
                     inputs=dict(X=rs.randn(8, 6), Y=rs.randn(8, 3), test_split=5, cv_perm=7, cv_lv=2))
    path = io.save_results(str(tmp_path / 'lv'), res)
    back = io.load_results(path)
    for key in ('lv_corr', 'perm_lv_corr', 'lv_corr_pvals'):
        assert np.array_equal(back.cvres[key], res.cvres[key], equal_nan=True), key
    assert int(back.inputs.cv_lv) == 2


def test_header_engine_and_library_carry_the_entries():
    from pypyls_amd import engine, _build
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+plsx_crossval_lv_batch\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*d_masks\s*,'
                     r'\s*int\s+m\s*,\s*double\s*\*\s*d_r\s*,\s*double\s*\*\s*d_r2\s*,\s*double\s*\*\s*d_lv\s*,'
                     r'\s*void\s*\*\s*stream\s*\)', header)
    assert re.search(r'\bint\s+plsx_crossval_perm_lv_batch\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*d_masks\s*,'
                     r'\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*d_perm_idx\s*,\s*int\s+m\s*,\s*double\s*\*\s*d_r\s*,'
                     r'\s*double\s*\*\s*d_r2\s*,\s*double\s*\*\s*d_lv\s*,\s*double\s*\*\s*d_lv_pairs\s*,'
                     r'\s*void\s*\*\s*stream\s*\)', header)
    # the existing entries keep their signatures
    assert re.search(r'\bint\s+plsx_crossval_batch\s*\(\s*plsx_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*d_masks\s*,\s*int\s+m\s*,'
                     r'\s*double\s*\*\s*d_r\s*,\s*double\s*\*\s*d_r2\s*,\s*void\s*\*\s*stream\s*\)', header)
    _build.build()
    lib = engine._load()
    for entry in ENTRIES:
        assert entry in engine.exported_symbols(), entry
        assert hasattr(lib, entry), entry
    assert hasattr(engine.Engine, 'crossval_perm_lv')
    labels, k = [], 0
    while lib.plsx_kernel_class_name(k):
        labels.append(lib.plsx_kernel_class_name(k).decode())
        k += 1
    assert 'k_cv_lv' in labels and 'k_cvp_lv' in labels and 'k_cv_final' in labels
