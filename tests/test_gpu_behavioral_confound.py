"""
behavioral_pls(confounds=Z) on the device: plsx_residualize (k_cf_resid), the fold-wise confound regression of the
cross-validation (plsx_crossval_confound_batch / plsx_crossval_confound_perm_batch: k_cf_fold_prep, k_cfb_fold_X,
k_cf_fold_Y, then the dual-space body of plsx_crossval_perm_batch on every split's own copy) and the front end, against
the numpy definition of tests/behavioral_confound_expect.py.  GPU only.

Tolerances: crossval_expect.TOL per ENTRY of r and r2 (the conditions it rests on -- kappa <= KAPPA_MAX, fold-wise and
whole-cohort scores >= 5e5 x TOL apart -- are asserted on the expectation, without a GPU, in
tests/test_behavioral_confound_host.py and again when the expectation is built); behavioral_cv_lv_expect.compare for
lv_corr; 1e-12 x max |column| for the residuals (the rule of tests/test_gpu_confound.py), RTOL = 1e-5 for the slopes.
Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import crossval_expect as cx
import behavioral_cv_lv_expect as lx
import behavioral_cv_perm_expect as bcp
import behavioral_confound_expect as bx
from confound_expect import residualise

pytestmark = pytest.mark.gpu
RTOL = 1e-5
SMALL = dict(scratch_gb=0.001)                          # one split's matrices and fold copy of C2 fit, two do not
_ENGINES = {}


def _engine(**options):
    from pypyls_amd.engine import Engine
    key = tuple(sorted(options.items()))
    if key not in _ENGINES:
        scratch = options.pop('scratch_gb', None)
        _ENGINES[key] = Engine(scratch_gb=scratch, options=options)
    return _ENGINES[key]


def _bind(eng, name):
    """Residualise on the device, bind the residuals, bind Z -> spec, X, Y, Z, masks and the residuals read back."""
    from pypyls_amd import resampling as rsmp
    case = bx.CASES[name]
    spec, X, Y, Z, masks = bx.problem(name)
    dX, dY = eng._dev(X, np.float64), eng._dev(Y, np.float64)
    gx, gy = eng.residualize(dX, Z), eng.residualize(dY, Z)
    eng.set_data(dX, dY, rsmp.cell_of_row(case['groups'], case['n_cond']), len(case['groups']), case['n_cond'], 0,
                 covariance=case['cov'])
    eng.set_confounds(Z)
    return spec, X, Y, Z, masks, dX.cpu().numpy(), dY.cpu().numpy(), gx.cpu().numpy(), gy.cpu().numpy()


def _same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _close(got, want, what, tol):
    err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    print('{}: max err relative to max(1, |value|) {:.3e}'.format(what, err))
    assert got.shape == want.shape and err <= tol, (what, err)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['C2', 'C4'])
def test_residual_kernel(name):
    eng = _engine()
    spec, X, Y, Z, masks, Xr, Yr, gx, gy = _bind(eng, name)
    allr = np.ones(len(X), dtype=bool)
    for got, raw, what in ((Xr, X, 'X'), (Yr, Y, 'Y')):
        err = np.abs(got - residualise(raw, Z, allr)) / np.abs(raw).max(axis=0)
        print('{} {}_r: max |error| / max |column| {:.3e}'.format(name, what, float(err.max())))
        assert err.max() <= 1e-12
    D = np.c_[np.ones(len(X)), Z - Z.mean(axis=0)]
    _close(gx, np.linalg.lstsq(D, X, rcond=None)[0][1:], name + ' slopes of X vs lstsq', RTOL)
    _close(gy, np.linalg.lstsq(D, Y, rcond=None)[0][1:], name + ' slopes of Y vs lstsq', RTOL)
    # rank deficient confounds: PLSX_ERR_ARG and nothing written
    from pypyls_amd.engine import PlsxError
    dX = eng._dev(X, np.float64)
    with pytest.raises(PlsxError, match=r'status -1: plsx_residualize: .*rank deficient'):
        eng.residualize(dX, np.c_[Z[:, :1], 2.0 * Z[:, :1]])
    assert np.array_equal(dX.cpu().numpy(), X)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(bx.CASES))
def test_fold_wise_crossval(name):
    exp = bx.expected(name)                              # (asserts the conditions before the device is looked at)
    eng = _engine()
    spec, X, Y, Z, masks = _bind(eng, name)[:5]
    r, r2, lv = eng.crossval_confound(masks, lv=True)
    cx.assert_entrywise(r, r2, exp['r'], exp['r2'], what=name + ' fold-wise')
    lx.compare(lv, exp['lv'], exp['relgap'], exp['live'], what=name + ' fold-wise lv_corr')
    # without d_lv: the same r, r2; run to run the same bits
    assert _same_bits(eng.crossval_confound(masks), (r, r2))
    assert _same_bits(eng.crossval_confound(masks, lv=True), (r, r2, lv))
    # ... and not the whole-cohort shortcut: the bound residuals through the entry without confounds miss by > TOL
    g_r, g_r2 = eng.crossval(masks)
    miss = float(np.abs(g_r - exp['r']).max())
    print('{}: whole-cohort residuals through plsx_crossval_batch miss the expectation by {:.3f}'.format(name, miss))
    assert miss >= 0.9 * bx.MIN_FOLD_GAP


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', bx.PERM_CASES)
def test_fold_wise_cv_perm(name):
    want_r, want_r2, _, _, wlv, relgap, live, _ = bx.null_expected(name)
    eng = _engine()
    spec, X, Y, Z, masks = _bind(eng, name)[:5]
    perms = bx.perms(name)
    P = perms.shape[1]
    r, r2, lv = eng.crossval_confound_perm(masks, perms, lv=True)
    cx.assert_entrywise(r, r2, want_r, want_r2, what=name + ' fold-wise null')
    lx.compare_mean(lv, wlv, relgap, live, what=name + ' fold-wise null lv_corr')
    # the identity column is the split mean of the observed entry, to the bit
    o_r, o_r2, o_lv = eng.crossval_confound(masks, lv=True)
    assert np.array_equal(r[:, 0], bcp.split_mean(o_r[:, None, :])[:, 0])
    assert np.array_equal(r2[:, 0], bcp.split_mean(o_r2[:, None, :])[:, 0])
    assert np.array_equal(lv[:, 0], bcp.split_mean(o_lv[:, None, :])[:, 0], equal_nan=True)
    # a repeat, and the permutations in pieces: the same bits
    assert _same_bits(eng.crossval_confound_perm(masks, perms, lv=True), (r, r2, lv))
    parts = [eng.crossval_confound_perm(masks, perms[:, a:b], lv=True) for a, b in ((0, 1), (1, P - 1), (P - 1, P))]
    assert _same_bits([np.hstack([p[k] for p in parts]) for k in range(3)], (r, r2, lv))
    assert _same_bits(eng.crossval_confound_perm(masks, perms), (r, r2))


# 4 ---------------------------------------------------------------------------------------------------------------
def test_grouping_does_not_change_the_bits():
    eng, small = _engine(), _engine(**SMALL)
    masks = _bind(eng, 'C2')[4]
    perms = bx.perms('C2')
    full = eng.crossval_confound(masks, lv=True)
    g_full = eng.crossval_confound_group()
    null_full = eng.crossval_confound_perm(masks, perms, lv=True)
    _bind(small, 'C2')
    one = small.crossval_confound(masks, lv=True)
    g_one = small.crossval_confound_group()
    null_one = small.crossval_confound_perm(masks, perms, lv=True)
    print('splits per group of fold copies: default {}, small budget {}'.format(g_full, g_one))
    assert g_one == 1 and g_full == masks.shape[1]
    assert small.crossval_confound_group() == 1
    assert _same_bits(one, full) and _same_bits(null_one, null_full)


# 5 ---------------------------------------------------------------------------------------------------------------
KW = dict(n_perm=16, n_boot=16, n_split=2, test_split=5, test_size=0.25, cv_perm=4, cv_lv=True, seed=11, verbose=False)


def _arrays(res, sections):
    out = {}
    for k in ('x_weights', 'y_weights', 'x_scores', 'y_scores', 'y_loadings', 'singvals', 'varexp'):
        out[k] = res[k]
    for sect in sections:
        for k, v in res[sect].items():
            if v is not None:
                out[sect + '.' + k] = v
    return out


def test_front_end(tmp_path):
    import pypyls_amd as pls
    case = bx.CASES['C2']
    eng = _engine()
    spec, X, Y, Z, _, Xr, Yr, gx, gy = _bind(eng, 'C2')
    kw = dict(KW, groups=case['groups'], n_cond=case['n_cond'])
    res = pls.behavioral_pls(X, Y, confounds=Z, **kw)
    plain = pls.behavioral_pls(Xr, Yr, **kw)
    assert 'confounds' not in plain.inputs and np.array_equal(res.inputs.confounds, Z)
    assert np.array_equal(res.inputs.X, X) and np.array_equal(res.inputs.Y, Y)
    # every non-CV array is that of the call without the keyword on the residuals, bit for bit; the draws are equal
    a, b = _arrays(plain, ('permres', 'bootres', 'splitres')), _arrays(res, ('permres', 'bootres', 'splitres'))
    assert set(a) == set(b) and 'permres.permsamples' in a and 'bootres.bootsamples' in a and 'splitres.ucorr' in a
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    cv = res.cvres
    for k in ('cvsamples', 'cvpermsamples'):
        assert np.array_equal(cv[k], plain.cvres[k]), k
    _close(res['confound_mean'], Z.mean(axis=0), 'confound_mean', 1e-12)
    assert np.array_equal(res['confound_x'], gx) and np.array_equal(res['confound_y'], gy)
    # cvres against the expectation on the drawn masks and permutations
    masks, perms = np.asarray(cv.cvsamples, dtype=bool), np.asarray(cv.cvpermsamples)
    S, T = Y.shape
    assert masks.shape == (S, 5) and perms.shape == (S, 4)
    ident = np.arange(S)[:, None]
    o_r, o_r2, o_lv, o_gap, o_live, info = bx.null('C2', ident, masks)
    n_r, n_r2, n_lv, n_gap, n_live, ninfo = bx.null('C2', perms, masks)
    assert max(i['kappa'] for i in info + ninfo) <= cx.KAPPA_MAX
    cx.assert_entrywise(cv.pearson_r, cv.r_squared, o_r[:, 0], o_r2[:, 0], what='front-end observed')
    lx.compare(cv.lv_corr, o_lv[:, 0], o_gap[:, 0], o_live[:, 0], what='front-end lv_corr')
    cx.assert_entrywise(cv.perm_pearson_r, cv.perm_r_squared, bcp.split_mean(n_r), bcp.split_mean(n_r2),
                        what='front-end null')
    lx.compare_mean(cv.perm_lv_corr, n_lv, n_gap, n_live, what='front-end null lv_corr')
    assert np.array_equal(cv.pearson_r_pvals, bcp.pvals(cv.perm_pearson_r, cv.pearson_r))
    assert np.array_equal(cv.r_squared_pvals, bcp.pvals(cv.perm_r_squared, cv.r_squared))
    # ... which the whole-cohort call misses
    assert np.abs(plain.cvres.pearson_r - o_r[:, 0]).max() > 1e3 * cx.TOL
    # a file round trip
    fname = str(tmp_path / 'res.hdf5')
    pls.save_results(fname, res)
    back = pls.load_results(fname)
    for k in ('confound_mean', 'confound_x', 'confound_y', 'singvals', 'x_weights'):
        assert np.array_equal(np.asarray(back[k]), np.asarray(res[k])), k
    for k in ('pearson_r', 'r_squared', 'lv_corr', 'perm_pearson_r', 'perm_r_squared', 'perm_lv_corr'):
        assert np.array_equal(np.asarray(back.cvres[k]), np.asarray(cv[k]), equal_nan=True), k
    assert np.array_equal(np.asarray(back.inputs.confounds), Z)
    # a team of two contexts on one GPU: every device residualises its own copy.  What the ranks shard and gather --
    # the permutations, the split-half nulls, the cross-validation and its null -- and the confound arrays have the bits
    # of the single context.  The bootstrap sums are added up across the ranks (a different order of summation than one
    # context's, with or without the keyword), so the bootstrap section is held to the bits of the SAME team call
    # without the keyword on (X_r, Y_r), as above.
    two = pls.behavioral_pls(X, Y, confounds=Z, device_ids=[0, 0], **kw)
    c = _arrays(two, ('permres', 'splitres', 'cvres'))
    d = _arrays(res, ('permres', 'splitres', 'cvres'))
    assert set(c) == set(d)
    for k in d:
        assert np.array_equal(c[k], d[k], equal_nan=True), k
    for k in ('confound_mean', 'confound_x', 'confound_y'):
        assert np.array_equal(two[k], res[k]), k
    plain_two = pls.behavioral_pls(Xr, Yr, device_ids=[0, 0], **kw)
    c, d = _arrays(two, ('bootres',)), _arrays(plain_two, ('bootres',))
    assert set(c) == set(d)
    for k in d:
        assert np.array_equal(c[k], d[k], equal_nan=True), k
    for k in ('x_weights_normed', 'x_weights_stderr'):
        _close(two.bootres[k], res.bootres[k], 'team vs one context: bootres.' + k, RTOL)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_without_the_keyword_a_golden_keeps_its_bits():
    import pypyls_amd as pls
    from conftest import load_golden, assert_close
    g = load_golden('bpls_2g2c_cv')
    kw = dict(groups=list(g['groups']), n_cond=int(g['n_cond']), verbose=False, seed=int(g['seed']),
              n_perm=g['ref_permres__perm_singval'].shape[1], n_boot=g['ref_bootres__bootsamples'].shape[1],
              test_split=g['cv_splits'].shape[1], test_size=float(g['test_size']))
    plain = pls.behavioral_pls(g['X'], g['Y'], **kw)
    none = pls.behavioral_pls(g['X'], g['Y'], confounds=None, **kw)
    for res in (plain, none):
        assert 'confounds' not in res.inputs
        assert all(res.get(k) is None for k in ('confound_mean', 'confound_x', 'confound_y'))
    a, b = _arrays(plain, ('permres', 'bootres', 'cvres')), _arrays(none, ('permres', 'bootres', 'cvres'))
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_array_equal(plain['bootres']['bootsamples'], g['ref_bootres__bootsamples'])
    assert_close(plain['cvres']['pearson_r'], g['ref_cvres__pearson_r'], RTOL, what='pearson_r')
    assert_close(plain['cvres']['r_squared'], g['ref_cvres__r_squared'], RTOL, what='r_squared')


# 7 ---------------------------------------------------------------------------------------------------------------
def test_abi_states():
    import torch
    from pypyls_amd.engine import PlsxError
    from pypyls_amd import resampling as rsmp
    eng = _engine()
    case = bx.CASES['C3']
    spec, X, Y, Z, masks = bx.problem('C3')
    perms = np.c_[np.arange(len(X)), np.random.RandomState(2).permutation(len(X))]
    cells = rsmp.cell_of_row(case['groups'], case['n_cond'])
    # a behavioural binding without confounds: PLSX_ERR_STATE
    eng.set_data(X, Y, cells, 1, 1, 0)
    with pytest.raises(PlsxError, match=r'status -4: plsx_crossval_confound_batch: no confounds are bound'):
        eng.crossval_confound(masks)
    with pytest.raises(PlsxError, match=r'status -4: plsx_crossval_confound_perm_batch: no confounds are bound'):
        eng.crossval_confound_perm(masks, perms)
    # plsx_set_data clears a binding of confounds
    eng.set_confounds(Z)
    eng.set_data(X, Y, cells, 1, 1, 0)
    with pytest.raises(PlsxError, match=r'status -4: plsx_crossval_confound_batch: no confounds are bound'):
        eng.crossval_confound(masks)
    # a regression binding: PLSX_ERR_ARG from all three
    eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), 2)
    with pytest.raises(PlsxError, match=r'status -1: plsx_set_confounds: .*behavioral PLS'):
        eng.set_confounds(Z)
    with pytest.raises(PlsxError, match=r'status -1: plsx_crossval_confound_batch: .*behavioral PLS'):
        eng.crossval_confound(masks)
    with pytest.raises(PlsxError, match=r'status -1: plsx_crossval_confound_perm_batch: .*behavioral PLS'):
        eng.crossval_confound_perm(masks, perms)
    # bad arguments at the C ABI
    _bind(eng, 'C3')
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    out = eng._empty((masks.shape[1], eng.T))
    lib, st = eng.lib, eng._stream()
    for args in ((None, 5, out.data_ptr(), out.data_ptr(), None), (dm.data_ptr(), 0, out.data_ptr(), out.data_ptr(), None),
                 (dm.data_ptr(), 5, None, out.data_ptr(), None), (dm.data_ptr(), 5, out.data_ptr(), None, None)):
        assert lib.plsx_crossval_confound_batch(eng.ctx, *args, st) == -1
        assert lib.plsx_last_error(eng.ctx).decode().startswith('plsx_crossval_confound_batch: bad arguments')
    # one binary confound that is constant on the training side of split 1: refused by index, nothing computed
    ind = np.zeros(len(X))
    ind[np.flatnonzero(~masks[:, 1])[:3]] = 1.0
    assert np.ptp(ind[masks[:, 1]]) == 0 and all(np.ptp(ind[masks[:, s]]) > 0 for s in (0, 2, 3, 4))
    eng.set_confounds(ind[:, None])
    with pytest.raises(PlsxError, match=r'status -1: plsx_crossval_confound_batch: .*rank deficient on the training rows '
                                        r'of split 1$'):
        eng.crossval_confound(masks)
    with pytest.raises(PlsxError, match=r'status -1: plsx_crossval_confound_perm_batch: .*training rows of split 1$'):
        eng.crossval_confound_perm(masks, perms)
    # a budget that holds no split: refused with the sizes
    tiny = _engine(scratch_gb=0.00025, min_batch=8)      # (the smallest budget of tests/test_gpu_crossval.py)
    _bind(tiny, 'C3')
    with pytest.raises(PlsxError, match=r'status -2: plsx_crossval_confound_batch: one split \(S = 65, B = 255: .* and its '
                                        r'fold copy of X\)'):
        tiny.crossval_confound(masks)
    # the contexts are usable afterwards
    exp = bx.expected('C3')
    _bind(eng, 'C3')
    r, r2 = eng.crossval_confound(masks)
    cx.assert_entrywise(r, r2, exp['r'], exp['r2'], what='C3 after the refusals')
    # ... the refused one too: its residual kernel still runs
    dY = tiny._dev(Y, np.float64)
    tiny.residualize(dY, Z, slopes=False)
    assert np.abs(dY.cpu().numpy() - bx.residuals('C3')[1]).max() <= 1e-12 * np.abs(Y).max()
