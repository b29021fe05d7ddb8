"""
The out-of-sample score correlation of the latent variables on the device (plsx_crossval_lv_batch: k_cv_lv after
k_cv_final; plsx_crossval_perm_lv_batch: k_cvp_lv after k_cvp_final, the mean over the splits) against the numpy
definition of tests/behavioral_cv_lv_expect.py, through Engine.crossval(lv=True), Engine.crossval_perm_lv and
behavioral_pls(cv_lv=).  GPU only.

Tolerance (behavioral_cv_lv_expect.compare): a live entry is compared iff its relative gap is >= 1e-6, within
crossval_expect.TOL * max(1, 1e-4 / relgap) absolute; at most 2 % of the live entries of a case are left out and never
LV 0, asserted on the expectation before the device is looked at.  tests/test_behavioral_cv_lv_host.py measures a
Gram-side solve on the host a factor 1000 inside it.
"""
import numpy as np
import pytest

from oracle import cpu_ref as ref
import crossval_expect as cx
import behavioral_cv_perm_expect as px
import behavioral_cv_lv_expect as lx

pytestmark = pytest.mark.gpu

SMALL = dict(scratch_gb=0.00025, min_batch=8)           # the budget of tests/test_gpu_crossval.py: one split a group here
_ENGINES = {}


def _engine(**options):
    from pypyls_amd.engine import Engine
    key = tuple(sorted(options.items()))
    if key not in _ENGINES:
        scratch = options.pop('scratch_gb', None)
        _ENGINES[key] = Engine(scratch_gb=scratch, options=options) if key else Engine()
    return _ENGINES[key]


def _bind(eng, name, X=None):
    """Bind the data of a case -> spec, X, Y, masks of crossval_expect."""
    from pypyls_amd import resampling as rsmp
    case = cx.CASES[name]
    spec, X0, Y, masks = cx.problem(name)
    eng.set_data(X0 if X is None else X, Y, rsmp.cell_of_row(case['groups'], case['n_cond']), len(case['groups']),
                 case['n_cond'], 0, covariance=case['cov'])
    return spec, X0, Y, masks


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('name', list(cx.CASES))
def test_feature_route_against_the_expectation(name):
    case = cx.CASES[name]
    want, relgap, live = lx.expected(name)
    lx.check_cap(relgap, live, name)
    eng = _engine()
    spec, X, Y, masks = _bind(eng, name)
    r, r2, lv = eng.crossval(masks, lv=True)
    assert lv.shape == want.shape == (eng.L, masks.shape[1])
    lx.compare(lv, want, relgap, live, what=name)
    # d_r / d_r2 are those of plsx_crossval_batch, bit for bit; run to run the same bits
    plain = eng.crossval(masks)
    assert np.array_equal(plain[0], r) and np.array_equal(plain[1], r2)
    assert _same(eng.crossval(masks, lv=True)[2], lv)
    if name in ('E10', 'E11_corr', 'E11_cov'):
        assert len(cx.slices_of(eng.Tp, case['T'], len(case['groups']) * case['n_cond'])) > 1     # the sliced layout
    if case['deficient']:
        assert not live.all() and np.isnan(lv[~live]).all()


@pytest.mark.parametrize('name', px.CASES)
def test_dual_route_against_the_expectation(name):
    want, relgap, live = lx.null_expected(name)
    L = want.shape[0]
    assert lx.check_cap(relgap.reshape(L, -1), live.reshape(L, -1), name + ' null') == 0      # the permuted cases leave out none
    eng = _engine()
    _bind(eng, name)
    _, _, _, masks, perms = px.problem(name)
    r, r2, mean, pairs = eng.crossval_perm_lv(masks, perms)
    assert pairs.shape == want.shape == (eng.L, perms.shape[1], masks.shape[1]) and mean.shape == pairs.shape[:2]
    lx.compare(pairs, want, relgap, live, what=name + ' pairs')
    assert _same(mean, lx.split_mean(pairs)), 'd_lv is the split-order mean of the pairs'
    lx.compare_mean(mean, want, relgap, live, what=name + ' means')
    plain = eng.crossval_perm(masks, perms)
    assert np.array_equal(plain[0], r) and np.array_equal(plain[1], r2)


def test_dual_route_with_a_cell_constant_feature():
    """A feature made bit-constant in one training cell of one split: scale 0, as the definition says."""
    name = 'E2'
    spec, X, Y, masks, perms = px.problem(name)
    mask = masks[:, 0]
    cell = spec.dummy[:, 1].astype(bool)
    Xk = X.copy()
    Xk[cell & mask, 3] = Xk[cell & mask, 3][0]
    assert px.cell_constant(spec, Xk, mask)[1, 3]
    eng = _engine()
    _bind(eng, name, X=Xk)
    _, _, mean, pairs = eng.crossval_perm_lv(masks, perms)
    want, relgap, live = lx.null(spec, Xk, Y, perms, masks)
    assert live.all() and np.isfinite(pairs).all()
    lx.compare(pairs, want, relgap, live, what=name + ' with a cell-constant feature')


@pytest.mark.parametrize('name', ['E2', 'E4', 'E7', 'E13'])
def test_the_two_kernels_agree_on_the_identity_permutation(name):
    want, relgap, live = lx.expected(name)
    eng = _engine()
    _bind(eng, name)
    _, X, _, masks, _ = px.problem(name)
    n = masks.shape[1]
    feature = eng.crossval(masks, lv=True)[2]
    _, _, mean, pairs = eng.crossval_perm_lv(masks, np.arange(len(X))[:, None])
    lx.compare(pairs[:, 0, :], feature, relgap[:, :n], live[:, :n], what=name + ' dual route vs feature route')


def test_same_bits_however_the_work_is_cut():
    name = 'E2'
    eng = _engine()
    _bind(eng, name)
    _, _, _, masks, perms = px.problem(name)
    full = eng.crossval_perm_lv(masks, perms)
    # the permutations cut into two calls: the pairs and the means of each piece are the rows of the whole
    P = perms.shape[1]
    a, b = eng.crossval_perm_lv(masks, perms[:, :2]), eng.crossval_perm_lv(masks, perms[:, 2:])
    assert P > 3 and _same(np.concatenate([a[3], b[3]], axis=1), full[3]) and _same(np.hstack([a[2], b[2]]), full[2])
    # splits and permutations in the groups of the smallest budget, on both routes
    small = _engine(**SMALL)
    _bind(small, name)
    got = small.crossval_perm_lv(masks, perms)
    for x, y in zip(got, full):
        assert _same(x, y)
    all_masks = cx.problem(name)[3]
    assert _same(small.crossval(all_masks, lv=True)[2], eng.crossval(all_masks, lv=True)[2])


def test_same_bits_with_a_team_of_two_contexts_on_one_gpu():
    """E2 through the public call: two team contexts on one GPU (the pattern of tests/test_gpu_team.py) shard the splits
    of the observed leg and the permutations of the null, and return the bits of one device."""
    import pypyls_amd as pls
    case = cx.CASES['E2']
    _, X, Y, _, perms = px.problem('E2')
    kw = dict(groups=case['groups'], n_cond=case['n_cond'], n_perm=0, n_boot=0, test_split=5, test_size=cx.TEST_SIZE,
              seed=5, verbose=False, cv_perm=perms.shape[1], cvpermsamples=perms, cv_lv=True)
    one = pls.behavioral_pls(X, Y, **kw)
    two = pls.behavioral_pls(X, Y, device_ids=[0, 0], **kw)
    assert one.cvres.lv_corr.shape == (12, 5) and one.cvres.perm_lv_corr.shape == (12, perms.shape[1])
    assert np.isfinite(one.cvres.lv_corr).all() and np.isfinite(one.cvres.perm_lv_corr).all()
    for k in ('pearson_r', 'r_squared', 'perm_pearson_r', 'perm_r_squared', 'lv_corr', 'perm_lv_corr', 'lv_corr_pvals'):
        assert _same(two.cvres[k], one.cvres[k]), k


def test_bad_arguments_name_the_entries():
    import torch
    eng = _engine()
    _bind(eng, 'E2')
    _, _, _, masks, perms = px.problem('E2')
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    di = eng.rows_tensor(np.ascontiguousarray(perms.T))
    out = eng._empty((max(perms.shape[1], masks.shape[1]), max(eng.T, eng.L)))
    lib, st, o = eng.lib, eng._stream(), out.data_ptr()
    n, m = dm.shape[0], di.shape[0]
    assert lib.plsx_crossval_lv_batch(eng.ctx, dm.data_ptr(), n, o, o, None, st) == -1
    assert lib.plsx_last_error(eng.ctx).decode().startswith('plsx_crossval_lv_batch: bad arguments')
    assert lib.plsx_crossval_perm_lv_batch(eng.ctx, dm.data_ptr(), n, di.data_ptr(), m, o, o, None, None, st) == -1
    assert lib.plsx_last_error(eng.ctx).decode().startswith('plsx_crossval_perm_lv_batch: bad arguments')
    # d_lv_pairs may be NULL: the means are the same bits
    mean = eng._empty((m, eng.L))
    r, r2 = eng._empty((m, eng.T)), eng._empty((m, eng.T))
    eng.crossval_perm_into(dm, di, r, r2, mean)
    eng.sync()
    assert _same(mean.cpu().numpy().T, eng.crossval_perm_lv(masks, perms)[2])


# ---------------------------------------------------------------------------
# front-end
# ---------------------------------------------------------------------------

def _design():
    rs = np.random.RandomState(3)
    groups, n_cond, T = [10, 12], 2, 3
    S = sum(groups) * n_cond
    X = rs.randn(S, 70) + 2.0 * rs.rand(1, 70)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    return X, Y, groups, n_cond


KW = dict(n_perm=6, n_boot=5, n_split=0, test_split=5, test_size=0.25, seed=11, verbose=False)


def _arrays(res):
    out = {}
    for k in ('x_weights', 'y_weights', 'x_scores', 'y_scores', 'y_loadings', 'singvals', 'varexp'):
        out[k] = res[k]
    for sect in ('permres', 'bootres', 'cvres'):
        for k, v in res[sect].items():
            if v is not None:
                out[sect + '.' + k] = v
    return out


def test_front_end_against_the_expectation_and_the_unchanged_rest():
    import pypyls_amd as pls
    X, Y, groups, n_cond = _design()
    kw = dict(KW, groups=groups, n_cond=n_cond)
    plain = pls.behavioral_pls(X, Y, cv_perm=4, **kw)
    res = pls.behavioral_pls(X, Y, cv_perm=4, cv_lv=True, **kw)
    assert 'cv_lv' not in plain.inputs and res.inputs.cv_lv is True
    for k in ('lv_corr', 'perm_lv_corr', 'lv_corr_pvals'):
        assert k not in plain.cvres, k
    # every key the call had before keeps its bits, the resampling arrays included
    a, b = _arrays(plain), _arrays(res)
    assert set(a) <= set(b) and set(b) - set(a) == {'cvres.lv_corr', 'cvres.perm_lv_corr', 'cvres.lv_corr_pvals'}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    cv = res.cvres
    L = min(len(groups) * n_cond * Y.shape[1], X.shape[1])
    assert cv.lv_corr.shape == (L, 5) and cv.perm_lv_corr.shape == (L, 4) and cv.lv_corr_pvals.shape == (L,)
    spec = ref.Spec('behavioral', groups, n_cond, False)
    want, relgap, live = lx.crossval_lv(spec, X, Y, cv.cvsamples)
    lx.compare(cv.lv_corr, want, relgap, live, what='front-end observed')
    wantn, relgapn, liven = lx.null(spec, X, Y, cv.cvpermsamples, cv.cvsamples)
    lx.compare_mean(cv.perm_lv_corr, wantn, relgapn, liven, what='front-end null')
    assert _same(cv.lv_corr_pvals, lx.pvals(cv.perm_lv_corr, cv.lv_corr))
    # without cv_perm: the observed values alone, the same bits
    alone = pls.behavioral_pls(X, Y, cv_lv=True, **kw)
    assert _same(alone.cvres.lv_corr, cv.lv_corr) and 'perm_lv_corr' not in alone.cvres
    # cv_lv = 2: the first two rows
    two = pls.behavioral_pls(X, Y, cv_perm=4, cv_lv=2, **kw)
    assert two.inputs.cv_lv == 2
    for k in ('lv_corr', 'perm_lv_corr', 'lv_corr_pvals'):
        assert _same(two.cvres[k], cv[k][:2]), k
    # a team of two contexts on one GPU returns the bits of the single context
    team = pls.behavioral_pls(X, Y, cv_perm=4, cv_lv=True, device_ids=[0, 0], **kw)
    for k in ('pearson_r', 'r_squared', 'perm_pearson_r', 'perm_r_squared', 'lv_corr', 'perm_lv_corr', 'lv_corr_pvals'):
        assert _same(team.cvres[k], cv[k]), k


def test_results_round_trip_through_a_file(tmp_path):
    import pypyls_amd as pls
    X, Y, groups, n_cond = _design()
    res = pls.behavioral_pls(X, Y, cv_perm=3, cv_lv=2, **dict(KW, groups=groups, n_cond=n_cond, n_perm=0, n_boot=0))
    fname = str(tmp_path / 'res.hdf5')
    pls.save_results(fname, res)
    back = pls.load_results(fname)
    for k in ('lv_corr', 'perm_lv_corr', 'lv_corr_pvals'):
        assert _same(np.asarray(back.cvres[k]), np.asarray(res.cvres[k])), k
    assert int(back.inputs.cv_lv) == 2
