"""
The permutation null of the behavioural cross-validation on the device (plsx_crossval_perm_batch: k_cvp_moments,
k_cvp_gram + k_cvp_reduce, k_cvp_build_A, the products W' = A M^T and G = W' A^T, the small solver returning V and d,
k_cvp_final, the mean over the splits) against the numpy definition of tests/behavioral_cv_perm_expect.py, through
Engine.crossval_perm and behavioral_pls(cv_perm=).  GPU only.

Tolerance: crossval_expect.TOL per ENTRY of perm_pearson_r and perm_r_squared.  The dual route solves on a Gram matrix
exactly as plsx_crossval_batch does (error ~ eps * kappa^2), and tests/test_behavioral_cv_perm_host.py asserts, without
a GPU, kappa <= KAPPA_MAX for every (permutation, split) of every case: eps * kappa^2 <= 2.3e-10.
"""
import numpy as np
import pytest

from oracle import cpu_ref as ref
import crossval_expect as cx
import behavioral_cv_perm_expect as px

pytestmark = pytest.mark.gpu

SMALL = dict(scratch_gb=0.00025, min_batch=8)           # the budget of tests/test_gpu_crossval.py: one split a group here
_ENGINES = {}


def _engine(**options):
    from pypyls_amd.engine import Engine
    if not options:
        return Engine()
    key = tuple(sorted(options.items()))
    if key not in _ENGINES:
        scratch = options.pop('scratch_gb', None)
        _ENGINES[key] = Engine(scratch_gb=scratch, options=options)
    return _ENGINES[key]


def _bind(eng, name, X=None):
    from pypyls_amd import resampling as rsmp
    case = cx.CASES[name]
    spec, X0, Y, masks, perms = px.problem(name)
    eng.set_data(X0 if X is None else X, Y, rsmp.cell_of_row(case['groups'], case['n_cond']), len(case['groups']),
                 case['n_cond'], 0, covariance=case['cov'])
    return spec, X0, Y, masks, perms


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('name', px.CASES)
def test_case_against_the_expectation(name):
    case = cx.CASES[name]
    eng = _engine()
    spec, X, Y, masks, perms = _bind(eng, name)
    T, P = case['T'], perms.shape[1]
    want_r, want_r2 = px.expected(name)[:2]
    r, r2 = eng.crossval_perm(masks, perms)
    assert r.shape == r2.shape == (T, P)
    cx.assert_entrywise(r, r2, want_r, want_r2, what=name)
    # run to run: the same call, the same bits
    assert _same_bits(eng.crossval_perm(masks, perms), (r, r2))
    # the edge the case is there for
    if name in ('E6_65', 'E6_127'):
        assert case['S'] % 64 in (1, 63)
    if name.startswith('E5'):
        assert case['B'] % 128 == 1 and case['B'] % 32 != 0 and eng.Tp == T
    if name == 'E8':
        assert eng.Tp > case['B'] == eng.L and case['B'] < 16
    if case['deficient']:
        assert all(i['n_live'] < i['L'] for i in px.expected(name)[4])


@pytest.mark.parametrize('name', ['E2', 'E4', 'E13'])
def test_identity_permutation_is_the_split_mean_of_crossval(name):
    eng = _engine()
    spec, X, Y, masks, _ = _bind(eng, name)
    obs_r, obs_r2 = eng.crossval(masks)
    r, r2 = eng.crossval_perm(masks, np.arange(len(X))[:, None])
    cx.assert_entrywise(r, r2, px.split_mean(obs_r[:, None, :]), px.split_mean(obs_r2[:, None, :]),
                        what=name + ' identity permutation vs crossval')


@pytest.mark.parametrize('name', ['E1', 'E2', 'E6_127'])
def test_same_bits_however_the_call_is_cut(name):
    eng = _engine()
    spec, X, Y, masks, perms = _bind(eng, name)
    full = eng.crossval_perm(masks, perms)
    # permutations in pieces
    P = perms.shape[1]
    parts = [eng.crossval_perm(masks, perms[:, a:b]) for a, b in ((0, 1), (1, P - 1), (P - 1, P))]
    assert _same_bits((np.hstack([p[0] for p in parts]), np.hstack([p[1] for p in parts])), full)
    if name == 'E6_127':
        return                                           # (one split of S = 127 does not fit the smallest budget)
    # splits and permutations in the groups of the smallest budget
    small = _engine(**SMALL)
    _bind(small, name)
    assert _same_bits(small.crossval_perm(masks, perms), full)


@pytest.mark.parametrize('name', ['E2', 'E4'])
def test_cell_constant_feature_has_scale_zero(name):
    """A feature made bit-constant in one training cell of one split: finite, and the definition with scale 0."""
    eng = _engine()
    spec, X, Y, masks, perms = px.problem(name)
    mask = masks[:, 0]
    cell = spec.dummy[:, 1].astype(bool)
    Xk = X.copy()
    Xk[cell & mask, 3] = Xk[cell & mask, 3][0]
    const = [px.cell_constant(spec, Xk, masks[:, s]) for s in range(masks.shape[1])]
    assert const[0][1, 3] and const[0].sum() == 1
    _bind(eng, name, X=Xk)
    r, r2 = eng.crossval_perm(masks, perms)
    assert np.isfinite(r).all() and np.isfinite(r2).all()
    wr, wr2, _ = px.null(spec, Xk, Y, perms, masks)
    cx.assert_entrywise(r, r2, px.split_mean(wr), px.split_mean(wr2), what=name + ' with a cell-constant feature')


@pytest.mark.parametrize('name', ['E4', 'E2'])
def test_crossval_perm_leaves_the_context_as_it_found_it(name):
    """Permutations, bootstraps, split-half, the cross-covariance and crossval give the same bits after a
    crossval_perm call as before it (the pattern of test_crossval_leaves_the_context_as_it_found_it)."""
    from pypyls_amd import resampling as rsmp
    case = cx.CASES[name]
    eng = _engine()
    spec, X, Y, masks, cvperms = _bind(eng, name)
    U, d, V = ref.decompose(spec, X, Y)
    eng.set_original(U, np.diag(d), V)
    perms = rsmp.gen_permsamp(case['groups'], case['n_cond'], 3, seed=1)
    boots = rsmp.gen_bootsamp(case['groups'], case['n_cond'], 3, seed=2)
    halves = rsmp.gen_splits(case['groups'], case['n_cond'], 2, seed=3)

    def legs():
        usum, usq, dist = eng.boot(boots)
        uc, vc = eng.split_half(halves)
        r, r2 = eng.crossval(masks)
        return [eng.perm(perms), usum.cpu().numpy(), usq.cpu().numpy(), dist, uc, vc, eng.crosscov(ysrc=perms), r, r2], \
            eng.last_timing()['resamples_per_group']

    before, npg_before = legs()
    r, r2 = eng.crossval_perm(masks, cvperms)
    want_r, want_r2 = px.expected(name)[:2]
    cx.assert_entrywise(r, r2, want_r, want_r2, what=name + ' between the other legs')
    after, npg_after = legs()
    for what, a, b in zip(('perm', 'u_sum', 'u_square', 'distrib', 'ucorr', 'vcorr', 'crosscov', 'cv r', 'cv r2'),
                          before, after):
        assert np.all(np.isfinite(a)), what
        assert np.array_equal(a, b), what
    assert npg_after == npg_before


def test_refusals_name_the_entry_and_leave_the_context_alive():
    from pypyls_amd.engine import PlsxError
    from pypyls_amd import resampling as rsmp
    rs = np.random.RandomState(0)
    eng = _engine()
    # a mean-centred binding
    eng.set_data(rs.randn(24, 30), None, rsmp.cell_of_row([6, 6], 2), 2, 2, 1)
    perms = np.stack([rs.permutation(24) for _ in range(2)], axis=1)
    masks = rs.rand(24, 2) < 0.7
    with pytest.raises(PlsxError, match=r'status -1: plsx_crossval_perm_batch: .*behavioral PLS'):
        eng.crossval_perm(masks, perms)
    # contrasts set
    spec, X, Y, masks, perms = _bind(eng, 'E2')
    V = np.linalg.qr(rs.randn(eng.Tp, 2))[0]
    eng.set_contrasts(V)
    with pytest.raises(PlsxError, match=r'status -2: plsx_crossval_perm_batch: .*contrasts are set'):
        eng.crossval_perm(masks, perms)
    eng.set_contrasts(None)
    # bad arguments, at the C ABI
    import torch
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    di = eng.rows_tensor(np.ascontiguousarray(perms.T))
    out = eng._empty((perms.shape[1], eng.T))
    lib, st = eng.lib, eng._stream()
    n, m = dm.shape[0], di.shape[0]
    for args in ((None, n, di.data_ptr(), m, out.data_ptr(), out.data_ptr()),
                 (dm.data_ptr(), n, None, m, out.data_ptr(), out.data_ptr()),
                 (dm.data_ptr(), n, di.data_ptr(), m, None, out.data_ptr()),
                 (dm.data_ptr(), n, di.data_ptr(), m, out.data_ptr(), None),
                 (dm.data_ptr(), 0, di.data_ptr(), m, out.data_ptr(), out.data_ptr()),
                 (dm.data_ptr(), n, di.data_ptr(), 0, out.data_ptr(), out.data_ptr())):
        assert lib.plsx_crossval_perm_batch(eng.ctx, *args, st) == -1
        assert lib.plsx_last_error(eng.ctx).decode().startswith('plsx_crossval_perm_batch: bad arguments')
    # a split that does not fit the scratch budget: refused with the sizes, the context still usable
    small = _engine(**SMALL)
    _, _, _, m3, p3 = _bind(small, 'E3')
    with pytest.raises(PlsxError, match=r'status -2: plsx_crossval_perm_batch: one split \(S = 320, B = 130'):
        small.crossval_perm(m3, p3)
    _, _, _, m1, p1 = _bind(small, 'E1')
    r, r2 = small.crossval_perm(m1, p1)
    cx.assert_entrywise(r, r2, *px.expected('E1')[:2], what='E1 after a refusal')
    # ... and so is the context of the refusals above
    r, r2 = eng.crossval_perm(masks, perms)
    cx.assert_entrywise(r, r2, *px.expected('E2')[:2], what='E2 after the refusals')


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
    plain = pls.behavioral_pls(X, Y, **kw)
    res = pls.behavioral_pls(X, Y, cv_perm=4, **kw)
    assert 'cv_perm' not in plain.inputs and res.inputs.cv_perm == 4
    assert 'perm_pearson_r' not in plain.cvres and 'cvsamples' not in plain.cvres
    # every array of the same seeded call without the keyword keeps its bits
    a, b = _arrays(plain), _arrays(res)
    assert set(a) <= set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    cv = res.cvres
    S, T = Y.shape
    assert cv.cvpermsamples.shape == (S, 4) and cv.cvsamples.shape == (S, 5) and cv.cvsamples.dtype == bool
    assert np.array_equal(np.sort(cv.cvpermsamples, axis=0), np.broadcast_to(np.arange(S)[:, None], (S, 4)))
    assert cv.perm_pearson_r.shape == cv.perm_r_squared.shape == (T, 4)
    spec = ref.Spec('behavioral', groups, n_cond, False)
    obs_r, obs_r2, _ = cx.crossval(spec, X, Y, cv.cvsamples)
    cx.assert_entrywise(cv.pearson_r, cv.r_squared, obs_r, obs_r2, what='front-end observed')
    wr, wr2, info = px.null(spec, X, Y, cv.cvpermsamples, cv.cvsamples)
    assert max(i['kappa'] for i in info) <= cx.KAPPA_MAX
    cx.assert_entrywise(cv.perm_pearson_r, cv.perm_r_squared, px.split_mean(wr), px.split_mean(wr2), what='front-end null')
    assert np.array_equal(cv.pearson_r_pvals, px.pvals(cv.perm_pearson_r, cv.pearson_r))
    assert np.array_equal(cv.r_squared_pvals, px.pvals(cv.perm_r_squared, cv.r_squared))
    # given cvpermsamples reproduces the drawn run
    again = pls.behavioral_pls(X, Y, cv_perm=4, cvpermsamples=cv.cvpermsamples, **kw)
    for k in ('perm_pearson_r', 'perm_r_squared', 'pearson_r_pvals', 'r_squared_pvals', 'cvpermsamples', 'cvsamples'):
        assert np.array_equal(again.cvres[k], cv[k]), k
    # a team of two contexts on one GPU shards the permutations and returns the bits of the single context
    two = pls.behavioral_pls(X, Y, cv_perm=4, device_ids=[0, 0], **kw)
    for k in ('pearson_r', 'r_squared', 'perm_pearson_r', 'perm_r_squared', 'pearson_r_pvals', 'r_squared_pvals',
              'cvpermsamples', 'cvsamples'):
        assert np.array_equal(two.cvres[k], cv[k]), k
    three = pls.behavioral_pls(X, Y, cv_perm=2, device_ids=[0, 0, 0], cvpermsamples=cv.cvpermsamples[:, :2], **kw)
    assert np.array_equal(three.cvres.perm_pearson_r, cv.perm_pearson_r[:, :2])      # (a rank with an empty shard)


def test_results_round_trip_through_a_file(tmp_path):
    import pypyls_amd as pls
    X, Y, groups, n_cond = _design()
    res = pls.behavioral_pls(X, Y, cv_perm=3, **dict(KW, groups=groups, n_cond=n_cond, n_perm=0, n_boot=0))
    fname = str(tmp_path / 'res.hdf5')
    pls.save_results(fname, res)
    back = pls.load_results(fname)
    for k in ('pearson_r', 'r_squared', 'perm_pearson_r', 'perm_r_squared', 'pearson_r_pvals', 'r_squared_pvals',
              'cvpermsamples', 'cvsamples'):
        assert np.array_equal(np.asarray(back.cvres[k]), np.asarray(res.cvres[k])), k
    assert int(back.inputs.cv_perm) == 3
