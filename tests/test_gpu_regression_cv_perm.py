"""pls_regression(cv_perm=P) on the device (plsx_simpls_crossval_perm_batch: k_sd_cvp_expand, k_sd_cv_score<., true>,
k_sd_cvp_reduce): against the reference fixtures, the oracle, the two routes of the solver, solver batches, teams and
persistence.

Tolerance: the project's parity bar for regression (tests/test_gpu_regression_cv.py), absolute on r, relative to
max(1, |value|) on r^2 and mse.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from conftest import load_golden
from regression_cv_perm_expect import cv_perm_expected, null_errs, abs_err, rel_err

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROUTES = 1e-9
NULLS = ('perm_pearson_r', 'perm_r_squared', 'perm_mse')
PVALS = ('pearson_r_pvals', 'r_squared_pvals', 'mse_pvals')


def _global_engine(**kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1}, **kw)


def _design(S, B, T, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    return X, rs.randn(S, T) + 0.5 * X[:, :T], rs


def _check_null(cv, want, what, tol=RTOL):
    errs = null_errs(cv['perm_pearson_r'], cv['perm_r_squared'], cv['perm_mse'], want['null'])
    print('{}: max err of the null r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}'.format(what, **errs))
    assert max(errs.values()) <= tol, (what, errs)
    return errs


def _check_pvals(cv, want, what):
    for key, name in (('r', 'pearson_r_pvals'), ('r2', 'r_squared_pvals'), ('mse', 'mse_pvals')):
        diff = int(np.sum(cv[name] != want[key]))
        print('{}: {} differing from the expected in {} of {} entries; range {:.4f} .. {:.4f}'
              .format(what, name, diff, want[key].size, float(np.min(cv[name])), float(np.max(cv[name]))))
        assert cv[name].shape == want[key].shape and diff == 0, (what, name)


def _same_bits(a, b, what, keys=NULLS + PVALS):
    for key in keys:
        same = np.array_equal(a[key], b[key], equal_nan=True)
        print('{}: {} bit-identical: {}'.format(what, key, same))
        assert same, (what, key)


@pytest.mark.parametrize('tag', ['a', 'b', 'nan'])
def test_goldens_on_both_routes(tag):
    import pypyls_amd as pls
    g, f = load_golden('simpls_cv_' + tag), load_golden('simpls_cv_perm_' + tag)
    k, masks, perms = int(g['n_components']), g['cvsamples'], f['cvpermsamples']
    T, P = g['Y'].shape[1], perms.shape[1]
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=masks.shape[1], cvsamples=masks, cv_perm=P,
              cvpermsamples=perms, seed=1, verbose=False)
    want = dict(null=dict(r=f['ref_perm_r'], r2=f['ref_perm_r2'], mse=f['ref_perm_mse']))
    pv = dict(r=f['pvals_r'], r2=f['pvals_r2'], mse=f['pvals_mse'])
    chip = pls.pls_regression(g['X'], g['Y'], **kw)
    _check_null(chip.cvres, want, 'simpls_cv_perm_{} on-chip vs reference'.format(tag))
    _check_pvals(chip.cvres, pv, 'simpls_cv_perm_{} on-chip'.format(tag))
    eng = _global_engine()
    try:
        glob_ = pls.pls_regression(g['X'], g['Y'], _engine=eng, **kw)
    finally:
        eng.close()
    _check_null(glob_.cvres, want, 'simpls_cv_perm_{} global vs reference'.format(tag))
    _check_pvals(glob_.cvres, pv, 'simpls_cv_perm_{} global'.format(tag))
    routes = null_errs(chip.cvres.perm_pearson_r, chip.cvres.perm_r_squared, chip.cvres.perm_mse,
                       dict(r=glob_.cvres.perm_pearson_r, r2=glob_.cvres.perm_r_squared, mse=glob_.cvres.perm_mse))
    print('simpls_cv_perm_{} on-chip vs global: {}'.format(tag, routes))
    assert max(routes.values()) <= ROUTES
    cv = chip.cvres
    assert cv.perm_pearson_r.shape == (T, k, P) and cv.perm_r_squared.shape == (T, k, P) and cv.perm_mse.shape == (k + 1, P)
    assert cv.pearson_r_pvals.shape == (T, k) and cv.r_squared_pvals.shape == (T, k) and cv.mse_pvals.shape == (k + 1,)
    for key in NULLS + PVALS:
        assert cv[key].dtype == np.float64, key
    assert np.array_equal(cv.cvpermsamples, perms) and np.issubdtype(cv.cvpermsamples.dtype, np.integer)
    assert chip.inputs.cv_perm == P


def test_identity_permutation_gives_the_observed_split_means():
    """The same arithmetic apart from the summation order of at most 8 terms."""
    import pypyls_amd as pls
    X, Y, rs = _design(110, 260, 6, 13)
    X[[7, 90]] = np.nan
    Y[33] = np.nan
    res = pls.pls_regression(X, Y, n_components=5, n_perm=0, n_boot=0, test_split=8, seed=5, cv_perm=1,
                             cvpermsamples=np.arange(110)[:, None], verbose=False)
    cv = res.cvres
    errs = dict(r=abs_err(cv.perm_pearson_r[..., 0], cv.pearson_r_ncomp.mean(axis=-1)),
                r2=rel_err(cv.perm_r_squared[..., 0], cv.r_squared_ncomp.mean(axis=-1)),
                mse=rel_err(cv.perm_mse[..., 0], cv.mse.mean(axis=-1)))
    print('identity permutation vs the observed split-means: {}'.format(errs))
    assert max(errs.values()) <= 1e-12, errs


def test_past_the_reference_pin_t20_k15():
    """T = 20, k = 15, 16 drawn splits, 6 drawn permutations against the oracle; the drawn permutations are the next
    draw of the call's generator after the split masks."""
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    S, B, T, k = 300, 2000, 20, 15
    X, Y, rs = _design(S, B, T, 7)
    res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, test_split=16, test_size=0.25, seed=99,
                             cv_perm=6, verbose=False)
    masks, perms = res.cvres.cvsamples, res.cvres.cvpermsamples
    assert perms.shape == (S, 6) and np.issubdtype(perms.dtype, np.integer)
    rstate = np.random.RandomState(99)
    for _ in range(k):
        rstate.normal(size=(min(B, T), 11))                  # what the call draws before the splits
    assert np.array_equal(masks, rsmp.gen_splits([S], 1, 16, seed=rstate, test_size=0.25))
    assert np.array_equal(perms, rsmp.gen_permsamp([S], 1, 6, seed=rstate, verbose=False))
    want = cv_perm_expected(X, Y, masks, perms, k)
    _check_null(res.cvres, want, 'T=20 k=15 vs oracle')
    obs = dict(r=abs_err(res.cvres.pearson_r_ncomp.mean(axis=-1), want['obs']['r']),
               r2=rel_err(res.cvres.r_squared_ncomp.mean(axis=-1), want['obs']['r2']),
               mse=rel_err(res.cvres.mse.mean(axis=-1), want['obs']['mse']))
    print('T=20 k=15 observed split-means vs oracle: {}'.format(obs))
    assert max(obs.values()) <= RTOL
    assert res.cvres.pearson_r_pvals.min() >= 1 / 7 - 1e-15 and res.cvres.pearson_r_pvals.max() <= 1.0


def test_missing_rows_with_drawn_splits():
    """Rows of X and of Y that are NaN throughout: position p is usable iff okx[p] and oky[perm[p]], so the usable test
    rows differ from permutation to permutation (get_mask(X, Y[perm]) in the oracle)."""
    import pypyls_amd as pls
    X, Y, rs = _design(90, 140, 4, 23)
    X[[5, 50, 77]] = np.nan
    Y[[20, 61]] = np.nan
    res = pls.pls_regression(X, Y, n_components=4, n_perm=0, n_boot=0, test_split=9, test_size=0.3, seed=6, cv_perm=7,
                             verbose=False)
    masks, perms = res.cvres.cvsamples, res.cvres.cvpermsamples
    assert masks.shape == (90, 9) and perms.shape == (90, 7)
    n_te = [(~masks & (~np.isnan(X[:, 0]) & ~np.isnan(Y[perms[:, p], 0]))[:, None]).sum(axis=0) for p in range(7)]
    print('usable test rows per (permutation, split): {}'.format(np.array(n_te).tolist()))
    assert len({tuple(v) for v in n_te}) > 1                 # n_test really belongs to the pair
    want = cv_perm_expected(X, Y, masks, perms, 4)
    _check_null(res.cvres, want, 'drawn splits with NaN rows vs oracle')
    assert np.isfinite(res.cvres.perm_mse).all()


def test_3d_y_median():
    """3-D Y: the rows of the aggregated Y are permuted."""
    import pypyls_amd as pls
    S, B, T, C, k = 70, 120, 4, 5, 5
    rs = np.random.RandomState(21)
    X = rs.randn(S, B)
    Y = rs.randn(S, T, C) + 0.5 * X[:, :T, None]
    X[[3, 40]] = np.nan
    Y[11] = np.nan
    res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, aggfunc='median', test_split=6, seed=2, cv_perm=5,
                             verbose=False)
    want = cv_perm_expected(X, np.median(Y, axis=-1), res.cvres.cvsamples, res.cvres.cvpermsamples, k)
    _check_null(res.cvres, want, '3-D Y median with NaN rows vs oracle')


def test_solver_batches_do_not_change_the_bits():
    """7 splits x 9 permutations = 63 fits at S = 1000, T = 6, k = 5: a fit holds 49 142 doubles of solver state plus
    80 000 bytes of dual weights and scores, 5000 of sources and mask and 776 of scores -- 0.48 MB.  Half of a 0.02 GB
    budget takes 22 of them, so the batches are 22 + 22 + 19 and permutations 3 and 6 straddle two batches each."""
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, B, T, k = 1000, 200, 6, 5
    X, Y, rs = _design(S, B, T, 29)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=7, seed=12, cv_perm=9, verbose=False)
    one = pls.pls_regression(X, Y, **kw)
    batches = {}
    for name, gb in (('default', None), ('0.02 GB', 0.02)):
        eng = Engine(scratch_gb=gb) if gb else Engine()
        try:
            eng.set_timing(True)
            got = pls.pls_regression(X, Y, _engine=eng, **kw)
            # (two timed brackets per solver batch of the permuted fits -- expansion; scoring and reduction -- and one
            # for the single batch of the 7 observed splits)
            batches[name] = (eng.kernel_timing()['k_sd_cv_score'][1] - 1) // 2
        finally:
            eng.close()
        print('scratch {}: {} solver batches of permuted fits'.format(name, batches[name]))
        _same_bits(one.cvres, got.cvres, 'scratch {} vs the default engine'.format(name))
    assert batches['default'] == 1 and batches['0.02 GB'] == 3
    _check_null(one.cvres, cv_perm_expected(X, Y, one.cvres.cvsamples, one.cvres.cvpermsamples, k), 'S=1000 vs oracle')


def test_one_call_of_2560_fits_takes_the_large_batch_instantiations():
    """Above 2048 fits per batch the solver and k_sd_cv_score<8, true> run their three-waves-per-SIMD instantiations: 8
    distinct permutations under 8 splits at c5's solver shape class (S = 1000, T = 20, k = 15), the permutations
    replicated to 320 rows: ONE call, ONE solver batch of 2560 fits."""
    import torch
    from pypyls_amd.engine import Engine
    from pypyls_amd import resampling as rsmp
    S, B, T, k = 1000, 2000, 20, 15
    X, Y, rs = _design(S, B, T, 3)
    m, nd, n = 320, 8, 8
    masks = rsmp.gen_splits([S], 1, n, seed=77, test_size=0.25)
    perms = rsmp.gen_permsamp([S], 1, nd, seed=78, verbose=False)
    which = np.arange(m) % nd
    which[[0, 1, m - 2, m - 1]] = [5, 2, 7, 0]
    eng = Engine()
    try:
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        di = eng.rows_tensor(perms[:, which].T)
        r, r2, mse = eng._zeros((m, k, T)), eng._zeros((m, k, T)), eng._zeros((m, k + 1))
        eng.set_timing(True)
        eng.simpls_crossval_perm_into(dm, di, r, r2, mse)
        eng.sync()
        launches = eng.kernel_timing()['k_sd_cv_score'][1]
        r, r2, mse = r.cpu().numpy(), r2.cpu().numpy(), mse.cpu().numpy()
    finally:
        eng.close()
    print('timed brackets of the cross-validation class: {}'.format(launches))
    assert launches == 2                                     # one solver batch
    for d in range(nd):
        rows = np.flatnonzero(which == d)
        for name, arr in (('r', r), ('r2', r2), ('mse', mse)):
            same = all(np.array_equal(arr[rows[0]], arr[i]) for i in rows[1:])
            assert same, (d, name)
    print('replicas of the 8 permutations are bit-identical')
    first = [int(np.flatnonzero(which == d)[0]) for d in range(nd)]
    want = cv_perm_expected(X, Y, masks, perms, k)
    got = dict(perm_pearson_r=r[first].transpose(2, 1, 0), perm_r_squared=r2[first].transpose(2, 1, 0),
               perm_mse=mse[first].T)
    _check_null(got, want, 'one batch of 2560 fits vs oracle')


@pytest.mark.parametrize('ids', [[0, 0], [0, 0, 0]])
def test_sharded_over_a_team(ids, monkeypatch):
    """7 permutations over 2 or 3 contexts, uneven shards: the null is bit-identical to one device's, the p-values are
    equal, and the call still makes ONE data collective."""
    import pypyls_amd as pls
    from pypyls_amd import team as _team
    X, Y, rs = _design(100, 250, 5, 41)
    kw = dict(n_components=4, n_perm=10, n_boot=12, seed=17, test_split=5, cv_perm=7, verbose=False)
    one = pls.pls_regression(X, Y, **kw)
    calls = []
    orig = _team.Team.allgather

    def counting(self, rank, flat):
        calls.append(rank)
        return orig(self, rank, flat)
    monkeypatch.setattr(_team.Team, 'allgather', counting)
    team = pls.pls_regression(X, Y, device_ids=ids, **kw)
    print('all-gather calls per rank with cv_perm: {}'.format(sorted(calls)))
    assert sorted(calls) == list(range(len(ids)))
    assert np.array_equal(team.cvres.cvpermsamples, one.cvres.cvpermsamples)
    _same_bits(one.cvres, team.cvres, 'team {} vs one device'.format(ids))


def _flat(res, skip=('inputs',)):
    out = {}
    for key, val in res.items():
        if key in skip:
            continue
        if isinstance(val, dict):
            for k2, v2 in val.items():
                out[key + '.' + k2] = v2
        else:
            out[key] = val
    return out


def test_leaves_the_rest_alone_and_repeats_to_the_bit():
    import pypyls_amd as pls
    X, Y, rs = _design(120, 300, 6, 31)
    kw = dict(n_components=5, n_perm=40, n_boot=40, coef_components=3, test_split=12, seed=4242, verbose=False)
    off = pls.pls_regression(X, Y, **kw)
    on = pls.pls_regression(X, Y, cv_perm=11, **kw)
    again = pls.pls_regression(X, Y, cv_perm=11, **kw)
    new = set('cvres.' + key for key in NULLS + PVALS + ('cvpermsamples',))
    fa, fb, fc = _flat(off), _flat(on), _flat(again)
    assert not new & set(fa) and set(fb) == set(fa) | new
    for key in fa:
        if fa[key] is None:
            assert fb[key] is None, key
        else:
            assert np.array_equal(np.asarray(fa[key]), np.asarray(fb[key]), equal_nan=True), key
    print('{} arrays of the call without cv_perm keep their bits with it'.format(len(fa)))
    for key in new:
        assert np.array_equal(fb[key], fc[key], equal_nan=True), key
    assert 'cv_perm' not in off.inputs and on.inputs.cv_perm == 11
    for key in ('n_perm', 'n_boot', 'n_split', 'n_components', 'seed', 'test_split', 'test_size', 'coef_components'):
        assert on.inputs.get(key) == off.inputs.get(key), key
    want = cv_perm_expected(X, Y, on.cvres.cvsamples, on.cvres.cvpermsamples, 5)
    _check_null(on.cvres, want, 'seeded call vs oracle')


def test_save_and_load_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    X, Y, rs = _design(60, 80, 3, 51)
    res = pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=5, seed=3, cv_perm=4, verbose=False)
    back = pls.load_results(pls.save_results(str(tmp_path / 'cv_perm'), res))
    for key in NULLS + PVALS + ('cvpermsamples',):
        assert np.array_equal(back.cvres[key], res.cvres[key]) and back.cvres[key].shape == res.cvres[key].shape, key
    assert back.cvres.perm_pearson_r.shape == (3, 3, 4) and back.cvres.perm_mse.shape == (4, 4)
    assert int(back.inputs.cv_perm) == 4


def test_abi_refusals():
    """A context bound with PLS-C data, null pointers, m = 0: negative status, a message, and the context works after."""
    import torch
    from pypyls_amd.engine import Engine, PLSX_BEHAVIORAL
    X, Y, rs = _design(40, 50, 3, 61)
    eng = Engine()
    try:
        dm = torch.ones((2, 40), dtype=torch.uint8, device=eng.device)
        dm[:, :10] = 0
        di = eng.rows_tensor(np.stack([rs.permutation(40) for _ in range(3)]))
        out = [eng._zeros((3, 3, 3)), eng._zeros((3, 3, 3)), eng._zeros((3, 4))]

        def call(masks, n, idx, m, o0, o1, o2):
            rc = eng.lib.plsx_simpls_crossval_perm_batch(eng.ctx, masks, n, idx, m, o0, o1, o2, eng._stream())
            msg = eng.lib.plsx_last_error(eng.ctx).decode()
            print('status {}: {}'.format(rc, msg))
            return rc, msg
        ptrs = [t.data_ptr() for t in out]
        eng.set_data(X, Y, np.zeros(40, np.int32), 1, 1, PLSX_BEHAVIORAL)
        rc, msg = call(dm.data_ptr(), 2, di.data_ptr(), 3, *ptrs)
        assert rc == -4 and 'regression' in msg
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), 3)
        for args in ((None, 2, di.data_ptr(), 3) + tuple(ptrs), (dm.data_ptr(), 2, None, 3) + tuple(ptrs),
                     (dm.data_ptr(), 2, di.data_ptr(), 3, None, ptrs[1], ptrs[2]),
                     (dm.data_ptr(), 2, di.data_ptr(), 3, ptrs[0], ptrs[1], None),
                     (dm.data_ptr(), 2, di.data_ptr(), 0) + tuple(ptrs), (dm.data_ptr(), 0, di.data_ptr(), 3) + tuple(ptrs)):
            rc, msg = call(*args)
            assert rc == -1 and 'plsx_simpls_crossval_perm_batch' in msg
        eng.simpls_crossval_perm_into(dm, di, *out)
        eng.sync()
        assert all(torch.isfinite(t).all().item() for t in out)
    finally:
        eng.close()
