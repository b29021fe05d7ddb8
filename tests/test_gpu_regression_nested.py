"""pls_regression(inner_split=ni) on the device (plsx_simpls_crossval_nested_batch / _perm_batch: k_sd_cvn_expand, the
fit-and-score body of the cross-validation on tri-state masks, k_sd_cvn_select, k_sd_cvn_reduce): against the oracle
(tests/regression_nested_expect.py), the plain cross-validation, the two routes of the solver, solver batches, teams,
persistence and the refusals of the C ABI.

Tolerance: the project's parity bar for regression (tests/test_gpu_regression_cv.py), RTOL = 1e-5 absolute on r,
relative to max(1, |value|) on r^2, mse and inner_mse.  The selection is discrete, so every design compared with the
oracle must have the ORACLE's own selection_gap >= 1e-4 (10 x the bar): asserted on the oracle's values before the
device result is looked at; given that, the selected counts are compared exactly.  Every figure is printed before it is
asserted."""
import numpy as np
import pytest

import regression_nested_expect as ne

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROUTES = 1e-9
GAP = 1e-4
OBS = ('nested_ncomp', 'nested_pearson_r', 'nested_r_squared', 'nested_mse', 'inner_mse')
NULLS = ('perm_nested_pearson_r', 'perm_nested_r_squared', 'perm_nested_mse', 'perm_nested_ncomp')
PVALS = ('nested_pearson_r_pvals', 'nested_r_squared_pvals', 'nested_mse_pvals')
# S, B, T, k, outer, inner, P, seed, sig: the three designs of the null (the first is also the observed case)
DESIGNS = [(90, 150, 3, 5, 6, 4, 5, 3, 0.5), (130, 300, 4, 6, 5, 3, 4, 11, 0.5), (70, 40, 2, 4, 4, 3, 6, 5, 0.8)]


def _global_engine(**kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1}, **kw)


def _codes(cv):
    from pypyls_amd.regression import nested_codes
    return nested_codes(cv['cvsamples'], cv['innersamples'])


def _oracle(X, Y, cv, k, what, perms=True):
    """The oracle on the call's own splits, folds and permutations; its selection gap is asserted HERE, before any
    device number is compared."""
    codes = _codes(cv)
    obs = ne.nested_expected(X, Y, codes, k)
    nul = ne.nested_perm_expected(X, Y, codes, k, cv['cvpermsamples']) if perms and 'cvpermsamples' in cv else None
    gap = ne.selection_gap(obs['inner_mse'], *([nul['inner_mse']] if nul is not None else []))
    print('{}: oracle selection gap {:.3e}; observed ncomp {}'.format(what, gap, obs['ncomp']))
    assert gap >= GAP, (what, gap)
    return obs, nul


def _check_obs(cv, obs, what):
    errs = dict(r=ne.abs_err(cv['nested_pearson_r'], obs['r']), r2=ne.rel_err(cv['nested_r_squared'], obs['r2']),
                mse=ne.rel_err(cv['nested_mse'], obs['mse']), inner=ne.rel_err(cv['inner_mse'], obs['inner_mse']))
    print('{}: max err of nested r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}  inner_mse {inner:.3e}; ncomp {nc}'
          .format(what, nc=cv['nested_ncomp'], **errs))
    assert np.array_equal(cv['nested_ncomp'], obs['ncomp']), (what, cv['nested_ncomp'], obs['ncomp'])
    assert max(errs.values()) <= RTOL, (what, errs)


def _check_null(cv, obs, nul, what, n):
    errs = dict(r=ne.abs_err(cv['perm_nested_pearson_r'], nul['r']), r2=ne.rel_err(cv['perm_nested_r_squared'], nul['r2']),
                mse=ne.rel_err(cv['perm_nested_mse'], nul['mse']))
    print('{}: max err of the nested null r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}; counts\n{cnt}'
          .format(what, cnt=cv['perm_nested_ncomp'], **errs))
    assert np.array_equal(cv['perm_nested_ncomp'], nul['ncomp']), what
    assert (cv['perm_nested_ncomp'].sum(axis=0) == n).all(), what
    assert max(errs.values()) <= RTOL, (what, errs)
    want = dict(nested_pearson_r_pvals=ne.pvals(ne.split_mean(obs['r']), nul['r']),
                nested_r_squared_pvals=ne.pvals(ne.split_mean(obs['r2']), nul['r2']),
                nested_mse_pvals=ne.pvals(ne.split_mean(obs['mse']), nul['mse'], smaller=True))
    for key, val in want.items():
        print('{}: {} {} expected {}'.format(what, key, cv[key], val))
        assert np.array_equal(np.asarray(cv[key]), np.asarray(val)), (what, key)


def _same_bits(a, b, what, keys=OBS + NULLS + PVALS):
    for key in keys:
        same = np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True)
        print('{}: {} bit-identical: {}'.format(what, key, same))
        assert same, (what, key)


def _call(design, **extra):
    import pypyls_amd as pls
    S, B, T, k, no, ni, P, seed, sig = design
    X, Y = ne.design(S, B, T, seed, sig)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=no, inner_split=ni, seed=seed, verbose=False)
    kw.update(extra)
    return X, Y, pls.pls_regression(X, Y, **kw)


@pytest.fixture(scope='module')
def first():
    """Design 1 with its null on the default engine: shared by the tests that read it (and leave it unchanged)."""
    X, Y, res = _call(DESIGNS[0], cv_perm=DESIGNS[0][6])
    return X, Y, res


def test_observed_vs_oracle_on_both_routes(first):
    """S = 90 (no multiple of 64), k = 5 (no multiple of 4), 6 x 4 drawn splits."""
    X, Y, res = first
    obs, _ = _oracle(X, Y, res.cvres, 5, 'S=90 observed', perms=False)
    _check_obs(res.cvres, obs, 'S=90 on-chip vs oracle')
    assert res.cvres.nested_pearson_r.shape == (3, 6) and res.cvres.inner_mse.shape == (6, 6)
    assert res.cvres.innersamples.shape == (90, 6, 4) and res.cvres.innersamples.dtype == np.uint8
    eng = _global_engine()
    try:
        _, _, gl = _call(DESIGNS[0], cv_perm=DESIGNS[0][6], _engine=eng)
    finally:
        eng.close()
    assert np.array_equal(gl.cvres.innersamples, res.cvres.innersamples)
    _check_obs(gl.cvres, obs, 'S=90 simpls_global vs oracle')
    diff = max(ne.abs_err(gl.cvres[key], res.cvres[key]) for key in OBS + NULLS)
    print('routes differ by at most {:.3e}'.format(diff))
    assert diff <= ROUTES


def test_consistent_with_the_plain_cross_validation_to_the_bit(first):
    import pypyls_amd as pls
    from pypyls_amd import resampling
    from pypyls_amd.regression import _draw_inner_codes
    X, Y, res = first
    S, B, T, k, no, ni, P, seed, sig = DESIGNS[0]
    cv = res.cvres
    nc = cv.nested_ncomp
    assert nc.min() >= 1
    for s in range(no):
        assert np.array_equal(cv.nested_pearson_r[:, s], cv.pearson_r_ncomp[:, nc[s] - 1, s]), s
        assert np.array_equal(cv.nested_r_squared[:, s], cv.r_squared_ncomp[:, nc[s] - 1, s]), s
    plain = cv.mse[nc, np.arange(no)]
    err = float(np.max(np.abs(cv.nested_mse - plain) / np.abs(plain)))
    print('nested_mse vs mse[ncomp[s], s]: {:.3e} relative'.format(err))
    assert err <= 1e-12
    # every array of the same call without inner_split is bit-identical
    off = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, test_split=no, seed=seed, cv_perm=P, verbose=False)
    new = set(OBS + NULLS + PVALS + ('innersamples',))
    assert not new & set(off.cvres.keys()) and set(cv.keys()) == set(off.cvres.keys()) | new
    for key in off.cvres.keys():
        assert np.array_equal(np.asarray(off.cvres[key]), np.asarray(cv[key]), equal_nan=True), key
    for key in ('x_weights', 'x_scores', 'y_loadings', 'y_scores', 'varexp'):
        if off.get(key) is not None:
            assert np.array_equal(off[key], res[key], equal_nan=True), key
    assert 'inner_split' not in off.inputs and res.inputs.inner_split == ni
    # its seeded draws are unchanged, and the inner folds are the next draw of the call's generator
    rs = resampling.check_random_state(seed)
    for _ in range(k):
        rs.normal(size=(min(B, T), 11))
    masks = resampling.gen_splits([S], 1, no, seed=rs, test_size=0.25)
    perms = resampling.gen_permsamp([S], 1, P, seed=rs, verbose=False)
    assert np.array_equal(masks, cv.cvsamples) and np.array_equal(perms, cv.cvpermsamples)
    assert np.array_equal(_draw_inner_codes(masks, ni, rs, 0.25), cv.innersamples)


@pytest.mark.parametrize('i', [0, 1, 2])
def test_null_vs_oracle(i, first):
    design = DESIGNS[i]
    X, Y, res = first if i == 0 else _call(design, cv_perm=design[6])
    S, B, T, k, no, ni, P = design[:7]
    obs, nul = _oracle(X, Y, res.cvres, k, 'design {}'.format(design))
    assert res.cvres.perm_nested_pearson_r.shape == (T, P) and res.cvres.perm_nested_ncomp.shape == (k, P)
    assert res.cvres.perm_nested_mse.shape == (P,) and np.issubdtype(res.cvres.perm_nested_ncomp.dtype, np.integer)
    _check_obs(res.cvres, obs, 'design {} observed'.format(i))
    _check_null(res.cvres, obs, nul, 'design {} null'.format(i), no)


def test_identity_permutation_ties_with_the_observed_means():
    S, B, T, k, no, ni, P, seed, sig = DESIGNS[2]
    perms = np.stack([np.arange(S), np.random.RandomState(1).permutation(S)], axis=1)
    X, Y, res = _call(DESIGNS[2], cv_perm=2, cvpermsamples=perms)
    cv = res.cvres
    errs = dict(r=ne.abs_err(cv.perm_nested_pearson_r[:, 0], ne.split_mean(cv.nested_pearson_r)),
                r2=ne.rel_err(cv.perm_nested_r_squared[:, 0], ne.split_mean(cv.nested_r_squared)),
                mse=ne.rel_err(cv.perm_nested_mse[0], ne.split_mean(cv.nested_mse)))
    print('identity permutation vs the observed split means: {}'.format(errs))
    assert max(errs.values()) <= 1e-12
    assert np.array_equal(cv.perm_nested_ncomp[:, 0], np.bincount(cv.nested_ncomp, minlength=k + 1)[1:])
    # a tie is not larger / not smaller
    assert (cv.nested_pearson_r_pvals <= 2 / 3).all() and cv.nested_mse_pvals <= 2 / 3


def test_rows_nan_throughout_in_x_and_in_y():
    """S = 70 with masked rows of X, of Y and of both: the usable test rows differ per (permutation, fold)."""
    import pypyls_amd as pls
    S, B, T, k, no, ni, P, seed, sig = DESIGNS[2]
    X, Y = ne.design(S, B, T, seed, sig)
    X[[3, 40]] = np.nan
    Y[[17, 40, 55]] = np.nan
    res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, test_split=no, inner_split=ni, seed=seed,
                             cv_perm=P, verbose=False)
    obs, nul = _oracle(X, Y, res.cvres, k, 'S=70 with masked rows')
    _check_obs(res.cvres, obs, 'masked rows observed')
    _check_null(res.cvres, obs, nul, 'masked rows null', no)


def _given_folds(S, no, ni, seed):
    from pypyls_amd import resampling
    from pypyls_amd.regression import _draw_inner_codes
    masks = resampling.gen_splits([S], 1, no, seed=seed, test_size=0.25)
    return masks, _draw_inner_codes(masks, ni, np.random.RandomState(seed + 1), 0.25)


@pytest.mark.parametrize('kind, want', [('low rank', 4), ('noise', 1)])
def test_given_innersamples(kind, want):
    """A strong signal of rank k = 4 spread evenly over four orthogonal directions: every inner fold set chooses c = k;
    pure noise: c = 1.  Checked on the oracle first."""
    import pypyls_amd as pls
    S, B, T, k, no, ni = 80, 30, 4, 4, 3, 3
    rs = np.random.RandomState(21)
    X = rs.randn(S, B)
    if kind == 'low rank':
        X[:, :4] *= np.array([4.0, 3.0, 2.0, 1.5])                # distinct variances: one component per direction
        Y = X[:, :4] * np.array([1.0, 1.4, 2.0, 2.6]) + 0.05 * rs.randn(S, T)
    else:
        Y = rs.randn(S, T)
    masks, inner = _given_folds(S, no, ni, 8)
    res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, test_split=no, cvsamples=masks, inner_split=ni,
                             innersamples=inner, verbose=False)
    assert np.array_equal(res.cvres.innersamples, inner) and np.array_equal(res.cvres.cvsamples, masks)
    obs, _ = _oracle(X, Y, res.cvres, k, kind, perms=False)
    assert (obs['ncomp'] == want).all(), obs['ncomp']
    _check_obs(res.cvres, obs, 'given folds, {}'.format(kind))


def test_solver_batches_do_not_change_the_bits():
    """3 outer x 2 inner x 5 permutations at S = 1000, T = 6, k = 5: 15 groups of 3 fits of about 0.48 MB each.  Half of
    a 0.02 GB budget takes 22 fits, so 7 whole groups: batches of 7 + 7 + 1 groups, and permutations 2 and 4 straddle
    two batches each.  A budget below one group is refused and the context works afterwards."""
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine, PlsxError
    S, B, T, k = 1000, 200, 6, 5
    X, Y = ne.design(S, B, T, 29, 0.5)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=3, inner_split=2, seed=12, cv_perm=5, verbose=False)
    one = pls.pls_regression(X, Y, **kw)
    for name, gb in (('default', None), ('0.02 GB', 0.02)):
        eng = Engine(scratch_gb=gb) if gb else Engine()
        try:
            got = pls.pls_regression(X, Y, _engine=eng, **kw)
        finally:
            eng.close()
        _same_bits(one.cvres, got.cvres, 'scratch {} vs the default engine'.format(name))
    # ... and however the permutations are cut into calls: one at a time
    from pypyls_amd.regression import nested_codes
    codes = nested_codes(one.cvres.cvsamples, one.cvres.innersamples)
    eng = Engine(scratch_gb=0.02)
    try:
        eng.set_data_regression(X, Y - np.nanmean(Y, axis=0, keepdims=True), k)     # (as the front end binds it)
        for p in (2, 4):
            part = eng.simpls_crossval_nested_perm(codes, one.cvres.cvpermsamples[:, p:p + 1])
            for key in NULLS:
                assert np.array_equal(part[key][..., 0], one.cvres[key][..., p]), (p, key)
    finally:
        eng.close()
    eng = Engine(scratch_gb=0.002)
    try:
        eng.set_data_regression(X, Y - np.nanmean(Y, axis=0, keepdims=True), k)
        with pytest.raises(PlsxError, match=r'status -2.*one group of 1 \+ 2 fits.*S = 1000, T = 6, k = 5') as info:
            eng.simpls_crossval_nested(codes)
        print(info.value)
        dm = torch.from_numpy(np.ascontiguousarray(one.cvres.cvsamples.T, dtype=np.uint8)).to(eng.device)
        out = [eng._zeros((3, k, T)), eng._zeros((3, k, T)), eng._zeros((3, k + 1, T))]
        eng.simpls_crossval_into(dm, *out)
        eng.sync()
        r = out[0].cpu().numpy().transpose(2, 1, 0)
        assert np.array_equal(r, one.cvres.pearson_r_ncomp)
    finally:
        eng.close()


@pytest.mark.parametrize('ids', [[0, 0], [0, 0, 0]])
def test_sharded_over_a_team(ids, first, monkeypatch):
    """5 permutations and 6 outer splits over 2 or 3 contexts: bit-identical to one device, ONE data collective."""
    from pypyls_amd import team as _team
    X, Y, one = first
    calls = []
    orig = _team.Team.allgather

    def counting(self, rank, flat):
        calls.append(rank)
        return orig(self, rank, flat)
    monkeypatch.setattr(_team.Team, 'allgather', counting)
    _, _, team = _call(DESIGNS[0], cv_perm=DESIGNS[0][6], device_ids=ids)
    print('all-gather calls per rank with inner_split: {}'.format(sorted(calls)))
    assert sorted(calls) == list(range(len(ids)))
    assert np.array_equal(team.cvres.innersamples, one.cvres.innersamples)
    _same_bits(one.cvres, team.cvres, 'team {} vs one device'.format(ids))


def test_save_load_and_repeat(first, tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    X, Y, res = first
    _, _, again = _call(DESIGNS[0], cv_perm=DESIGNS[0][6])
    _same_bits(res.cvres, again.cvres, 'repeat of the call', keys=OBS + NULLS + PVALS + ('innersamples',))
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    back = pls.load_results(pls.save_results(str(tmp_path / 'nested'), res))
    for key in OBS + NULLS + PVALS[:2] + ('innersamples',):
        assert np.array_equal(back.cvres[key], res.cvres[key], equal_nan=True), key
        assert back.cvres[key].shape == res.cvres[key].shape and back.cvres[key].dtype == res.cvres[key].dtype, key
    assert float(back.cvres.nested_mse_pvals) == float(res.cvres.nested_mse_pvals)
    assert int(back.inputs.inner_split) == DESIGNS[0][5]


def test_abi_refusals():
    """A PLS-C binding, null pointers, n / ni / m = 0, an open series of counts, bound confounds: a negative status, a
    message, and the context is usable afterwards."""
    import torch
    from pypyls_amd.engine import Engine, PLSX_BEHAVIORAL
    from pypyls_amd.regression import nested_codes
    S, k, T, n, ni, m = 40, 3, 3, 2, 2, 3
    rs = np.random.RandomState(61)
    X = rs.randn(S, 50)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    masks, inner = _given_folds(S, n, ni, 3)
    codes = nested_codes(masks, inner)
    eng = Engine()
    try:
        dc = torch.from_numpy(np.ascontiguousarray(codes.transpose(1, 2, 0))).to(eng.device)
        di = eng.rows_tensor(np.stack([rs.permutation(S) for _ in range(m)]))
        obs = [eng._zeros((n, T)), eng._zeros((n, T)), eng._zeros((n,)),
               torch.zeros((n,), dtype=torch.int32, device=eng.device), eng._zeros((n, k + 1))]
        nul = [eng._zeros((m, T)), eng._zeros((m, T)), eng._zeros((m,)),
               torch.zeros((m, k), dtype=torch.int32, device=eng.device)]
        op, nup = [t.data_ptr() for t in obs], [t.data_ptr() for t in nul]

        def call_obs(c, n_, ni_, *o):
            rc = eng.lib.plsx_simpls_crossval_nested_batch(eng.ctx, c, n_, ni_, *o, eng._stream())
            msg = eng.lib.plsx_last_error(eng.ctx).decode()
            print('observed: status {}: {}'.format(rc, msg))
            return rc, msg

        def call_nul(c, n_, ni_, i, m_, *o):
            rc = eng.lib.plsx_simpls_crossval_nested_perm_batch(eng.ctx, c, n_, ni_, i, m_, *o, eng._stream())
            msg = eng.lib.plsx_last_error(eng.ctx).decode()
            print('permuted: status {}: {}'.format(rc, msg))
            return rc, msg
        eng.set_data(X, Y, np.zeros(S, np.int32), 1, 1, PLSX_BEHAVIORAL)
        for rc, msg in (call_obs(dc.data_ptr(), n, ni, *op), call_nul(dc.data_ptr(), n, ni, di.data_ptr(), m, *nup)):
            assert rc == -4 and 'regression' in msg
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)
        for args in ((None, n, ni) + tuple(op), (dc.data_ptr(), 0, ni) + tuple(op), (dc.data_ptr(), n, 0) + tuple(op)) + \
                tuple((dc.data_ptr(), n, ni) + tuple(None if j == i else p for j, p in enumerate(op)) for i in range(5)):
            rc, msg = call_obs(*args)
            assert rc == -1 and 'plsx_simpls_crossval_nested_batch' in msg
        for args in ((None, n, ni, di.data_ptr(), m) + tuple(nup), (dc.data_ptr(), n, ni, None, m) + tuple(nup),
                     (dc.data_ptr(), 0, ni, di.data_ptr(), m) + tuple(nup), (dc.data_ptr(), n, 0, di.data_ptr(), m) + tuple(nup),
                     (dc.data_ptr(), n, ni, di.data_ptr(), 0) + tuple(nup)) + \
                tuple((dc.data_ptr(), n, ni, di.data_ptr(), m) + tuple(None if j == i else p for j, p in enumerate(nup))
                      for i in range(4)):
            rc, msg = call_nul(*args)
            assert rc == -1 and 'plsx_simpls_crossval_nested_perm_batch' in msg
        # an open series of counts (PLS-DA)
        eng.simpls_set_classes(np.arange(S) % T)
        conf = torch.zeros((4, k, T, T), dtype=torch.int32, device=eng.device)
        eng.simpls_cv_class_begin(conf)
        for rc, msg in (call_obs(dc.data_ptr(), n, ni, *op), call_nul(dc.data_ptr(), n, ni, di.data_ptr(), m, *nup)):
            assert rc == -4 and 'series of counts' in msg
        eng.simpls_cv_class_end()
        eng.simpls_crossval_nested_into(dc, *obs)
        eng.simpls_crossval_nested_perm_into(dc, di, *nul)
        eng.sync()
        assert all(torch.isfinite(t.to(torch.float64)).all().item() for t in obs + nul)
        assert (nul[3].sum(dim=1) == n).all().item() and 1 <= int(obs[3].min()) and int(obs[3].max()) <= k
        want = ne.nested_expected(X, Y, codes, k)
        print('after the refusals: ncomp {} expected {}'.format(obs[3].cpu().numpy(), want['ncomp']))
        assert ne.rel_err(obs[4].cpu().numpy().T, want['inner_mse']) <= RTOL
        # bound confounds
        eng.simpls_set_confounds(rs.randn(S, 2))
        for rc, msg in (call_obs(dc.data_ptr(), n, ni, *op), call_nul(dc.data_ptr(), n, ni, di.data_ptr(), m, *nup)):
            assert rc == -2 and 'confounds' in msg
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)
        eng.simpls_crossval_nested_into(dc, *obs)
        eng.sync()
        assert ne.rel_err(obs[4].cpu().numpy().T, want['inner_mse']) <= RTOL
    finally:
        eng.close()
