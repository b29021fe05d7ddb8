"""pls_regression(confounds=Z) on the device (plsx_simpls_set_confounds: k_cf_resid; plsx_simpls_crossval_confound_batch /
_perm_batch: k_cf_fold_prep, k_cf_fold_F, k_cf_fold_K, k_cf_fold_Y, k_cf_cvp_acc) against the numpy expectation of
tests/confound_expect.py: the residualised analysis, the fold-wise cross-validation and its null, groups of splits,
masked rows, a team, the C ABI, the untouched default and predict / persistence.

Tolerances are the project's own: RTOL = 1e-5 against the oracle (absolute on r, relative to max(1, |value|) on r^2 and
mse), ROUTES = 1e-9 between groupings.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

from confound_expect import (cv_expected_confound, cv_expected_global, cv_perm_expected_confound, residualise,
                             abs_err, rel_err)

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROUTES = 1e-9
NULLS = ('perm_pearson_r', 'perm_r_squared', 'perm_mse')
PVALS = ('pearson_r_pvals', 'r_squared_pvals', 'mse_pvals')


def _masks(rs, S, n):
    masks = np.ones((S, n), dtype=bool)
    for s in range(n):
        masks[rs.choice(S, S // 4, replace=False), s] = False
    return masks


@functools.lru_cache(maxsize=None)
def _linked(S=130, B=300, T=3, q=2, n=5, seed=0):
    """X and Y linked through Z only: unadjusted, the cross-validated r is large; adjusted fold-wise it is about zero."""
    rs = np.random.RandomState(seed)
    Z = rs.randn(S, q)
    X = rs.randn(S, B) + Z @ rs.randn(q, B) * 2.0
    Y = rs.randn(S, T) + Z @ rs.randn(q, T) * 2.0
    return X, Y, Z, _masks(rs, S, n)


@functools.lru_cache(maxsize=None)
def _design(S, B, T, q, n, seed):
    """... and one with a signal of its own next to the confounds."""
    rs = np.random.RandomState(seed)
    Z = rs.randn(S, q)
    X = rs.randn(S, B) + Z @ rs.randn(q, B)
    Y = rs.randn(S, T) + Z @ rs.randn(q, T) + 0.5 * X[:, :T]
    return X, Y, Z, _masks(rs, S, n)


@functools.lru_cache(maxsize=None)
def _perm_case():
    X, Y, Z, masks = _linked()
    masks = masks[:, :4]
    rs = np.random.RandomState(5)
    perms = np.stack([np.arange(len(X))] + [rs.permutation(len(X)) for _ in range(5)], axis=1)
    return X, Y, Z, masks, perms, cv_perm_expected_confound(X, Y, Z, masks, perms, 3)


def _cv_errs(cv, want, what, tol=RTOL):
    errs = dict(r=abs_err(cv['pearson_r_ncomp'], want['r']), r2=rel_err(cv['r_squared_ncomp'], want['r2']),
                mse=rel_err(cv['mse'], want['mse']), r_full=abs_err(cv['pearson_r'], want['r'][:, -1]),
                r2_full=rel_err(cv['r_squared'], want['r2'][:, -1]))
    print('{}: max err r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}  (full model r {r_full:.3e}  r2 {r2_full:.3e})'
          .format(what, **errs))
    assert max(errs.values()) <= tol, (what, errs)


def _null_errs(cv, want, what, tol=RTOL):
    errs = dict(r=abs_err(cv['perm_pearson_r'], want['null']['r']), r2=rel_err(cv['perm_r_squared'], want['null']['r2']),
                mse=rel_err(cv['perm_mse'], want['null']['mse']))
    print('{}: max err of the null r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}'.format(what, **errs))
    assert max(errs.values()) <= tol, (what, errs)


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


def _close(got, want, what, tol):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    err = float(np.max(np.abs(got - want)[~nan] / np.maximum(1.0, np.abs(want[~nan])))) if (~nan).any() else 0.0
    print('{}: max err relative to max(1, |value|) {:.3e}'.format(what, err))
    assert np.array_equal(np.isnan(got), nan) and err <= tol, (what, err)


def test_residual_equivalence():
    """The call with confounds=Z against the call on numpy-residualised (X_r, Y_r), same seed: every numeric array of
    the analysis within RTOL, the drawn samples equal, the slopes against lstsq.  (``intercept`` is the one array that
    speaks of the raw variables: it is checked against its definition, ybar - xbar @ coefs.)"""
    import pypyls_amd as pls
    X, Y, Z, _ = _design(65, 130, 3, 2, 3, 11)
    allr = np.ones(len(X), dtype=bool)
    Xr, Yr = residualise(X, Z, allr), residualise(Y, Z, allr)
    kw = dict(n_components=3, n_perm=20, n_boot=20, n_split=4, coef_components=2, coef_ci=True, vip_components=2,
              seed=7, verbose=False)
    got = pls.pls_regression(X, Y, confounds=Z, **kw)
    want = pls.pls_regression(Xr, Yr, **kw)
    fg, fw = _flat(got), _flat(want)
    new = {'confound_mean', 'confound_x', 'confound_y'}
    assert set(fg) - set(fw) == new and set(fw) <= set(fg)
    for key in sorted(fw):
        if key in ('permres.permsamples', 'bootres.bootsamples'):
            same = np.array_equal(fg[key], fw[key])
            print('{}: equal: {}'.format(key, same))
            assert same, key
        elif key == 'intercept':
            _close(fg[key], Y.mean(axis=0) - X.mean(axis=0) @ fg['coefs'], 'intercept vs ybar - xbar @ coefs', RTOL)
        else:
            _close(fg[key], fw[key], key, RTOL)
    D = np.c_[np.ones(len(X)), Z - Z.mean(axis=0)]
    _close(got['confound_mean'], Z.mean(axis=0), 'confound_mean', 1e-12)
    _close(got['confound_x'], np.linalg.lstsq(D, X, rcond=None)[0][1:], 'confound_x vs lstsq', RTOL)
    _close(got['confound_y'], np.linalg.lstsq(D, Y, rcond=None)[0][1:], 'confound_y vs lstsq', RTOL)
    assert np.array_equal(got.inputs.confounds, Z)


CV_CASES = [(40, 50, 1, 1, 2, 3), (130, 300, 3, 2, 3, 5), (200, 260, 20, 15, 6, 4)]


@pytest.mark.parametrize('S,B,T,q,k,n', CV_CASES)
def test_foldwise_cv_against_the_oracle(S, B, T, q, k, n):
    import pypyls_amd as pls
    X, Y, Z, masks = _linked() if (S, B, T, q, n) == (130, 300, 3, 2, 5) else _design(S, B, T, q, n, 100 + S)
    want = cv_expected_confound(X, Y, Z, masks, k)
    short = cv_expected_global(X, Y, Z, masks, k)
    gap = abs_err(want['r'], short['r'])
    print('S={} B={} T={} q={} k={} n={}: fold-wise vs whole-cohort expectation differ by up to {:.3e} in r; mean test-row r '
          'fold-wise {:.3f}, whole-cohort {:.3f}'.format(S, B, T, q, k, n, gap, want['r'][:, -1].mean(), short['r'][:, -1].mean()))
    if (S, B, T, q, n) == (130, 300, 3, 2, 5):
        # a device path that residualises once over the whole cohort fails the comparison below
        assert gap > 100 * RTOL
    got = pls.pls_regression(X, Y, confounds=Z.ravel() if q == 1 else Z, n_components=k, n_perm=0, n_boot=0, test_split=n,
                             cvsamples=masks, verbose=False)
    assert np.array_equal(got.cvres.cvsamples, masks)
    _cv_errs(got.cvres, want, 'fold-wise CV vs oracle')


def test_cv_perm_against_the_oracle_and_repeats_to_the_bit():
    import pypyls_amd as pls
    X, Y, Z, masks, perms, want = _perm_case()
    kw = dict(confounds=Z, n_components=3, n_perm=0, n_boot=0, test_split=4, cvsamples=masks, cv_perm=6,
              cvpermsamples=perms, verbose=False)
    got = pls.pls_regression(X, Y, **kw)
    cv = got.cvres
    _cv_errs(cv, cv_expected_confound(X, Y, Z, masks, 3), 'observed entry next to cv_perm')
    # the identity permutation reproduces the observed split means
    ident = dict(r=abs_err(cv['perm_pearson_r'][..., 0], cv['pearson_r_ncomp'].mean(axis=-1)),
                 r2=rel_err(cv['perm_r_squared'][..., 0], cv['r_squared_ncomp'].mean(axis=-1)),
                 mse=rel_err(cv['perm_mse'][..., 0], cv['mse'].mean(axis=-1)))
    print('identity permutation vs observed split means: r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}'.format(**ident))
    assert max(ident.values()) <= ROUTES
    _null_errs(cv, want, 'cv_perm null vs oracle')
    for key in ('r', 'r2', 'mse'):
        # (the identity column ties with the observed value exactly; every other null value is far from it)
        gap = float(np.min(np.abs(want['null'][key][..., 1:] - want['obs'][key][..., None])))
        print('smallest distance of a permuted null {} from the observed value: {:.3e}'.format(key, gap))
        assert gap > 100 * RTOL and np.array_equal(want['null'][key][..., 0], want['obs'][key]), key
    for key, name in (('r', 'pearson_r_pvals'), ('r2', 'r_squared_pvals'), ('mse', 'mse_pvals')):
        diff = int(np.sum(cv[name] != want['pvals'][key]))
        print('{} differing from the expected in {} of {} entries'.format(name, diff, want['pvals'][key].size))
        assert cv[name].shape == want['pvals'][key].shape and diff == 0
    again = pls.pls_regression(X, Y, **kw).cvres
    for key in NULLS + PVALS + ('pearson_r_ncomp', 'r_squared_ncomp', 'mse'):
        same = np.array_equal(cv[key], again[key], equal_nan=True)
        print('repeat: {} bit-identical: {}'.format(key, same))
        assert same, key


def test_groups_of_splits_agree_with_the_default():
    """S = 130, T = 3, k = 3: K_s is 135 200 bytes and a fit 39 864 (40 234 under permutations: its scores and mask).
    Half of a 0.0005 GB budget (268 435 bytes) takes one K_s with its fits, so the 4 splits go one per group, and under
    permutations 3 fits share it: the 6 permutations go in two chunks per split."""
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    X, Y, Z, masks, perms, want = _perm_case()
    kw = dict(confounds=Z, n_components=3, n_perm=0, n_boot=0, test_split=4, cvsamples=masks, cv_perm=6,
              cvpermsamples=perms, verbose=False)
    brackets, res = {}, {}
    for name, gb in (('default', None), ('0.0005 GB', 0.0005)):
        eng = Engine(scratch_gb=gb) if gb else Engine()
        try:
            eng.set_timing(True)
            res[name] = pls.pls_regression(X, Y, _engine=eng, **kw).cvres
            kt = eng.kernel_timing()
            brackets[name] = tuple(kt[key][1] for key in ('k_cf_resid', 'k_cf_fold_prep', 'k_cf_fold_K', 'k_cf_fold_Y'))
        finally:
            eng.close()
        print('scratch {}: timed brackets of k_cf_resid / k_cf_fold_prep / k_cf_fold_K / k_cf_fold_Y: {}'
              .format(name, brackets[name]))
    # set_confounds: 2.  Per group of splits, in either entry: 2 of k_cf_fold_prep (with k_cf_fold_F), 1 of k_cf_fold_K.
    # k_cf_fold_Y: 1 per group in the observed entry, 2 per (group, chunk of permutations) in the permuted one.
    assert brackets['default'] == (2, 2 + 2, 1 + 1, 1 + 2)
    assert brackets['0.0005 GB'] == (2, 4 * 2 + 4 * 2, 4 + 4, 4 + 4 * 2 * 2)
    for key in NULLS + ('pearson_r_ncomp', 'r_squared_ncomp', 'mse'):
        err = (abs_err if 'pearson' in key else rel_err)(res['0.0005 GB'][key], res['default'][key])
        print('one K_s per group vs default: {} {:.3e}'.format(key, err))
        assert err <= ROUTES, key
    for key in PVALS:
        assert np.array_equal(res['0.0005 GB'][key], res['default'][key]), key
    _null_errs(res['0.0005 GB'], want, 'one K_s per group vs oracle')


def test_masked_rows():
    import pypyls_amd as pls
    X, Y, Z, masks = (a.copy() for a in _design(90, 120, 3, 2, 4, 23))
    X[4], X[50], Y[17], Z[31] = np.nan, np.nan, np.nan, np.nan
    want = cv_expected_confound(X, Y, Z, masks, 3)
    print('usable test rows per split: {}'.format(want['n_test']))
    got = pls.pls_regression(X, Y, confounds=Z, n_components=3, n_perm=0, n_boot=0, test_split=4, cvsamples=masks,
                             verbose=False)
    _cv_errs(got.cvres, want, 'masked rows: fold-wise CV vs oracle')
    ok = np.ones(len(X), dtype=bool)
    ok[[4, 50, 17, 31]] = False
    _close(got['confound_mean'], Z[ok].mean(axis=0), 'confound_mean over the usable rows', 1e-12)
    assert np.isnan(got['x_scores'][~ok]).all() and np.isfinite(got['x_scores'][ok]).all()
    with pytest.raises(ValueError, match=r'`confounds` with `cv_perm` needs complete data: 4 rows'):
        pls.pls_regression(X, Y, confounds=Z, n_components=3, n_perm=0, n_boot=0, test_split=4, cvsamples=masks,
                           cv_perm=3, verbose=False)


def test_sharded_over_a_team(monkeypatch):
    import pypyls_amd as pls
    from pypyls_amd import team as _team
    X, Y, Z, _ = _design(100, 150, 4, 3, 7, 41)
    kw = dict(confounds=Z, n_components=3, n_perm=6, n_boot=6, seed=17, test_split=7, cv_perm=5, verbose=False)
    one = pls.pls_regression(X, Y, **kw)
    calls = []
    orig = _team.Team.allgather

    def counting(self, rank, flat):
        calls.append(rank)
        return orig(self, rank, flat)
    monkeypatch.setattr(_team.Team, 'allgather', counting)
    team = pls.pls_regression(X, Y, device_ids=[0, 0, 0], **kw)
    print('all-gather calls per rank with confounds: {}'.format(sorted(calls)))
    assert sorted(calls) == [0, 1, 2]
    assert np.array_equal(team.cvres.cvsamples, one.cvres.cvsamples)
    for key in NULLS + ('pearson_r', 'r_squared', 'pearson_r_ncomp', 'r_squared_ncomp', 'mse'):
        err = (abs_err if 'pearson' in key else rel_err)(team.cvres[key], one.cvres[key])
        print('team of 3 vs one device: {} {:.3e}'.format(key, err))
        assert err <= ROUTES, key
    _cv_errs(team.cvres, cv_expected_confound(X, Y, Z, one.cvres.cvsamples, 3), 'team vs oracle')


def _cv_outputs(eng, m, perm=False):
    k, T = eng.k, eng.T
    last = eng._zeros((m, k + 1)) if perm else eng._zeros((m, k + 1, T))
    return eng._zeros((m, k, T)), eng._zeros((m, k, T)), last


def test_abi_states_and_refusals():
    import torch
    from pypyls_amd.engine import Engine, PlsxError, PLSX_BEHAVIORAL
    X, Y, Z, masks = _design(40, 50, 2, 2, 3, 5)
    eng = Engine()
    try:
        # a PLS-C binding: refused with a message, the context works afterwards
        eng.set_data(X, Y, np.zeros(len(X), np.int32), 1, 1, PLSX_BEHAVIORAL)
        before = eng.crosscov()
        with pytest.raises(PlsxError, match=r'status -4: plsx_simpls_set_confounds: data not bound for regression'):
            eng.simpls_set_confounds(Z)
        assert np.array_equal(eng.crosscov(), before)
        # regression data, no confounds yet: both fold entries PLSX_ERR_STATE
        eng.set_data_regression(X, Y - Y.mean(axis=0), 2)
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        idx = eng.rows_tensor(np.stack([np.random.RandomState(s).permutation(len(X)) for s in range(2)]))
        with pytest.raises(PlsxError, match=r'status -4: plsx_simpls_crossval_confound_batch: no confounds are bound'):
            eng.simpls_crossval_confound_into(dm, *_cv_outputs(eng, 3))
        with pytest.raises(PlsxError, match=r'status -4: plsx_simpls_crossval_confound_perm_batch: no confounds are bound'):
            eng.simpls_crossval_confound_perm_into(dm, idx, *_cv_outputs(eng, 2, perm=True))
        # bad q and rank deficient confounds: PLSX_ERR_ARG, the binding untouched
        with pytest.raises(PlsxError, match=r'status -1: .*q outside 1 \.\. 15'):
            eng.simpls_set_confounds(np.random.RandomState(0).randn(len(X), 16))
        with pytest.raises(PlsxError, match=r'status -1: .*rank deficient'):
            eng.simpls_set_confounds(np.c_[Z, Z[:, :1]])
        # bound: the entry works, a new binding clears the confounds
        eng.simpls_set_confounds(Z)
        out = _cv_outputs(eng, 3)
        eng.simpls_crossval_confound_into(dm, *out)
        eng.sync()
        want = cv_expected_confound(X, Y, Z, masks, 2)
        err = abs_err(out[0].cpu().numpy().transpose(2, 1, 0), want['r'])
        print('engine-level fold-wise CV vs oracle: r {:.3e}'.format(err))
        assert err <= RTOL
        eng.set_data_regression(X, Y - Y.mean(axis=0), 2)
        with pytest.raises(PlsxError, match=r'status -4: .*no confounds are bound'):
            eng.simpls_crossval_confound_into(dm, *_cv_outputs(eng, 3))
    finally:
        eng.close()
    # the global route of the solver: PLSX_ERR_UNSUPPORTED, the context still usable
    eng = Engine(options={'simpls_global': 1})
    try:
        eng.set_data_regression(X, Y - Y.mean(axis=0), 2)
        eng.simpls_set_confounds(Z)
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        idx = eng.rows_tensor(np.stack([np.random.RandomState(s).permutation(len(X)) for s in range(2)]))
        with pytest.raises(PlsxError, match=r'status -2: plsx_simpls_crossval_confound_batch: .*on-chip route'):
            eng.simpls_crossval_confound_into(dm, *_cv_outputs(eng, 3))
        with pytest.raises(PlsxError, match=r'status -2: plsx_simpls_crossval_confound_perm_batch: .*on-chip route'):
            eng.simpls_crossval_confound_perm_into(dm, idx, *_cv_outputs(eng, 2, perm=True))
        out = _cv_outputs(eng, 3)
        eng.simpls_crossval_into(dm, *out)             # (the entry without fold-wise regression still runs, on X_r, Y_r)
        eng.sync()
        assert np.isfinite(out[0].cpu().numpy()).all()
    finally:
        eng.close()


def test_no_keyword_changes_nothing():
    import pypyls_amd as pls
    X, Y, Z, masks = _design(65, 130, 3, 2, 3, 11)
    kw = dict(n_components=3, n_perm=12, n_boot=12, n_split=3, coef_components=2, coef_ci=True, vip_components=2,
              test_split=3, cv_perm=4, seed=9, verbose=False)
    a, b = _flat(pls.pls_regression(X, Y, **kw)), _flat(pls.pls_regression(X, Y, confounds=None, **kw))
    assert sorted(a) == sorted(b)
    for key in sorted(a):
        same = np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True)
        print('confounds=None vs no keyword: {} bit-identical: {}'.format(key, same))
        assert same, key
    assert 'confounds' not in pls.pls_regression(X, Y, confounds=None, **kw).inputs


def test_predict_and_persistence(tmp_path):
    import pypyls_amd as pls
    X, Y, Z, _ = _design(65, 130, 3, 2, 3, 11)
    res = pls.pls_regression(X, Y, confounds=Z, n_components=3, n_perm=0, n_boot=0, coef_components=2, verbose=False)
    # on the training rows the prediction is the fitted values of the model of the residuals, in raw units
    allr = np.ones(len(X), dtype=bool)
    Xr, Yr = residualise(X, Z, allr), residualise(Y, Z, allr)
    want = Y - Yr + Xr @ res['coefs']
    got = pls.predict(res, X, confounds=Z)
    _close(got, want, 'predict on the training rows vs numpy', RTOL)
    path = str(tmp_path / 'confound_result.hdf5')
    pls.save_results(path, res)
    back = pls.load_results(path)
    for key in ('confound_mean', 'confound_x', 'confound_y'):
        assert np.array_equal(back[key], res[key]), key
    assert np.array_equal(back.inputs.confounds, Z)
    _close(pls.predict(back, X, confounds=Z), got, 'predict from the reloaded result', 1e-12)
    with pytest.raises(ValueError, match=r'fitted with confounds'):
        pls.predict(back, X)
