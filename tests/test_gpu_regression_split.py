"""pls_regression split-half reliability on the device (plsx_simpls_split_half_batch; k_sd_sh_prep, k_sd_sh_expand,
k_sd_sh_score): against the reference fixtures, the oracle on both routes of the solver, batches, a seeded call, teams
and persistence.

Tolerance: correlations are compared as absolute error against tests/regression_split_expect.py; the ceiling is the
parity bar of the cross-validation tests (tests/test_gpu_regression_cv.py, RTOL).  Every figure is printed before it is
asserted."""
import numpy as np
import pytest

from conftest import load_golden
from regression_split_expect import split_expected, split_null, corr_err

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def _design(S, B, T, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    return X, rs.randn(S, T) + 0.5 * X[:, :T], rs


def _halves(rs, S, n):
    return np.stack([rs.permutation(S) < (S + s % 2) // 2 for s in range(n)], axis=1)


def _bind(eng, X, Y, k):
    """Bind (X, Y) as pls_regression binds them: centred over the rows that are not NaN, NaN rows zeroed and masked."""
    Xc, Yc = X - np.nanmean(X, axis=0), Y - np.nanmean(Y, axis=0)
    okx, oky = ~np.isnan(X).all(axis=1), ~np.isnan(Y).all(axis=1)
    eng.set_data_regression(np.nan_to_num(Xc), np.nan_to_num(Yc), k)
    if not (okx.all() and oky.all()):
        eng.simpls_set_row_masks(okx, oky)


def _entry(eng, masks, perms=None):
    """masks (n, S, ns) bool, perms (S, n) or None -> per-split ucorr, vcorr (n, k, ns) through the engine entry."""
    import torch
    masks = np.asarray(masks)
    n, S, ns = masks.shape
    dm = torch.from_numpy(np.ascontiguousarray(masks.transpose(0, 2, 1), dtype=np.uint8)).to(eng.device)
    dp = None if perms is None else eng.rows_tensor(np.asarray(perms).T)
    uc, vc = eng._empty((n, ns, eng.k)), eng._empty((n, ns, eng.k))
    eng.simpls_split_half_into(dp, dm, uc, vc)
    eng.sync()
    return uc.cpu().numpy().transpose(0, 2, 1), vc.cpu().numpy().transpose(0, 2, 1)


def _engine(glob_=False, **kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1}, **kw) if glob_ else Engine(**kw)


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_fixtures_through_the_public_call(tag):
    """Given permsamples, _splitsamples and _perm_splitsamples: means, p-values and limits through splitres (empty
    before n_split existed), per-split values through the engine entry."""
    import pypyls_amd as pls
    g = load_golden('simpls_split_' + tag)
    k, P = int(g['n_components']), g['permsamples'].shape[1]
    res = pls.pls_regression(g['X'], g['Y'], n_components=k, n_perm=P, n_boot=0, n_split=5, permsamples=g['permsamples'],
                             _splitsamples=g['splitsamples'], _perm_splitsamples=g['perm_splitsamples'], seed=1, ci=90,
                             verbose=False)
    sr = res.splitres
    assert sr._filled() and res.inputs.n_split == 5
    errs = dict(ucorr=corr_err(sr.ucorr, g['ref_ucorr_mean']), vcorr=corr_err(sr.vcorr, g['ref_vcorr_mean']))
    print('simpls_split_{}: observed means vs reference {}'.format(tag, errs))
    assert max(errs.values()) <= RTOL
    assert sr.ucorr.shape == (k,) and sr.vcorr.shape == (k,)
    assert np.array_equal(sr.ucorr_pvals, g['ref_ucorr_pvals']) and np.array_equal(sr.vcorr_pvals, g['ref_vcorr_pvals'])
    for key, null in (('ucorr', g['ref_perm_ucorr_mean']), ('vcorr', g['ref_perm_vcorr_mean'])):
        lo, hi = np.percentile(null, [5, 95], axis=-1)
        e = max(corr_err(sr[key + '_lolim'], lo), corr_err(sr[key + '_uplim'], hi))
        print('simpls_split_{}: {} limits vs reference {:.3e}'.format(tag, key, e))
        assert e <= RTOL
    Y = g['Y'] if g['Y'].ndim == 2 else np.mean(g['Y'], axis=-1)
    eng = _engine()
    try:
        _bind(eng, g['X'], Y, k)
        uc, vc = _entry(eng, g['splitsamples'][None])
        puc, pvc = _entry(eng, g['perm_splitsamples'], g['permsamples'])
    finally:
        eng.close()
    errs = dict(ucorr=corr_err(uc[0], g['ref_ucorr']), vcorr=corr_err(vc[0], g['ref_vcorr']),
                perm_ucorr=corr_err(puc, g['ref_perm_ucorr']), perm_vcorr=corr_err(pvc, g['ref_perm_vcorr']))
    print('simpls_split_{}: per-split values vs reference {}'.format(tag, errs))
    assert max(errs.values()) <= RTOL


@pytest.mark.parametrize('glob_', [False, True], ids=['on-chip', 'global'])
@pytest.mark.parametrize('S,B,T,k', [(61, 130, 5, 6), (90, 33, 3, 4), (64, 100, 1, 1), (70, 200, 9, 9)])
def test_entry_against_the_oracle(S, B, T, k, glob_):
    """The observed arrangement and 3 permutations, 4 splits each; then the same with rows that are NaN throughout in X
    and in Y under permutations that move them.  T = 1: vcorr is NaN where numpy's is."""
    X, Y, rs = _design(S, B, T, 100 + S)
    for nan in (False, True):
        if nan:
            X[[3, 17, S - 1]] = np.nan
            Y[[5, 40]] = np.nan
        masks = np.stack([_halves(rs, S, 4) for _ in range(4)])
        perms = np.stack([np.arange(S)] + [rs.permutation(S) for _ in range(3)], axis=1)
        eng = _engine(glob_)
        try:
            _bind(eng, X, Y, k)
            uc, vc = _entry(eng, masks, perms)
            uc0, vc0 = _entry(eng, masks[:1])                # (no permutation rows: the observed arrangement)
        finally:
            eng.close()
        want = split_null(X, Y, masks, perms, k)
        errs = (corr_err(uc, want[0]), corr_err(vc, want[1]))
        print('S={} B={} T={} k={} {} nan={}: ucorr {:.3e} vcorr {:.3e}'.format(S, B, T, k, 'global' if glob_ else 'on-chip',
                                                                            nan, *errs))
        assert max(errs) <= RTOL
        assert np.array_equal(uc0[0], uc[0]) and np.array_equal(vc0[0], vc[0], equal_nan=True)
        assert np.isnan(want[1]).all() == (T == 1)


def test_bits_do_not_depend_on_the_batches():
    """12 arrangements x 5 splits at S = 61, T = 5, k = 6.  An arrangement holds 3108 doubles of solver state and
    8 k (T + S) = 3168 bytes of y-loadings: 28 032 bytes; a split adds 32 k S = 11 712.  Half of the default budget
    takes everything at once; half of 900 000 bytes takes 5 arrangements with all their splits (86 592 bytes each):
    batches of 5 + 5 + 2; half of 114 624 bytes takes one arrangement and 2 splits: 12 batches of 2 + 2 + 1 splits.
    Launches of the class: one for the row sums of X, one per batch for the y-loadings, two per group of splits."""
    S, B, T, k = 61, 130, 5, 6
    X, Y, rs = _design(S, B, T, 77)
    masks = np.stack([_halves(rs, S, 5) for _ in range(12)])
    perms = np.stack([rs.permutation(S) for _ in range(12)], axis=1)
    got, launches = {}, {}
    for name, gb in (('default', None), ('900 000 B', 900000 / 2 ** 30), ('114 624 B', 114624 / 2 ** 30)):
        eng = _engine(scratch_gb=gb) if gb else _engine()
        try:
            _bind(eng, X, Y, k)
            eng.set_timing(True)
            got[name] = _entry(eng, masks, perms)
            launches[name] = eng.kernel_timing()['k_sd_cv_score'][1]
            if gb is None:
                eng.set_timing(False)
                a, b = _entry(eng, masks[:7], perms[:, :7]), _entry(eng, masks[7:], perms[:, 7:])
                got['two calls'] = tuple(np.concatenate([x, y]) for x, y in zip(a, b))
        finally:
            eng.close()
        print('scratch {}: {} launches of the class'.format(name, launches[name]))
    assert launches == {'default': 1 + 1 + 2, '900 000 B': 1 + 3 * (1 + 2), '114 624 B': 1 + 12 * (1 + 2 * 3)}
    for name in ('900 000 B', '114 624 B', 'two calls'):
        assert np.array_equal(got[name][0], got['default'][0]) and np.array_equal(got[name][1], got['default'][1]), name
    want = split_null(X, Y, masks, perms, k)
    assert max(corr_err(got['default'][0], want[0]), corr_err(got['default'][1], want[1])) <= RTOL


def test_one_split_that_does_not_fit_is_refused():
    from pypyls_amd.engine import PlsxError
    S, B, T, k = 61, 130, 5, 6
    X, Y, rs = _design(S, B, T, 78)
    eng = _engine(scratch_gb=60000 / 2 ** 30)               # half of it: 30 000 < 28 032 + 11 712
    try:
        _bind(eng, X, Y, k)
        with pytest.raises(PlsxError, match='do not fit half the scratch budget'):
            _entry(eng, _halves(rs, S, 2)[None])
        uc, vc = eng.simpls_decompose()[:2]                  # (the context works afterwards)
        assert np.isfinite(uc).all()
    finally:
        eng.close()


def _flat(res, skip=('splitres', 'inputs')):
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


def _assert_same_fields(a, b, what):
    fa, fb = _flat(a), _flat(b)
    assert set(fa) == set(fb), what
    for key in fa:
        if fa[key] is None:
            assert fb[key] is None, key
        else:
            assert np.array_equal(np.asarray(fa[key]), np.asarray(fb[key]), equal_nan=True), (what, key)


def test_a_seeded_call_draws_its_masks_last_and_leaves_the_rest_alone():
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    S, B, T, k, P, ns = 80, 150, 4, 3, 9, 6
    X, Y, rs = _design(S, B, T, 31)
    kw = dict(n_components=k, n_perm=P, n_boot=10, test_split=4, cv_perm=3, seed=4242, verbose=False)
    off = pls.pls_regression(X, Y, **kw)
    assert not off.splitres._filled() and off.inputs.n_split is None
    assert not pls.pls_regression(X, Y, n_split=None, **kw).splitres._filled()
    on = pls.pls_regression(X, Y, n_split=ns, **kw)
    again = pls.pls_regression(X, Y, n_split=ns, **kw)
    _assert_same_fields(off, on, 'n_split 0 vs {}'.format(ns))
    for key in ('permsamples',):
        assert np.array_equal(off.permres[key], on.permres[key])
    assert np.array_equal(off.bootres.bootsamples, on.bootres.bootsamples)
    assert np.array_equal(off.cvres.cvsamples, on.cvres.cvsamples)
    assert np.array_equal(off.cvres.cvpermsamples, on.cvres.cvpermsamples)
    for key in on.splitres:
        assert np.array_equal(on.splitres[key], again.splitres[key], equal_nan=True), key
    for key in ('n_perm', 'n_boot', 'n_components', 'seed', 'rotate', 'ci', 'aggfunc', 'test_size', 'test_split'):
        assert on.inputs.get(key) == off.inputs.get(key), key
    # the stream positions: k SVD seeds, permutations, bootstraps, cross-validation splits, its permutations, THEN the
    # observed data's split masks; permutation i takes the masks of RandomState(i)
    r = np.random.RandomState(4242)
    for _ in range(k):
        r.normal(size=(min(B, T), 11))
    assert np.array_equal(rsmp.gen_permsamp([S], 1, P, seed=r, verbose=False), on.permres.permsamples)
    rsmp.gen_bootsamp([S], 1, 10, seed=r, verbose=False)
    assert np.array_equal(rsmp.gen_splits([S], 1, 4, seed=r, test_size=0.25), on.cvres.cvsamples)
    rsmp.gen_permsamp([S], 1, 3, seed=r, verbose=False)
    masks = rsmp.gen_splits([S], 1, ns, seed=r, test_size=0.5)
    perm_masks = rsmp.gen_splits_seeded([S], 1, ns, np.arange(P), test_size=0.5)
    uc, vc = split_expected(X, Y, masks, k)
    puc, pvc = split_null(X, Y, perm_masks, on.permres.permsamples, k)
    errs = dict(ucorr=corr_err(on.splitres.ucorr, uc.mean(axis=-1)), vcorr=corr_err(on.splitres.vcorr, vc.mean(axis=-1)))
    null_u, null_v = puc.mean(axis=-1).T, pvc.mean(axis=-1).T
    lo, hi = np.percentile(null_u, [2.5, 97.5], axis=-1)
    errs['ucorr_lim'] = max(corr_err(on.splitres.ucorr_lolim, lo), corr_err(on.splitres.ucorr_uplim, hi))
    lo, hi = np.percentile(null_v, [2.5, 97.5], axis=-1)
    errs['vcorr_lim'] = max(corr_err(on.splitres.vcorr_lolim, lo), corr_err(on.splitres.vcorr_uplim, hi))
    print('seeded call vs oracle at the documented stream positions: {}'.format(errs))
    assert max(errs.values()) <= RTOL


def test_without_permutations_only_the_observed_means_are_filled():
    import pypyls_amd as pls
    X, Y, rs = _design(60, 90, 3, 37)
    res = pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, n_split=4, seed=5, verbose=False)
    assert res.splitres._filled() == {'ucorr', 'vcorr'}
    r = np.random.RandomState(5)
    for _ in range(3):
        r.normal(size=(3, 11))
    from pypyls_amd import resampling as rsmp
    uc, vc = split_expected(X, Y, rsmp.gen_splits([60], 1, 4, seed=r, test_size=0.5), 3)
    assert max(corr_err(res.splitres.ucorr, uc.mean(axis=-1)), corr_err(res.splitres.vcorr, vc.mean(axis=-1))) <= RTOL


@pytest.mark.parametrize('ids', [[0, 0], [0, 0, 0]])
def test_sharded_over_a_team(ids, monkeypatch):
    """7 permutations over 2 or 3 contexts (uneven shards) and 2 over 3 (an empty one): splitres equals the one-device
    call, the rest equals the team call without split-half, and the call makes ONE data collective."""
    import pypyls_amd as pls
    from pypyls_amd import team as _team
    X, Y, rs = _design(70, 120, 4, 41)
    for P in (7, 2) if len(ids) == 3 else (7,):
        kw = dict(n_components=3, n_perm=P, n_boot=6, seed=17, verbose=False)
        one = pls.pls_regression(X, Y, n_split=5, **kw)
        calls = []
        orig = _team.Team.allgather

        def counting(self, rank, flat):
            calls.append(rank)
            return orig(self, rank, flat)
        monkeypatch.setattr(_team.Team, 'allgather', counting)
        team_off = pls.pls_regression(X, Y, device_ids=ids, **kw)
        del calls[:]
        team_on = pls.pls_regression(X, Y, device_ids=ids, n_split=5, **kw)
        monkeypatch.setattr(_team.Team, 'allgather', orig)
        print('all-gather calls per rank with split-half, {} permutations: {}'.format(P, sorted(calls)))
        assert sorted(calls) == list(range(len(ids)))        # every rank's thread enters the ONE collective once
        for key in one.splitres:
            assert np.array_equal(one.splitres[key], team_on.splitres[key], equal_nan=True), (P, key)
        _assert_same_fields(team_off, team_on, 'team without vs with split-half')


def test_3d_y_and_save_load_round_trip(tmp_path):
    import pypyls_amd as pls
    S, B, T, C, k = 60, 100, 4, 3, 3
    rs = np.random.RandomState(51)
    X = rs.randn(S, B)
    Y = rs.randn(S, T, C) + 0.5 * X[:, :T, None]
    Y[11] = np.nan
    masks = _halves(rs, S, 4)
    res = pls.pls_regression(X, Y, n_components=k, n_perm=5, n_boot=0, aggfunc='median', n_split=4, _splitsamples=masks,
                             seed=3, verbose=False)
    uc, vc = split_expected(X, np.median(Y, axis=-1), masks, k)
    errs = (corr_err(res.splitres.ucorr, uc.mean(axis=-1)), corr_err(res.splitres.vcorr, vc.mean(axis=-1)))
    print('3-D Y median with a missing subject: {}'.format(errs))
    assert max(errs) <= RTOL
    back = pls.load_results(pls.save_results(str(tmp_path / 'split'), res))
    assert set(back.splitres.keys()) == set(res.splitres.keys()) and len(res.splitres.keys()) == 8
    for key in res.splitres:
        assert np.array_equal(back.splitres[key], res.splitres[key]), key
    assert back.inputs.n_split == 4


def test_the_symbol_is_exported():
    from pypyls_amd import engine
    assert 'plsx_simpls_split_half_batch' in engine.exported_symbols()
