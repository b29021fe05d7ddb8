"""pls_regression cross-validation per component count on the device (plsx_simpls_crossval_batch, k_sd_cv_score):
against the reference fixtures, the oracle, the two routes of the solver, batches, teams and persistence.

Tolerance: the project's parity bar for regression (tests/test_gpu_regression.py), absolute on r, relative to
max(1, |value|) on r^2 and mse.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from conftest import load_golden
from regression_cv_expect import cv_expected, abs_err, rel_err

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROUTES = 1e-9


def _global_engine(**kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1}, **kw)


def _design(S, B, T, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    return X, rs.randn(S, T) + 0.5 * X[:, :T], rs


def _check(cv, want, what, tol=RTOL):
    """cvres against dict(r, r2, mse) (T, k, n) / (k + 1, n)."""
    k = want['r'].shape[1]
    errs = dict(r=abs_err(cv['pearson_r_ncomp'], want['r']), r2=rel_err(cv['r_squared_ncomp'], want['r2']),
                mse=rel_err(cv['mse'], want['mse']))
    print('{}: max err r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}'.format(what, **errs))
    assert max(errs.values()) <= tol, (what, errs)
    assert np.array_equal(cv['pearson_r'], cv['pearson_r_ncomp'][:, k - 1])
    assert np.array_equal(cv['r_squared'], cv['r_squared_ncomp'][:, k - 1])
    return errs


def _same(a, b, tol, what):
    errs = dict(r=abs_err(a['pearson_r_ncomp'], b['pearson_r_ncomp']),
                r2=rel_err(a['r_squared_ncomp'], b['r_squared_ncomp']), mse=rel_err(a['mse'], b['mse']))
    print('{}: max diff r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}'.format(what, **errs))
    assert max(errs.values()) <= tol, (what, errs)


@pytest.mark.parametrize('tag', ['a', 'b', 'nan'])
def test_goldens_on_both_routes(tag):
    import pypyls_amd as pls
    g = load_golden('simpls_cv_' + tag)
    k, masks = int(g['n_components']), g['cvsamples']
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=masks.shape[1], cvsamples=masks, seed=1, verbose=False)
    want = dict(r=g['ref_r'], r2=g['ref_r2'], mse=g['ref_mse'])
    chip = pls.pls_regression(g['X'], g['Y'], **kw)
    _check(chip.cvres, want, 'simpls_cv_{} on-chip vs reference'.format(tag))
    eng = _global_engine()
    try:
        glob_ = pls.pls_regression(g['X'], g['Y'], _engine=eng, **kw)
    finally:
        eng.close()
    _check(glob_.cvres, want, 'simpls_cv_{} global vs reference'.format(tag))
    _same(chip.cvres, glob_.cvres, ROUTES, 'simpls_cv_{} on-chip vs global'.format(tag))
    assert chip.cvres.pearson_r.shape == (g['Y'].shape[1], masks.shape[1])
    assert chip.cvres.mse.shape == (k + 1, masks.shape[1])
    assert np.array_equal(chip.cvres.cvsamples, masks) and chip.cvres.cvsamples.dtype == bool


def test_past_the_reference_pin_t20_k15():
    """T = 20 (the reference's randomized SVD is approximate beyond 11 columns): every (c, behaviour, split) of 16
    seeded splits against the oracle; mse[0] against the intercept-only model in numpy."""
    import pypyls_amd as pls
    S, B, T, k = 300, 2000, 20, 15
    X, Y, rs = _design(S, B, T, 7)
    res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, test_split=16, test_size=0.25, seed=99,
                             verbose=False)
    masks = res.cvres.cvsamples
    assert masks.shape == (S, 16) and masks.dtype == bool
    from pypyls_amd import resampling as rsmp
    rstate = np.random.RandomState(99)
    for _ in range(k):
        rstate.normal(size=(min(B, T), 11))                  # what the call draws before the splits
    assert np.array_equal(masks, rsmp.gen_splits([S], 1, 16, seed=rstate, test_size=0.25))
    want = cv_expected(X, Y, masks, k)
    _check(res.cvres, want, 'T=20 k=15 vs oracle')
    mse0 = np.array([np.mean(np.sum((Y[~masks[:, s]] - Y[masks[:, s]].mean(axis=0)) ** 2, axis=1))
                     for s in range(16)])
    e0 = rel_err(res.cvres.mse[0], mse0)
    print('mse[0] vs intercept-only model: {:.3e}'.format(e0))
    assert e0 <= RTOL


def test_one_batch_of_2304_takes_the_large_batch_instantiations():
    """Above 2048 splits per batch the solver and k_sd_cv_score run their three-waves-per-SIMD instantiations: 8
    distinct masks at c5's solver shape class (S = 1000, T = 20, k = 15) replicated into ONE call of 2304."""
    import torch
    from pypyls_amd.engine import Engine
    from pypyls_amd import resampling as rsmp
    S, B, T, k = 1000, 2000, 20, 15
    X, Y, rs = _design(S, B, T, 3)
    n, nd = 2304, 8
    masks = rsmp.gen_splits([S], 1, nd, seed=77, test_size=0.25)
    which = np.arange(n) % nd
    which[[0, 1, n - 2, n - 1]] = [5, 2, 7, 0]
    eng = Engine()
    try:
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)
        dm = torch.from_numpy(np.ascontiguousarray(masks[:, which].T, dtype=np.uint8)).to(eng.device)
        r, r2, sse = eng._zeros((n, k, T)), eng._zeros((n, k, T)), eng._zeros((n, k + 1, T))
        eng.simpls_crossval_into(dm, r, r2, sse)
        eng.sync()
        r, r2, sse = r.cpu().numpy(), r2.cpu().numpy(), sse.cpu().numpy()
    finally:
        eng.close()
    for d in range(nd):
        cols = np.flatnonzero(which == d)
        for name, arr in (('r', r), ('r2', r2), ('sse', sse)):
            spread = np.ptp(arr[cols], axis=0).max() / max(1.0, np.abs(arr[cols]).max())
            assert spread <= 1e-12, (d, name, spread)
    first = [int(np.flatnonzero(which == d)[0]) for d in range(nd)]
    want = cv_expected(X, Y, masks, k)
    got = dict(pearson_r_ncomp=r[first].transpose(2, 1, 0), r_squared_ncomp=r2[first].transpose(2, 1, 0),
               mse=sse[first].transpose(2, 1, 0).sum(axis=0) / want['n_test'][None, :])
    got['pearson_r'], got['r_squared'] = got['pearson_r_ncomp'][:, k - 1], got['r_squared_ncomp'][:, k - 1]
    _check(got, want, 'batch of 2304 vs oracle')


def test_large_cohort_s24000_and_several_solver_batches():
    """S = 24 000: the global route by necessity; small scratch budgets cut the 4 splits into several solver batches
    (as test_batches_repeats_and_team_s24000 arranges it for its shape)."""
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, B, T, k = 24000, 300, 3, 2
    X, Y, rs = _design(S, B, T, 5)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=4, test_size=0.25, seed=8, verbose=False)
    one = pls.pls_regression(X, Y, **kw)
    want = cv_expected(X, Y, one.cvres.cvsamples, k)
    _check(one.cvres, want, 'S=24000 vs oracle')
    eng = Engine(scratch_gb=0.1)
    try:
        small = pls.pls_regression(X, Y, _engine=eng, **kw)
    finally:
        eng.close()
    assert np.array_equal(small.cvres.cvsamples, one.cvres.cvsamples)
    _same(one.cvres, small.cvres, ROUTES, 'S=24000 default scratch vs 0.1 GB')
    # at T = 3, k = 2 a split holds 5.8 MB of solver state, dual weights and scores: half of 0.1 GB still takes the 4
    # splits in one batch; half of 0.02 GB takes one split per batch
    eng = Engine(scratch_gb=0.02)
    try:
        tiny = pls.pls_regression(X, Y, _engine=eng, **kw)
    finally:
        eng.close()
    _same(one.cvres, tiny.cvres, ROUTES, 'S=24000 one batch vs four')


def test_missing_rows_and_3d_y_median():
    """NaN rows in X, one subject missing from a 3-D Y, aggfunc='median': masked rows are on neither side."""
    import pypyls_amd as pls
    S, B, T, C, k = 70, 120, 4, 5, 5
    rs = np.random.RandomState(21)
    X = rs.randn(S, B)
    Y = rs.randn(S, T, C) + 0.5 * X[:, :T, None]
    X[[3, 40]] = np.nan
    Y[11] = np.nan
    masks = np.ones((S, 6), dtype=bool)
    for s in range(6):
        masks[rs.choice(S, size=18, replace=False), s] = False
    masks[[3, 11], 0] = [False, True]                        # masked rows sit on both sides of the masks as given
    masks[40, 1] = False
    res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, aggfunc='median', test_split=6,
                             cvsamples=masks, seed=2, verbose=False)
    want = cv_expected(X, np.median(Y, axis=-1), masks, k)
    _check(res.cvres, want, '3-D Y median with NaN rows vs oracle')
    assert np.isfinite(res.cvres.mse).all()


def test_drawn_splits_with_missing_rows():
    """Masks drawn by the call over all S rows; the rows that are NaN throughout drop out of whichever side they fell on."""
    import pypyls_amd as pls
    X, Y, rs = _design(90, 140, 4, 23)
    X[[5, 50, 77]] = np.nan
    Y[20] = np.nan
    res = pls.pls_regression(X, Y, n_components=4, n_perm=0, n_boot=0, test_split=9, test_size=0.3, seed=6, verbose=False)
    masks = res.cvres.cvsamples
    assert masks.shape == (90, 9)
    _check(res.cvres, cv_expected(X, Y, masks, 4), 'drawn splits with NaN rows vs oracle')


def _flat(res, skip=('cvres', 'inputs')):
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
        elif isinstance(fa[key], np.ndarray) and fa[key].dtype == object:
            assert all(np.array_equal(x, y) for x, y in zip(fa[key].ravel(), fb[key].ravel())), key
        else:
            assert np.array_equal(np.asarray(fa[key]), np.asarray(fb[key]), equal_nan=True), (what, key)


def test_leaves_the_rest_alone_and_repeats_to_the_bit():
    import pypyls_amd as pls
    X, Y, rs = _design(120, 300, 6, 31)
    kw = dict(n_components=5, n_perm=40, n_boot=40, seed=4242, verbose=False)
    off = pls.pls_regression(X, Y, test_split=0, **kw)
    assert not off.cvres._filled()
    assert not pls.pls_regression(X, Y, test_split=12, test_size=0, **kw).cvres._filled()
    on = pls.pls_regression(X, Y, test_split=12, **kw)
    again = pls.pls_regression(X, Y, test_split=12, **kw)
    assert np.array_equal(off.permres.permsamples, on.permres.permsamples)
    assert np.array_equal(off.bootres.bootsamples, on.bootres.bootsamples)
    _assert_same_fields(off, on, 'test_split 0 vs 12')
    _assert_same_fields(on, again, 'repeat')
    for key in ('pearson_r', 'r_squared', 'pearson_r_ncomp', 'r_squared_ncomp', 'mse', 'cvsamples'):
        assert np.array_equal(on.cvres[key], again.cvres[key], equal_nan=True), key
    # inputs: test_split / test_size as given (test_size is recorded with test_split = 0 too), the rest the same
    assert on.inputs.test_split == 12 and on.inputs.test_size == 0.25
    assert off.inputs.test_split is None and off.inputs.test_size == 0.25
    for key in ('n_perm', 'n_boot', 'n_split', 'n_components', 'seed', 'rotate', 'ci', 'aggfunc', 'test_size'):
        assert on.inputs.get(key) == off.inputs.get(key), key
    _check(on.cvres, cv_expected(X, Y, on.cvres.cvsamples, 5), 'seeded call vs oracle')


@pytest.mark.parametrize('ids, n_cv', [([0, 0], 7), ([0, 0, 0], 7), ([0, 0, 0], 2)])
def test_sharded_over_a_team(ids, n_cv, monkeypatch):
    """Uneven shards (7 splits over 2 or 3 contexts) and an empty one (2 splits over 3): cvres equals the one-device
    call, the rest equals the same team call without cross-validation, and the call makes ONE data collective."""
    import pypyls_amd as pls
    from pypyls_amd import team as _team
    X, Y, rs = _design(100, 250, 5, 41)
    kw = dict(n_components=4, n_perm=10, n_boot=12, seed=17, verbose=False)
    one = pls.pls_regression(X, Y, test_split=n_cv, **kw)
    calls = []
    orig = _team.Team.allgather

    def counting(self, rank, flat):
        calls.append(rank)
        return orig(self, rank, flat)
    monkeypatch.setattr(_team.Team, 'allgather', counting)
    team_off = pls.pls_regression(X, Y, device_ids=ids, test_split=0, **kw)
    assert sorted(calls) == list(range(len(ids)))
    del calls[:]
    team_on = pls.pls_regression(X, Y, device_ids=ids, test_split=n_cv, **kw)
    print('all-gather calls per rank with cross-validation: {}'.format(sorted(calls)))
    assert sorted(calls) == list(range(len(ids)))            # every rank's thread enters the ONE collective once
    assert np.array_equal(team_on.cvres.cvsamples, one.cvres.cvsamples)
    _same(one.cvres, team_on.cvres, ROUTES, 'team {} of {} splits vs one device'.format(ids, n_cv))
    _assert_same_fields(team_off, team_on, 'team without vs with cross-validation')


def test_save_and_load_round_trip(tmp_path):
    import pypyls_amd as pls
    X, Y, rs = _design(60, 80, 3, 51)
    res = pls.pls_regression(X, Y, n_components=3, n_perm=0, n_boot=0, test_split=5, seed=3, verbose=False)
    back = pls.load_results(pls.save_results(str(tmp_path / 'cv'), res))
    for key in ('pearson_r', 'r_squared', 'pearson_r_ncomp', 'r_squared_ncomp', 'mse', 'cvsamples'):
        assert np.array_equal(back.cvres[key], res.cvres[key]), key
    assert back.cvres.cvsamples.dtype == bool
    assert back.cvres.pearson_r_ncomp.shape == (3, 3, 5) and back.cvres.mse.shape == (4, 5)


def test_abi_refuses_a_context_with_plsc_data():
    """plsx_simpls_crossval_batch on a context bound for behavioral PLS: negative status, a message, and the context
    works afterwards."""
    import torch
    from pypyls_amd.engine import Engine, PLSX_BEHAVIORAL
    X, Y, rs = _design(40, 50, 3, 61)
    eng = Engine()
    try:
        eng.set_data(X, Y, np.zeros(40, np.int32), 1, 1, PLSX_BEHAVIORAL)
        dm = torch.ones((2, 40), dtype=torch.uint8, device=eng.device)
        out = [eng._zeros((2, 3, 3)), eng._zeros((2, 3, 3)), eng._zeros((2, 4, 3))]
        rc = eng.lib.plsx_simpls_crossval_batch(eng.ctx, dm.data_ptr(), 2, out[0].data_ptr(), out[1].data_ptr(),
                                                out[2].data_ptr(), eng._stream())
        msg = eng.lib.plsx_last_error(eng.ctx).decode()
        print('status {}: {}'.format(rc, msg))
        assert rc < 0 and 'regression' in msg
        xw, sv, yw = eng.decompose()[:3]
        assert np.isfinite(np.asarray(sv)).all() and np.asarray(sv)[0] > 0
        eng.sync()
    finally:
        eng.close()
