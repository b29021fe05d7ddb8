"""SIMPLS regression past the on-chip bound on S (the global route of the component-step kernels,
csrc/plsx_simpls.h, GL = true): forced on every SIMPLS golden, and chosen by itself for S = 24 000 and
S = 48 000 (S^2 > 2^31), against the reference, the oracle and the on-chip route."""
import numpy as np
import pytest

from conftest import load_golden, assert_close
from oracle import cpu_ref as ref

pytestmark = pytest.mark.gpu
RTOL = 1e-5
BOOT_KEYS = ('x_weights_normed', 'x_weights_stderr', 'y_loadings_boot', 'y_loadings_ci')


def _global_engine(**kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1}, **kw)


def _boot3(g):
    n = g['boot_subjects'].shape[1]
    bs = np.empty((2, n), dtype=object)
    for i in range(n):
        bs[0, i], bs[1, i] = g['boot_subjects'][:, i], g['boot_third'][:, i]
    return bs


def _same_route_stats(a, b, rtol=1e-12, sums_rtol=1e-12):
    """The two runs do the same arithmetic up to the summation order of the products with K.  ``sums_rtol``: the
    standard errors come from sums of squares over the bootstraps (E w^2 - (E w)^2), which turn a last-bit change of
    the weights into ~1e-11 of the ratios (the team tests of test_gpu_team.py allow 1e-9 there)."""
    assert_close(a['varexp'], b['varexp'], rtol, what='varexp')
    if a['permres'].get('pvals') is not None:
        assert_close(a['permres']['perm_singval'], b['permres']['perm_singval'], rtol, what='perm_singval')
        np.testing.assert_array_equal(a['permres']['pvals'], b['permres']['pvals'])
    for key in BOOT_KEYS:
        tol = sums_rtol if key in ('x_weights_normed', 'x_weights_stderr') else rtol
        assert_close(a['bootres'][key], b['bootres'][key], tol, what=key)


@pytest.mark.parametrize('tag', ['t4', 't8', 't16', 'nan'])
def test_forced_global_route_on_2d_goldens(tag):
    import pypyls_amd as pls
    g = load_golden('simpls_' + tag)
    k = int(g['n_components'])
    kw = dict(n_components=k, n_perm=g['permsamples'].shape[1], n_boot=g['ref_bootres__bootsamples'].shape[1],
              permsamples=g['permsamples'], bootsamples=g['ref_bootres__bootsamples'], seed=1234, verbose=False)
    res = pls.pls_regression(g['X'], g['Y'], _engine=_global_engine(), **kw)
    want = ref.run_regression(g['X'], g['Y'], k, permsamples=g['permsamples'],
                              bootsamples=g['ref_bootres__bootsamples'])
    for key in ('x_weights', 'x_scores', 'y_scores', 'y_loadings', 'varexp'):
        np.testing.assert_array_equal(np.isnan(res[key]), np.isnan(want[key]))
        assert_close(np.nan_to_num(res[key]), np.nan_to_num(want[key]), RTOL, what='oracle ' + key)
    assert_close(res['permres']['perm_singval'], want['permres']['perm_singval'], RTOL, what='oracle perm')
    np.testing.assert_array_equal(res['permres']['pvals'], want['permres']['pvals'])
    for key in BOOT_KEYS:
        assert_close(res['bootres'][key], want['bootres'][key], RTOL, what='oracle ' + key)
    if tag != 't16':                           # T <= 11: the reference's rank-1 randomized SVD is exact
        for key in ('x_weights', 'x_scores', 'y_scores', 'y_loadings', 'varexp'):
            assert_close(np.nan_to_num(res[key]), np.nan_to_num(g['ref_' + key]), RTOL, what='reference ' + key)
        assert_close(res['permres']['perm_singval'], g['ref_perm_varexp'], RTOL, what='reference perm')
        for key in BOOT_KEYS:
            assert_close(res['bootres'][key], g['ref_bootres__' + key], RTOL, what='reference ' + key)
    _same_route_stats(res, pls.pls_regression(g['X'], g['Y'], **kw))


@pytest.mark.parametrize('tag', ['3d_mean', '3d_median', '3d_nan'])
def test_forced_global_route_on_3d_goldens(tag):
    import pypyls_amd as pls
    g = load_golden('simpls_' + tag)
    bs = _boot3(g)
    kw = dict(n_components=int(g['n_components']), n_perm=0, n_boot=bs.shape[1], bootsamples=bs,
              aggfunc=tag[3:] if tag != '3d_nan' else 'mean', seed=1234, verbose=False)
    res = pls.pls_regression(g['X'], g['Y'], _engine=_global_engine(), **kw)
    for key in ('x_weights', 'x_scores', 'y_scores', 'y_loadings', 'varexp'):
        np.testing.assert_array_equal(np.isnan(res[key]), np.isnan(g['ref_' + key]))
        assert_close(np.nan_to_num(res[key]), np.nan_to_num(g['ref_' + key]), RTOL, what=key)
    for key in BOOT_KEYS:
        assert_close(res['bootres'][key], g['ref_bootres__' + key], RTOL, what=key)
    _same_route_stats(res, pls.pls_regression(g['X'], g['Y'], **kw))


def _cohort(S, B, T, seed, nan_rows=()):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = X[:, :T] * np.linspace(3.0, 1.0, T) + rs.randn(S, T)
    for i in nan_rows:
        X[i] = np.nan
    return X, Y, rs


def _check_oracle(res, want, tol=1e-8, boot=True):
    for key in ('x_weights', 'varexp'):
        assert_close(res[key], want[key], tol, what=key)
    assert_close(res['permres']['perm_singval'], want['permres']['perm_singval'], tol, what='perm_singval')
    np.testing.assert_array_equal(res['permres']['pvals'], want['permres']['pvals'])
    if boot:
        for key in ('x_weights_normed', 'y_loadings_ci'):
            assert_close(res['bootres'][key], want['bootres'][key], tol, what=key)


def test_past_the_onchip_bound_s24000():
    """S = 24 000, T = 10, k = 10: the on-chip slice would need 193 KB of LDS (plsx_set_data refused the shape)."""
    import pypyls_amd as pls
    S, B, T, k = 24000, 2000, 10, 10
    X, Y, rs = _cohort(S, B, T, 11)
    perms = np.stack([rs.permutation(S) for _ in range(8)], axis=1)
    boots = rs.randint(0, S, size=(S, 8))
    res = pls.pls_regression(X, Y, n_components=k, n_perm=8, n_boot=8, permsamples=perms, bootsamples=boots,
                             seed=5, verbose=False)
    _check_oracle(res, ref.run_regression(X, Y, k, permsamples=perms, bootsamples=boots))


def test_k_indexing_past_2_31_s48000():
    """S = 48 000: S^2 = 2.3e9 entries of K, past 32-bit indexing."""
    import pypyls_amd as pls
    S, B, T, k = 48000, 400, 4, 3
    X, Y, rs = _cohort(S, B, T, 12)
    perms = np.stack([rs.permutation(S) for _ in range(4)], axis=1)
    boots = rs.randint(0, S, size=(S, 4))
    res = pls.pls_regression(X, Y, n_components=k, n_perm=4, n_boot=4, permsamples=perms, bootsamples=boots,
                             seed=5, verbose=False)
    _check_oracle(res, ref.run_regression(X, Y, k, permsamples=perms, bootsamples=boots))


def test_nan_rows_and_3d_y_s24000():
    import pypyls_amd as pls
    S, B, T, k, C = 24000, 300, 3, 2, 3
    X, Y2, rs = _cohort(S, B, T, 13, nan_rows=(7, 5000, 23999))
    # all-NaN rows: X rows above, and one subject missing from Y altogether
    Y2[100] = np.nan
    perms = np.stack([rs.permutation(S) for _ in range(3)], axis=1)
    boots = rs.randint(0, S, size=(S, 3))
    res = pls.pls_regression(X, Y2, n_components=k, n_perm=3, n_boot=3, permsamples=perms, bootsamples=boots,
                             seed=5, verbose=False)
    want = ref.run_regression(X, Y2, k, permsamples=perms, bootsamples=boots)
    for key in ('x_weights', 'varexp'):
        assert_close(res[key], want[key], 1e-8, what='NaN rows ' + key)
    assert np.isnan(res['x_scores'][7]).all()
    assert_close(res['permres']['perm_singval'], want['permres']['perm_singval'], 1e-8, what='NaN rows perm')
    for key in ('x_weights_normed', 'y_loadings_ci'):
        assert_close(res['bootres'][key], want['bootres'][key], 1e-8, what='NaN rows ' + key)
    # 3-D Y (subjects and the third axis resampled)
    Y3 = Y2[..., None] + 0.3 * rs.randn(S, T, C)
    third = rs.randint(0, C, size=(C, 3))
    bs = np.empty((2, 3), dtype=object)
    for i in range(3):
        bs[0, i], bs[1, i] = boots[:, i], third[:, i]
    res = pls.pls_regression(X, Y3, n_components=k, n_perm=0, n_boot=3, bootsamples=bs, seed=5, verbose=False)
    want = ref.run_regression(X, Y3, k, bootsamples=bs)
    for key in ('x_weights', 'varexp'):
        assert_close(res[key], want[key], 1e-8, what='3-D ' + key)
    for key in ('x_weights_normed', 'y_loadings_ci'):
        assert_close(res['bootres'][key], want['bootres'][key], 1e-8, what='3-D ' + key)


def test_batches_repeats_and_team_s24000():
    """Several solver batches (a small scratch budget) = one batch; a repeat is bit-identical; a team of two
    contexts on one device = one device.  (Batches and shards of other sizes split the products with K into other
    contraction chunks: equal to rounding, not to the bit.)"""
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine
    S, B, T, k = 24000, 500, 10, 10
    X, Y, rs = _cohort(S, B, T, 14)
    kw = dict(n_components=k, n_perm=6, n_boot=40, seed=21, verbose=False)
    one = pls.pls_regression(X, Y, **kw)
    again = pls.pls_regression(X, Y, **kw)
    for key in ('x_weights', 'varexp'):
        assert np.array_equal(one[key], again[key]), key
    assert np.array_equal(one['permres']['perm_singval'], again['permres']['perm_singval'])
    for key in BOOT_KEYS:
        assert np.array_equal(one['bootres'][key], again['bootres'][key]), key
    # half of 0.1 GB holds the solver state of 3 resamples of this shape: 2 permutation batches; the bootstraps go
    # in whole groups of 38 (one group per batch): 2 batches
    small = pls.pls_regression(X, Y, _engine=Engine(scratch_gb=0.1), **kw)
    _same_route_stats(one, small, sums_rtol=1e-9)
    team = pls.pls_regression(X, Y, device_ids=[0, 0], **kw)
    _same_route_stats(one, team, sums_rtol=1e-9)


def test_refuses_k_beyond_device_memory():
    import pypyls_amd as pls
    from pypyls_amd.engine import PlsxError
    rs = np.random.RandomState(0)
    S = 300000                                   # K: 720 GB
    X, Y = rs.randn(S, 3), rs.randn(S, 2)
    with pytest.raises(PlsxError, match='does not fit in the free device memory'):
        pls.pls_regression(X, Y, n_components=1, n_perm=0, n_boot=0, verbose=False)
