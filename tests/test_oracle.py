"""
Pins oracle/cpu_ref.py against the golden fixtures produced by RUNNING THE
REFERENCE (tests/golden/make_golden.py) and against the reference's own
known-answer numbers.  CPU only.
"""
import numpy as np
import pytest

from conftest import load_golden, golden_names, live_lvs, assert_close, assert_close_per_lv
from oracle import cpu_ref as ref

# oracle (exact thin SVD) vs reference (sklearn randomized_svd, 4 LU-normalised
# power iterations): the reference itself carries ~eps * (s_1/s_k)^9 error in
# small singular directions (5e-8 observed on the 25x75 Matlab fixture), so the
# oracle is pinned at 1e-6 of the array's scale -- 10x inside the 1e-5 bar.
TOL = 1e-6
VTOL = 1e-5        # singular VECTORS of small LVs are noisier in the reference


def _run(g, method):
    kw = dict(method=method, groups=list(g['groups']), n_cond=int(g['n_cond']),
              covariance=bool(g.get('covariance', False)),
              rotate=bool(g.get('rotate', True)),
              mean_centering=int(g.get('mean_centering', 0)),
              permsamples=g.get('ref_permres__permsamples'),
              bootsamples=g.get('ref_bootres__bootsamples'),
              splitsamples=g.get('splitsamples'),
              perm_splitsamples=g.get('perm_splitsamples'))
    if 'ci' in g:
        kw['ci'] = float(g['ci'])
    return ref.run_plsc(g['X'], g.get('Y'), **kw)


def _boots_full_rank(g):
    """True when every bootstrap cross-correlation matrix keeps rank T'
    (needs more than T distinct subjects in every cell); otherwise the
    bootstrap decomposition has null LVs and the reference's rotation is
    noise-defined (oracle.procrustes_live docstring)."""
    if 'Y' not in g:
        return False
    T = g['Y'].shape[1]
    cells = ref.dummy_code(list(g['groups']), int(g['n_cond'])).T.astype(bool)
    boots = g['ref_bootres__bootsamples']
    return all(len(np.unique(boots[c, i])) - 1 >= T
               for i in range(boots.shape[1]) for c in cells)


def _check(g, out):
    keep = live_lvs(g['ref_singvals'])
    assert_close(out['singvals'][keep], g['ref_singvals'][keep], TOL, what='singvals')
    assert_close(out['varexp'][keep], g['ref_varexp'][keep], TOL, what='varexp')
    for k in ('x_weights', 'y_weights', 'x_scores', 'y_scores', 'y_loadings'):
        if 'ref_' + k in g:
            assert_close(out[k][:, keep], g['ref_' + k][:, keep], VTOL, what=k)
    if 'ref_permres__perm_singval' in g:
        assert_close(out['permres']['perm_singval'][keep],
                     g['ref_permres__perm_singval'][keep], TOL, what='perm_singval')
        # p-values: integer counts must agree exactly (strict '>', +1 smoothing)
        P = g['ref_permres__perm_singval'].shape[1]
        np.testing.assert_array_equal(
            np.rint(out['permres']['pvals'][keep] * (P + 1)),
            np.rint(g['ref_permres__pvals'][keep] * (P + 1)))
    if 'ref_bootres__x_weights_normed' in g:
        full_rank = bool(np.all(keep)) and _boots_full_rank(g)
        for k in ('x_weights_normed', 'x_weights_stderr'):
            a, b = out['bootres'][k][:, keep], g['ref_bootres__' + k][:, keep]
            if full_rank:
                assert_close(a, b, VTOL, what=k)
            else:
                # rank-deficient (mean-centred) decomposition: the reference's
                # rotated bootstrap vectors depend on noise-defined null-space
                # singular vectors (oracle docstring of procrustes_live), so
                # only a 'functional equivalence' bar in the spirit of the
                # reference's Matlab comparator (column correlation,
                # pyls/tests/matlab.py:35-80) applies; 0.9 because these
                # fixtures use only 20-40 bootstraps.
                r = ref.efficient_corr(a, b)
                assert np.all(r >= 0.9), (k, r)
        for k in ('y_loadings_boot', 'y_loadings_ci', 'contrast', 'contrast_boot',
                  'contrast_ci'):
            if 'ref_bootres__' + k in g:
                assert_close(out['bootres'][k][:, keep],
                             g['ref_bootres__' + k][:, keep], VTOL, what=k)
    if 'ref_splitres__ucorr' in g:
        for k in ('ucorr', 'vcorr', 'ucorr_lolim', 'ucorr_uplim', 'vcorr_lolim',
                  'vcorr_uplim'):
            assert_close(out['splitres'][k][keep], g['ref_splitres__' + k][keep],
                         TOL, what=k)
        for k in ('ucorr_pvals', 'vcorr_pvals'):
            np.testing.assert_allclose(out['splitres'][k][keep],
                                       g['ref_splitres__' + k][keep], atol=1e-12)


@pytest.mark.parametrize('name', golden_names('bpls_') + ['linnerud']
                         + golden_names('mat_bpls'))
def test_behavioral_vs_reference(name):
    g = load_golden(name)
    _check(g, _run(g, 'behavioral'))


@pytest.mark.parametrize('name', golden_names('mpls_') + golden_names('mat_mpls'))
def test_meancentered_vs_reference(name):
    g = load_golden(name)
    _check(g, _run(g, 'meancentered'))


@pytest.mark.parametrize('name', ['bpls_cv', 'bpls_2g2c_cv', 'bpls_cv_cov'])
def test_crossval_vs_reference(name):
    """BehavioralPLS.crossval / compute.rescale_test restatement."""
    g = load_golden(name)
    spec = ref.Spec('behavioral', list(g['groups']), int(g['n_cond']), bool(g.get('covariance', False)))
    r, r2 = ref.crossval(spec, g['X'], g['Y'], g['cv_splits'])
    assert_close(r, g['ref_cvres__pearson_r'], 1e-9, what='pearson_r')
    assert_close(r2, g['ref_cvres__r_squared'], 1e-9, what='r_squared')


def test_linnerud_doctest_numbers():
    """docs/user_guide/behavioral.rst:146-149,203-206,218-221,240-245."""
    g = load_golden('linnerud')
    R = ref.xcorr(g['X'], g['Y'])
    want = np.array([[-0.38969365, -0.49308365, -0.22629556],
                     [-0.55223213, -0.64559803, -0.19149937],
                     [0.15064802, 0.22503808, 0.03493306]])
    np.testing.assert_allclose(R, want, atol=1e-8)
    U, d, V = ref.svd(R)
    np.testing.assert_allclose(U[:, 0], [0.61330742, 0.7469717, 0.25668519], atol=1e-8)
    np.testing.assert_allclose(V[:, 0], [-0.58989118, -0.77134059, 0.23887675], atol=1e-8)
    assert abs(np.diag(ref.varexp(d))[0] - 0.9947) < 5e-5
    r = np.corrcoef((g['X'] @ U)[:, 0], (g['Y'] @ V)[:, 0])[0, 1]
    assert abs(r - 0.4900) < 5e-5
    # numbers observed when running the reference
    np.testing.assert_allclose(g['ref_singvals'],
                               [1.1280186599, 0.0752124667, 0.0332524411], atol=1e-9)
    np.testing.assert_allclose(g['ref_permres__pvals'],
                               [0.0495049505, 0.9306930693, 1.0], atol=1e-9)


@pytest.mark.parametrize('name', golden_names('mat_'))
def test_matlab_equivalence(name):
    """The reference's own Matlab comparison (pyls/tests/matlab.py:108-199):
    atol=1e-4 sign-flip-tolerant equality on the shared top-level arrays,
    LVs with singvals ~ 0 masked."""
    g = load_golden(name)
    method = 'behavioral' if 'bpls' in name else 'meancentered'
    out = _run(g, method)
    keep = ~np.isclose(out['singvals'], 0)      # pyls/tests/matlab.py:160
    for k in ('x_weights', 'singvals', 'y_weights', 'x_scores', 'y_scores', 'y_loadings'):
        if 'matlab_' + k not in g:
            continue
        a, b = np.asarray(out[k]), np.asarray(g['matlab_' + k])
        a, b = (a[keep], b[keep]) if a.ndim == 1 else (a[:, keep], b[:, keep])
        if a.ndim == 2:
            flip = np.sign(np.sum(a * b, axis=0, keepdims=True))
            b = b * flip
        np.testing.assert_allclose(a, b, atol=1e-4, err_msg=k)


def test_kernels_known_answers():
    """pyls/tests/test_compute.py:10-49."""
    rs = np.random.RandomState(1234)
    X = rs.rand(20, 200)
    assert np.allclose(np.linalg.norm(ref.normalize(X, axis=0), axis=0), 1)
    assert np.allclose(np.linalg.norm(ref.normalize(X, axis=1), axis=1), 1)
    assert ref.xcorr(rs.rand(20, 200), rs.rand(20, 25)).shape == (25, 200)
    with pytest.raises(ValueError):
        ref.xcorr(rs.rand(20, 200), rs.rand(19, 25))
    assert ref.efficient_corr(rs.rand(100, 10), rs.rand(100, 10)).shape == (10,)
    with pytest.raises(ValueError):
        ref.efficient_corr(rs.rand(100, 10), rs.rand(100, 5))
    np.testing.assert_allclose(
        ref.efficient_corr(np.array([[1., 2.], [2., 1.], [3., 0.]]),
                           np.array([[1., 2.], [2., 3.], [3., 4.]])), [1, -1])
    # dummy coding layout (pyls/tests/test_utils.py)
    assert ref.dummy_code([2, 3], 2).shape == (10, 4)
    np.testing.assert_array_equal(ref.dummy_label([2, 1], 2), [1, 1, 2, 2, 3, 4])


@pytest.mark.parametrize('tag', ['t4', 't8'])
def test_simpls_vs_reference(tag):
    """T <= 11: the reference's rank-1 randomized SVD is exact."""
    g = load_golden('simpls_' + tag)
    out = ref.run_regression(g['X'], g['Y'], int(g['n_components']),
                             permsamples=g['permsamples'],
                             bootsamples=g['ref_bootres__bootsamples'])
    for k in ('x_weights', 'x_scores', 'y_scores', 'y_loadings', 'varexp'):
        assert_close(out[k], g['ref_' + k], TOL, what=k)
    assert_close(out['permres']['perm_singval'], g['ref_perm_varexp'], 1e-8,
                 what='perm varexp')
    for k in ('x_weights_normed', 'x_weights_stderr', 'y_loadings_boot', 'y_loadings_ci'):
        assert_close(out['bootres'][k], g['ref_bootres__' + k], TOL, what=k)


@pytest.mark.parametrize('agg', ['mean', 'median'])
def test_simpls_3d_vs_reference(agg):
    g = load_golden('simpls_3d_' + agg)
    n = g['boot_subjects'].shape[1]
    bs = np.empty((2, n), dtype=object)
    for i in range(n):
        bs[0, i], bs[1, i] = g['boot_subjects'][:, i], g['boot_third'][:, i]
    out = ref.run_regression(g['X'], g['Y'], int(g['n_components']), bootsamples=bs, aggfunc=agg)
    for k in ('x_weights', 'x_scores', 'y_scores', 'y_loadings', 'varexp'):
        assert_close(out[k], g['ref_' + k], 1e-9, what=k)
    for k in ('x_weights_normed', 'x_weights_stderr', 'y_loadings_boot', 'y_loadings_ci'):
        assert_close(out['bootres'][k], g['ref_bootres__' + k], 1e-9, what=k)


def test_simpls_nan_rows_vs_reference():
    g = load_golden('simpls_nan')
    out = ref.run_regression(g['X'], g['Y'], 3, permsamples=g['permsamples'],
                             bootsamples=g['ref_bootres__bootsamples'])
    for k in ('x_weights', 'x_scores', 'y_scores', 'y_loadings', 'varexp'):
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(g['ref_' + k]))
        assert_close(np.nan_to_num(out[k]), np.nan_to_num(g['ref_' + k]), 1e-9, what=k)
    assert_close(out['permres']['perm_singval'], g['ref_perm_varexp'], 1e-9, what='perm')
    for k in ('x_weights_normed', 'y_loadings_boot'):
        assert_close(out['bootres'][k], g['ref_bootres__' + k], 1e-9, what=k)


def test_simpls_wide_is_unpinned_but_close():
    """T = 16 > 11: the reference's top singular vector is approximate and
    seed dependent; the exact restatement must still be close."""
    g = load_golden('simpls_t16')
    out = ref.run_regression(g['X'], g['Y'], int(g['n_components']))
    assert_close(out['varexp'], g['ref_varexp'], 5e-2, what='varexp (approximate ref)')


def test_simpls_3d_with_nan_rows_vs_reference():
    """3-D Y together with all-NaN rows of X and of Y (masked per bootstrap after the
    third axis is aggregated, regression.py:308-313)."""
    g = load_golden('simpls_3d_nan')
    n = g['boot_subjects'].shape[1]
    bs = np.empty((2, n), dtype=object)
    for i in range(n):
        bs[0, i], bs[1, i] = g['boot_subjects'][:, i], g['boot_third'][:, i]
    out = ref.run_regression(g['X'], g['Y'], int(g['n_components']), bootsamples=bs, aggfunc='mean')
    for k in ('x_weights', 'x_scores', 'y_scores', 'y_loadings', 'varexp'):
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(g['ref_' + k]))
        assert_close(np.nan_to_num(out[k]), np.nan_to_num(g['ref_' + k]), 1e-9, what=k)
    for k in ('x_weights_normed', 'x_weights_stderr', 'y_loadings_boot', 'y_loadings_ci'):
        assert_close(out['bootres'][k], g['ref_bootres__' + k], 1e-9, what=k)


def test_simpls_t20_oracle_within_the_reference_seed_envelope():
    """T = 20 > 11 (the regime of BASELINE config c5): the reference's rank-1 randomized SVD
    (regression.py:103) is approximate and seed dependent, so there is no single reference
    answer to pin.  tests/golden/simpls_t20_seeds.npz holds the reference's own x_weights /
    pctvar for seeds 0, 1, 2 on one design; the exact restatement must lie INSIDE the spread
    the reference shows against itself: for every component, the distance oracle <-> run is
    at most the largest run <-> run distance.  Measured: weights
    3.7e-3 vs 4.1e-3 relative (max over components), pctvar of Y 4.2e-4 vs 5.1e-4."""
    g = load_golden('simpls_t20_seeds')
    X, Y, k = g['X'], g['Y'], int(g['n_components'])
    out = ref.simpls(X, Y, k)
    W = [g['ref_x_weights_seed{}'.format(s)] for s in (0, 1, 2)]
    P = [g['ref_pctvar_y_seed{}'.format(s)] for s in (0, 1, 2)]

    def coldist(A, B):
        sg = np.sign(np.sum(A * B, axis=0))
        return np.max(np.abs(A * sg - B), axis=0) / np.max(np.abs(B), axis=0)
    ow = np.max([coldist(out['x_weights'], w) for w in W], axis=0)
    ww = np.max([coldist(W[a], W[b]) for a in range(3) for b in range(a + 1, 3)], axis=0)
    op = np.max([np.abs(np.asarray(out['pctvar'])[1] - p) / p for p in P], axis=0)
    pp = np.max([np.abs(P[a] - P[b]) / P[b] for a in range(3) for b in range(a + 1, 3)], axis=0)
    assert np.all(ow <= ww), (ow, ww)
    assert np.all(op <= pp), (op, pp)
    assert ww.max() < 1e-2 and pp.max() < 2e-3              # the envelope itself is what was recorded
    assert ow.max() > 1e-6                                  # and it is NOT a 1e-9 pin: "parity unpinned" stays


def _mpls_envelope(tag):
    """Reference runs (analysis seeds 0 .. 5) of tests/golden/seeds_mpls.npz for design ``tag`` and the oracle's
    rotated bootstrap vectors of the same six bootstraps; distances are column-wise relative 2-norms."""
    g = load_golden('seeds_mpls')
    X, groups = g[tag + '_X'], [int(v) for v in g[tag + '_groups']]
    spec = ref.Spec('meancentered', groups, int(g[tag + '_n_cond']), mean_centering=int(g[tag + '_mean_centering']))
    seeds = [int(s) for s in g[tag + '_seeds']]
    runs = np.array([g['{}_ref_uboot_seed{}'.format(tag, s)] for s in seeds])      # (seed, B, L, boot)
    sv = g[tag + '_singvals']
    d0 = np.diag(sv) if sv.ndim == 2 else sv
    live = live_lvs(d0)
    boots = g[tag + '_bootsamples']
    mine = np.stack([ref.single_boot(spec, X, spec.dummy, boots[:, i], g[tag + '_x_weights'], d_orig=np.diag(d0))[1]
                     for i in range(boots.shape[1])], -1)

    def dist(A, B):
        return np.linalg.norm(A - B, axis=0) / np.linalg.norm(A, axis=0)            # (L, boot)
    pairs = [dist(runs[a], runs[b]) for a in range(len(seeds)) for b in range(a + 1, len(seeds))]
    return g, spec, live, runs, mine, dist, np.max(pairs, axis=0)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_mpls_oracle_against_the_reference_seed_envelope(tag):
    """Rank-deficient Procrustes (mean-centred PLS, BASELINE config c3's method) has no 1e-5-reproducible reference
    answer: compute.procrustes (compute.py:260) multiplies the NULL-space singular vectors randomized_svd happens to
    return -- of the original and of every bootstrap -- into the polar factor, so BasePLS._single_boot
    (base.py:530-574) returns rotated vectors that move with the analysis seed.  tests/golden/seeds_mpls.npz holds
    the reference's own runs for seeds 0 .. 5 on two committed designs (3 groups x 2 conditions: 3 live LVs of 6;
    2 x 2: 2 live of 4): they differ from EACH OTHER by up to 2.2 % / 6.2 % / 18 % (design a, per live LV) and 2.9 % /
    4.5 % (design b).  The oracle (procrustes_live: live LVs against live LVs only -- the deliberate deviation of
    DESIGN.md section 3) is as far from any reference run as the reference is from itself: measured, its largest
    distance to a run is 1.11 / 1.21 / 0.83 (a) and 1.00 / 1.11 (b) times the largest run-to-run distance of that LV,
    at most 1.56 x for a single (LV, bootstrap).  Asserted: <= 1.35 x per LV, <= 2 x per (LV, bootstrap) -- i.e. the
    deviation is the size of the reference's own seed noise, not a 1e-5 pin; null LVs are not compared at all (the
    reference's differ from each other by 100 - 500 %)."""
    g, spec, live, runs, mine, dist, spread = _mpls_envelope(tag)
    od = np.max([dist(r, mine) for r in runs], axis=0)                              # (L, boot): worst run
    assert live.sum() in (2, 3) and not live.all()
    assert np.all(od[live] <= 2.0 * spread[live]), (od[live] / spread[live]).max()
    assert np.all(od[live].max(axis=1) <= 1.35 * spread[live].max(axis=1)), (od[live].max(1), spread[live].max(1))
    assert 0.01 < spread[live].max() < 0.25                 # the envelope itself is percents wide ...
    assert spread[~live].min() > 0.5                        # ... and the null columns are noise in the reference itself
    assert od[live].max() > 1e-3                            # not a tight pin: the deviation stays documented as one
    # the live columns of the ORIGINAL decomposition do not depend on the seed (only its null columns do)
    o = [g['{}_ref_original_seed{}'.format(tag, s)] for s in (0, 3)]
    assert np.abs(o[0][:, live] - o[1][:, live]).max() < 1e-12 and np.abs(o[0][:, ~live] - o[1][:, ~live]).max() > 1e-3


def _resamples(groups, n_cond, n, seed):
    """Within-cell permutation and bootstrap index arrays (S, n) drawn here, independent of the product."""
    rs = np.random.RandomState(seed)
    cells = np.split(np.arange(sum(groups) * n_cond), np.cumsum(np.repeat(groups, n_cond))[:-1])
    perms = np.stack([rs.permutation(sum(groups) * n_cond) for _ in range(n)], -1)
    boots = np.stack([np.concatenate([rs.choice(c, len(c)) for c in cells]) for _ in range(n)], -1)
    return perms, boots


@pytest.mark.parametrize('shape', ['c2', 'rank_deficient', 'cells_cov', 'no_rotate'])
def test_batched_oracle_equals_single_resample_oracle(shape):
    """batch_perm / batch_boot (the oracle of every resample of a c2-sized series, tests/test_gpu_timed_geometry.py)
    restate single_perm / single_boot over chunks of resamples: same arrays to 1e-12 of every LV's own scale, at the
    c2 shape (64 resamples, several chunks), at a rank-deficient shape (S - 1 < T': exactly-null LVs, live-LV
    Procrustes), with several cells in covariance mode, and without rotation."""
    S, B, T, groups, n_cond, n, cov, rot = dict(
        c2=(80, 10000, 10, [80], 1, 64, False, True),
        rank_deficient=(12, 40, 16, [12], 1, 6, False, True),
        cells_cov=(36, 300, 4, [10, 8], 2, 9, True, True),
        no_rotate=(40, 500, 6, [40], 1, 7, False, False))[shape]
    rs = np.random.RandomState(5)
    X = rs.randn(S, B) * (1.0 + rs.rand(1, B))
    Y = rs.randn(S, T) + 0.3 * X[:, :T]
    spec = ref.Spec('behavioral', groups, n_cond, covariance=cov, rotate=rot)
    U, d, V = ref.decompose(spec, X, Y)
    live = ref.live_lvs(d)
    assert live.all() == (shape != 'rank_deficient')
    perms, boots = _resamples(groups, n_cond, n, seed=6)
    old = ref.BATCH_BYTES
    ref.BATCH_BYTES = 8 * T * n_cond * len(groups) * B * 5        # five resamples per chunk: chunk edges are crossed
    try:
        got_p = ref.batch_perm(spec, X, Y, perms, V)
        got_d, got_u = ref.batch_boot(spec, X, Y, boots, U, d)
        sum_d, got_s, got_q = ref.batch_boot(spec, X, Y, boots, U, d, sums=True)
    finally:
        ref.BATCH_BYTES = old
    want_p = np.stack([ref.single_perm(spec, X, Y, perms[:, i], V)[0] for i in range(n)], -1)
    single = [ref.single_boot(spec, X, Y, boots[:, i], U, d) for i in range(n)]
    want_d = np.stack([s[0] for s in single], -1)
    want_u = np.stack([s[1] for s in single], -1)
    assert got_p.shape == want_p.shape and got_d.shape == want_d.shape and got_u.shape == want_u.shape
    for i in range(n):
        assert_close(got_p[:, i], want_p[:, i], 1e-12, what='batched perm {}'.format(i))
        assert_close_per_lv(got_d[..., i], want_d[..., i], 1, 1e-12, keep=live, what='batched distrib {}'.format(i))
        assert_close_per_lv(got_u[..., i], want_u[..., i], 1, 1e-12, keep=live, what='batched U_boot {}'.format(i))
    assert np.all(got_u[:, ~live] == 0)
    assert np.array_equal(sum_d, got_d)
    assert_close_per_lv(got_s, want_u.sum(-1), 1, 1e-12, keep=live, what='batched sum U')
    assert_close_per_lv(got_q, (want_u ** 2).sum(-1), 1, 1e-12, keep=live, what='batched sum U^2')
    with pytest.raises(ValueError):
        ref.batch_perm(ref.Spec('meancentered', groups, n_cond), X, spec.dummy, perms, V)
