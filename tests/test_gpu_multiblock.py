"""Multiblock PLS on the device (PLSX_MULTIBLOCK: both A-operand builders in one group, k_mb_rownorm / k_mb_rowscale)
against the numpy definition of tests/multiblock_expect.py.

Tolerances (the project's, tests/test_gpu_nonrotated.py): values derived from R (R itself, singular values, weights,
permuted statistics) 1e-10 of their own LV's or row's scale, the gen_distrib columns 1e-9, the bootstrap sums and what
is computed from them 1e-8 per live LV (oracle live_lvs).  P-values are compared as exact integer counts; every fixture
first asserts ON THE EXPECTATION that no permuted value lies within 1e-6 (relative) of the observed one.

Bit identity is asked of everything that belongs to ONE resample (its R, its permuted statistic, its gen_distrib
columns); the bootstrap SUMS are added batch by batch (k_urot) and rank by rank for every method, so they are compared
as values (tests/test_gpu_team.py says the same of the other methods).  The Gram pass cuts the features into chunks
whose number follows the batch once B >= 1024 (plsx_gram.hip, every method): the permuted statistics are compared bit
for bit at B = 1003, the largest B of the cases, and R itself -- the pass this method adds -- at a B of three chunks."""
import numpy as np
import pytest

import multiblock_expect as mb

pytestmark = pytest.mark.gpu

TOL_R, TOL_DIST, TOL_SUM = 1e-10, 1e-9, 1e-8
METHOD = 3
# name: (groups, n_cond, T, mean_centering, B of the decomposition cases)
DESIGNS = {
    'tp16_mc0': ([7, 9], 2, 3, 0, 129),                  # T' = 16: tile-exact
    'tp9_mc0': ([12], 3, 2, 0, 127),
    'tp15_mc1': ([6, 5, 8], 1, 4, 1, 128),
    'tp24_mc2': ([10, 11], 2, 5, 2, 17),                 # L = B < T'
    'tp44_mc0': ([30, 30], 2, 10, 0, 1003),
}
B_CHUNKS = 9000                                          # 4096 + 4096 + 808 columns: three chunks of the norm kernel, the last ragged
BS = (1, 17, 127, 128, 129, 1003, B_CHUNKS)
_ENGINES = {}
_CACHE = {}


def _engine(**options):
    """One engine per option set, kept for the module (a context maps its scratch once)."""
    from pypyls_amd.engine import Engine
    key = tuple(sorted(options.items()))
    if key not in _ENGINES:
        scratch = options.pop('scratch_gb', None)
        _ENGINES[key] = Engine(scratch_gb=scratch, options=options)
    return _ENGINES[key]


def _make(name, B, seed, covariance=False, n_perm=6, n_boot=6):
    """Random data of the design, permutations of the rows, bootstraps within the cells (with repeated rows)."""
    groups, n_cond, T, mc, _ = DESIGNS[name]
    rs = np.random.RandomState(seed)
    specs = mb.specs_of(groups, n_cond, covariance, mc)
    dummy = specs[1].dummy
    S = dummy.shape[0]
    cells = dummy.argmax(axis=1)
    X = rs.randn(S, B) + 0.3 * cells[:, None] * rs.randn(1, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :1]
    perms = np.stack([rs.permutation(S) for _ in range(n_perm)], axis=1)
    boots = np.zeros((S, n_boot), dtype=np.int64)
    for b in range(n_boot):
        for c in range(dummy.shape[1]):
            rows = np.flatnonzero(cells == c)
            while True:
                draw = rs.choice(rows, size=rows.size)
                if 3 <= np.unique(draw).size < rows.size:             # (never a constant cell, always a repeated row)
                    break
            boots[rows, b] = draw
    J = dummy.shape[1]
    return dict(specs=specs, groups=groups, n_cond=n_cond, mc=mc, cov=covariance, X=X, Y=Y, cells=cells, perms=perms,
                boots=boots, J=J, T=T, Tp=J + J * T, key=(name, B, seed, covariance, n_perm, n_boot))


def _set_data(eng, d):
    eng.set_data(d['X'], d['Y'], d['cells'], len(d['groups']), d['n_cond'], METHOD, mean_centering=d['mc'],
                 covariance=d['cov'])
    assert eng.Tp == d['Tp'] and eng.L == min(d['Tp'], d['X'].shape[1])


def _bind(eng, d):
    """set_data, decompose, the sign rule, set_original -> x_weights, singvals, y_weights."""
    from pypyls_amd import hostmath
    _set_data(eng, d)
    xw, sv, yw = eng.decompose()
    xw, yw = hostmath.sign_convention(xw, yw)
    eng.set_original(xw, sv, yw)
    return xw, sv, yw


def _expect(d, rotate=True):
    """The expectation of a fixture, computed once and shared (never modified)."""
    key = (d['key'], rotate)
    if key not in _CACHE:
        specs, X, Y = d['specs'], d['X'], d['Y']
        U, sv, V = mb.original(specs, X, Y)
        sp = mb.perm_singvals(specs, X, Y, V, d['perms'], rotate)
        assert mb.closest_tie(sv, sp) > 1e-6, 'fixture: a permuted value ties with the observed one'
        us, uq, dist = mb.boot_sums(specs, X, Y, U, sv, d['boots'])
        _CACHE[key] = dict(d=d, U=U, sv=sv, V=V, sp=sp, us=us, uq=uq, dist=dist, live=mb.ref.live_lvs(sv),
                           counts=np.sum(sp > sv[:, None], axis=1))
    return _CACHE[key]


def _per_lv(got, want, axis, tol, what, live=None):
    got, want = np.moveaxis(np.asarray(got), axis, 0), np.moveaxis(np.asarray(want), axis, 0)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in range(want.shape[0]):
        if live is not None and not live[k]:
            continue                                                # (a null LV: arbitrary vectors, 0 / 0 loadings)
        assert np.all(np.isfinite(got[k])), what + ': non-finite'
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max()
        assert err <= tol * scale, '{}: {} {}: err {:.3e}, scale {:.3e}, tol {:g}'.format(what, 'row' if live is None else 'LV',
                                                                                        k, err, scale, tol)


# ---- R itself ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(DESIGNS))
@pytest.mark.parametrize('B', BS)
def test_R_is_the_stacked_row_normalised_matrix(name, B):
    """plsx_crosscov_batch of the identity, a permutation (ONE index array in both roles) and bootstraps with repeated
    rows, every row at 1e-10 of its scale (1: unit rows); then the slots themselves: rows >= T' zero, the score columns
    the UNscaled gen_distrib, the padding columns zero."""
    d = _make(name, B, seed=len(name) + B, n_perm=3, n_boot=3)
    specs, X, Y, J, Tp = d['specs'], d['X'], d['Y'], d['J'], d['Tp']
    eng = _engine()
    xw, sv, yw = _bind(eng, d)
    got = eng.crosscov(n=1)[0]
    _per_lv(got, mb.R_mb(specs, X, Y), 0, TOL_R, 'R')
    assert np.abs(np.sqrt((got ** 2).sum(axis=1)) - 1).max() <= 1e-13
    assert abs((sv ** 2).sum() - Tp) <= 1e-10 * Tp                          # unit rows: sum of singvals^2 = T'
    got = eng.crosscov(ysrc=d['perms'])
    for i in range(d['perms'].shape[1]):
        _per_lv(got[i], mb.R_mb(specs, X, Y, perminds=d['perms'][:, i]), 0, TOL_R, 'R of permutation {}'.format(i))
    got = eng.crosscov(xsrc=d['boots'], ysrc=d['boots'])
    for i in range(d['boots'].shape[1]):
        _per_lv(got[i], mb.R_mb(specs, X, Y, bootinds=d['boots'][:, i]), 0, TOL_R, 'R of bootstrap {}'.format(i))
    # the slots of the last batch
    L = eng.L
    for i in range(d['boots'].shape[1]):
        slot = eng.scratch_rows(i)
        assert slot.shape[0] == -(-Tp // 4) * 4
        assert np.all(slot[Tp:] == 0), 'rows >= T\' of a slot must stay zero'
        assert np.all(slot[:, B + L:] == 0), 'padding columns'
        assert np.array_equal(slot[:Tp, :B], got[i])
        inds = d['boots'][:, i]
        want = mb.distrib(specs, X[inds], Y[inds], xw)
        _per_lv(slot[:Tp, B:B + L], want, 1, TOL_DIST, 'score columns (unscaled gen_distrib)', live=mb.ref.live_lvs(sv))


def test_R_in_covariance_mode():
    d = _make('tp16_mc0', 129, seed=31, covariance=True, n_perm=2, n_boot=2)
    specs, X, Y = d['specs'], d['X'], d['Y']
    eng = _engine()
    _bind(eng, d)
    _per_lv(eng.crosscov(n=1)[0], mb.R_mb(specs, X, Y), 0, TOL_R, 'R')
    got = eng.crosscov(ysrc=d['perms'])
    for i in range(2):
        _per_lv(got[i], mb.R_mb(specs, X, Y, perminds=d['perms'][:, i]), 0, TOL_R, 'R of permutation {}'.format(i))
    got = eng.crosscov(xsrc=d['boots'], ysrc=d['boots'])
    for i in range(2):
        _per_lv(got[i], mb.R_mb(specs, X, Y, bootinds=d['boots'][:, i]), 0, TOL_R, 'R of bootstrap {}'.format(i))


# ---- decomposition, permutations, bootstraps ---------------------------------------------------------------------

def _check_all(eng, d, want, want_plain):
    Tp = d['Tp']
    live = want['live']
    xw, sv, yw = _bind(eng, d)
    _per_lv(sv, want['sv'], 0, TOL_R, 'singvals', live=live)
    _per_lv(xw, want['U'], 1, TOL_R, 'x_weights', live=live)
    _per_lv(yw, want['V'], 1, TOL_R, 'y_weights', live=live)
    assert abs((sv ** 2).sum() - Tp) <= 1e-10 * Tp
    for rotate, w in ((True, want), (False, want_plain)):
        sp = eng.perm(d['perms'], rotate=rotate)
        _per_lv(sp, w['sp'], 0, TOL_R, 'perm_singval (rotate={})'.format(rotate), live=live)
        assert np.array_equal(np.sum(sp > sv[:, None], axis=1)[live], w['counts'][live])
    us, uq, dist = eng.boot(d['boots'])
    us, uq = us.cpu().numpy(), uq.cpu().numpy()
    _per_lv(dist, want['dist'], 1, TOL_DIST, 'distrib', live=live)
    _per_lv(us, want['us'], 1, TOL_SUM, 'sum of U_b', live=live)
    _per_lv(uq, want['uq'], 1, TOL_SUM, 'sum of U_b^2', live=live)
    n = d['boots'].shape[1]
    bs = want['U'] * want['sv']
    _, se_w = mb.ref.boot_rel(bs, want['us'] + bs, want['uq'] + bs ** 2, n + 1)
    _, se_g = mb.ref.boot_rel(bs, us + bs, uq + bs ** 2, n + 1)
    _per_lv(se_g, se_w, 1, TOL_SUM, 'standard error', live=live)
    return dict(sp=sp, us=us, uq=uq, dist=dist)


@pytest.mark.parametrize('name', sorted(DESIGNS))
def test_decomposition_permutations_bootstraps(name):
    d = _make(name, DESIGNS[name][4], seed=40 + len(name))
    _check_all(_engine(), d, _expect(d, True), _expect(d, False))


def test_decomposition_in_covariance_mode_and_three_chunks():
    d = _make('tp9_mc0', B_CHUNKS, seed=51, covariance=True, n_perm=4, n_boot=4)
    _check_all(_engine(), d, _expect(d, True), _expect(d, False))


# ---- batch independence ------------------------------------------------------------------------------------------

def test_same_bits_whatever_the_batch():
    """One batch, a scratch budget of one group per launch, a small min_batch: R (three chunks of the norm kernel), the
    permuted statistics and the gen_distrib columns (B = 1003) carry the same bits; the sums the same values."""
    dr = _make('tp44_mc0', B_CHUNKS, seed=61, n_perm=1, n_boot=20)
    d = _make('tp44_mc0', 1003, seed=62, n_perm=40, n_boot=40)
    want = _expect(d, True)
    got = []
    for opts in ({}, {'scratch_gb': 0.005}, {'min_batch': 8, 'scratch_gb': 0.05}):
        eng = _engine(**opts)
        _set_data(eng, dr)
        R = eng.crosscov(xsrc=dr['boots'], ysrc=dr['boots'])
        batch_r = int(eng.last_timing()['superbatch'])
        _bind(eng, d)
        sp = eng.perm(d['perms'])
        us, uq, dist = eng.boot(d['boots'])
        got.append(dict(R=R, sp=sp, us=us.cpu().numpy(), uq=uq.cpu().numpy(), dist=dist, batch_r=batch_r,
                        batch=int(eng.last_timing()['superbatch'])))
    assert got[0]['batch'] >= 40 and got[1]['batch'] < 20 and got[1]['batch_r'] < 20, [(g['batch'], g['batch_r']) for g in got]
    for g in got[1:]:
        for key in ('R', 'sp', 'dist'):
            assert np.array_equal(g[key], got[0][key]), key
    for g in got:
        _per_lv(g['us'], want['us'], 1, TOL_SUM, 'sum of U_b', live=want['live'])
        _per_lv(g['uq'], want['uq'], 1, TOL_SUM, 'sum of U_b^2', live=want['live'])


# ---- the engine after a multiblock binding -----------------------------------------------------------------------

def test_a_behavioural_binding_after_a_multiblock_one_keeps_its_bits():
    """Same cached engine, same X and Y: behavioural (every default route), multiblock, behavioural again."""
    d = _make('tp16_mc0', 1003, seed=71, n_perm=12, n_boot=12)
    eng = _engine()

    def behavioural():
        from pypyls_amd import hostmath
        eng.set_data(d['X'], d['Y'], d['cells'], len(d['groups']), d['n_cond'], 0)
        xw, sv, yw = eng.decompose()
        xw, yw = hostmath.sign_convention(xw, yw)
        eng.set_original(xw, sv, yw)
        sp = eng.perm(d['perms'])
        us, uq, dist = eng.boot(d['boots'])
        return [xw, sv, yw, sp, us.cpu().numpy(), uq.cpu().numpy(), dist, eng.crosscov(ysrc=d['perms'])]

    before = behavioural()
    _check_all(eng, d, _expect(d, True), _expect(d, False))
    after = behavioural()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# ---- limits ------------------------------------------------------------------------------------------------------

def test_limits_refuse_by_name():
    from pypyls_amd.engine import PlsxError
    import pypyls_amd as pls
    rs = np.random.RandomState(0)
    eng = _engine()
    # J = 4 cells, T = 90: T' = 364 rows = 23 data tiles + 2 moment tiles > 24: behavioral PLS would slice it
    X, Y = rs.randn(24, 40), rs.randn(24, 90)
    cells = np.repeat(np.arange(4), 6)
    with pytest.raises(PlsxError, match=r"-2.*T' = 364.*J = 4"):
        eng.set_data(X, Y, cells, 2, 2, METHOD)
    with pytest.raises(PlsxError, match=r"T' = 364.*J = 4"):
        pls.multiblock_pls(X, Y, groups=[6, 6], n_cond=2, n_perm=0, n_boot=0, verbose=False)
    d = _make('tp16_mc0', 60, seed=81, n_perm=2, n_boot=2)
    _bind(eng, d)
    masks = rs.rand(d['X'].shape[0], 3) < 0.5
    with pytest.raises(PlsxError, match='-2'):
        eng.split_half(masks)
    with pytest.raises(PlsxError, match='-2'):
        eng.crossval(masks)
    with pytest.raises(PlsxError, match='-2'):
        eng.set_contrasts(np.linalg.qr(rs.randn(16, 2))[0])
    with pytest.raises(PlsxError):
        eng.perm_ystack(np.stack([d['Y'], d['Y']]))
    # the binding is still good
    assert np.all(np.isfinite(eng.perm(d['perms'])))


# ---- the public call ---------------------------------------------------------------------------------------------

def _compare_public(res, want, n_perm):
    live = mb.ref.live_lvs(want['singvals'])
    _per_lv(res['singvals'], want['singvals'], 0, TOL_R, 'singvals', live=live)
    for key in ('x_weights', 'y_weights', 'x_scores', 'y_scores'):
        _per_lv(res[key], want[key], 1, TOL_R, key, live=live)
    _per_lv(res['varexp'], want['varexp'], 0, TOL_R, 'varexp', live=live)
    _per_lv(res['y_loadings'], want['y_loadings'], 1, TOL_DIST, 'y_loadings', live=live)
    _per_lv(res['permres']['perm_singval'], want['permres']['perm_singval'], 0, TOL_R, 'perm_singval', live=live)
    counts = np.rint(res['permres']['pvals'] * (n_perm + 1)).astype(int) - 1
    assert np.array_equal(counts[live], want['permres']['counts'][live])
    bw, bg = want['bootres'], res['bootres']
    assert sorted(bg._filled()) == sorted(bw)
    _per_lv(bg['y_loadings_boot'], bw['y_loadings_boot'], 1, TOL_DIST, 'y_loadings_boot', live=live)
    _per_lv(bg['y_loadings_ci'], bw['y_loadings_ci'], 1, TOL_DIST, 'y_loadings_ci', live=live)
    _per_lv(bg['y_loadings'], bw['y_loadings'], 1, TOL_DIST, 'bootres.y_loadings', live=live)
    _per_lv(bg['x_weights_stderr'], bw['x_weights_stderr'], 1, TOL_SUM, 'x_weights_stderr', live=live)
    _per_lv(bg['x_weights_normed'], bw['x_weights_normed'], 1, TOL_SUM, 'x_weights_normed', live=live)


@pytest.mark.parametrize('rotate', [True, False])
def test_public_call_against_the_expectation(rotate):
    import pypyls_amd as pls
    d = _make('tp16_mc0', 129, seed=91, n_perm=1, n_boot=1)
    kw = dict(groups=d['groups'], n_cond=d['n_cond'], mean_centering=d['mc'], n_perm=64, n_boot=64, rotate=rotate,
              seed=1234, verbose=False)
    res = pls.multiblock_pls(d['X'], d['Y'], **kw)
    assert res.inputs['method'] == 'multiblock'
    assert not res['cvres']._filled() and not res['splitres']._filled()
    perms, boots = res['permres']['permsamples'], res['bootres']['bootsamples']
    assert perms.shape == (d['X'].shape[0], 64) and boots.shape == (d['X'].shape[0], 64)
    want = mb.run_multiblock(d['X'], d['Y'], groups=d['groups'], n_cond=d['n_cond'], mean_centering=d['mc'],
                             rotate=rotate, permsamples=perms, bootsamples=boots)
    assert mb.closest_tie(want['singvals'], want['permres']['perm_singval']) > 1e-6
    _compare_public(res, want, 64)
    if not rotate:
        return
    # a team of two contexts on one device: what belongs to one resample carries the same bits, the sums the same values
    two = pls.multiblock_pls(d['X'], d['Y'], device_ids=[0, 0], **kw)
    for key in ('singvals', 'x_weights', 'y_weights'):
        assert np.array_equal(two[key], res[key]), key
    assert np.array_equal(two['permres']['perm_singval'], res['permres']['perm_singval'])
    assert np.array_equal(two['permres']['pvals'], res['permres']['pvals'])
    assert np.array_equal(two['bootres']['y_loadings_boot'], res['bootres']['y_loadings_boot'])
    _compare_public(two, want, 64)
    # ... and the results go through save_results / load_results
    import tempfile
    import os
    from pypyls_amd import io
    try:
        io._h5py()
    except ImportError:
        return
    with tempfile.TemporaryDirectory() as tmp:
        back = pls.load_results(pls.save_results(os.path.join(tmp, 'mb'), res))
    assert back.inputs.method == 'multiblock'
    assert np.array_equal(back.bootres.x_weights_normed, res.bootres.x_weights_normed, equal_nan=True)   # (null LVs: 0 / 0)
    assert np.array_equal(back.permres.pvals, res.permres.pvals)
