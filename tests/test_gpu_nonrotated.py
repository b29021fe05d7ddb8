"""Non-rotated PLS on the device (plsx_set_contrasts; k_contrast_norms, k_contrast_quad, k_contrast_fill) against the
numpy definition of tests/nonrotated_expect.py.

Tolerances (the project's): values derived from R (singular values, weights, permuted statistics) 1e-10 of their own
LV's scale, the gen_distrib columns 1e-9, the bootstrap sums and what is computed from them 1e-8 per live LV.
P-values are compared as exact integer counts; every fixture first asserts ON THE EXPECTATION that no permuted value
lies within 1e-6 (relative) of the observed one, so that a count cannot turn on rounding."""
import warnings

import numpy as np
import pytest

from conftest import load_golden
import nonrotated_expect as nr

pytestmark = pytest.mark.gpu

TOL_R, TOL_DIST, TOL_SUM = 1e-10, 1e-9, 1e-8
_ENGINES = {}


def _engine(**options):
    """One engine per option set, kept for the module (a context maps its scratch once)."""
    from pypyls_amd.engine import Engine
    key = tuple(sorted(options.items()))
    if key not in _ENGINES:
        scratch = options.pop('scratch_gb', None)
        _ENGINES[key] = Engine(scratch_gb=scratch, options=options)
    return _ENGINES[key]


def _make(method, groups, n_cond, T, B, seed, covariance=False, mean_centering=0, n_perm=6, n_boot=6):
    """Random data of the design, permutations of the rows, bootstraps within the cells."""
    rs = np.random.RandomState(seed)
    spec = nr.spec_of(method, groups, n_cond, covariance, mean_centering)
    S = spec.dummy.shape[0]
    cells = spec.dummy.argmax(axis=1)
    X = rs.randn(S, B) + 0.3 * cells[:, None] * rs.randn(1, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :1] if method == 'behavioral' else spec.dummy
    perms = np.stack([rs.permutation(S) for _ in range(n_perm)], axis=1)
    boots = np.zeros((S, n_boot), dtype=np.int64)
    for b in range(n_boot):
        for c in range(spec.dummy.shape[1]):
            rows = np.flatnonzero(cells == c)
            while True:
                draw = rs.choice(rows, size=rows.size)
                if np.unique(draw).size >= min(rows.size - 1, 3):     # (never a constant cell, never only permutations)
                    break
            boots[rows, b] = draw
    return dict(spec=spec, method=method, X=X, Y=Y, cells=cells, perms=perms, boots=boots,
                Tp=spec.dummy.shape[1] * (T if method == 'behavioral' else 1))


def _contrasts(Tp, Lc, seed, orthonormal=True):
    C = np.random.RandomState(1000 + seed).randn(Tp, Lc)
    return np.linalg.qr(C)[0] if orthonormal else C


def _expect(d, C):
    spec, X, Y = d['spec'], d['X'], d['Y']
    U, sv, V = nr.original(spec, X, Y, C)
    sp = nr.perm_singvals(spec, X, Y, V, d['perms'])
    assert nr.closest_tie(sv, sp) > 1e-6, 'fixture: a permuted value ties with the observed one'
    us, uq, dist = nr.boot_sums(spec, X, Y, V, U, d['boots'])
    return dict(U=U, sv=sv, V=V, sp=sp, us=us, uq=uq, dist=dist, counts=np.sum(sp > sv[:, None], axis=1))


def _bind(eng, d, C):
    """set_data, set_contrasts, decompose, set_original -> (x_weights, singvals, y_weights), all L columns."""
    spec = d['spec']
    eng.set_data(d['X'], d['Y'] if d['method'] == 'behavioral' else None, d['cells'], len(spec.groups), spec.n_cond,
                 0 if d['method'] == 'behavioral' else 1, mean_centering=spec.mean_centering,
                 covariance=spec.covariance)
    eng.set_contrasts(nr.ref.normalize(np.asarray(C, dtype=float)))
    xw, sv, yw = eng.decompose()
    eng.set_original(xw, sv, yw)
    return xw, sv, yw


def _per_lv(got, want, axis, tol, what, live=None):
    got, want = np.moveaxis(np.asarray(got), axis, 0), np.moveaxis(np.asarray(want), axis, 0)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), what + ': non-finite'
    for k in range(want.shape[0]):
        if live is not None and not live[k]:
            continue
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max()
        assert err <= tol * scale, '{}: LV {}: err {:.3e}, scale {:.3e}, tol {:g}'.format(what, k, err, scale, tol)


def _check_all(eng, d, C, want, perms=True, boots=True):
    Lc = np.asarray(C).shape[1]
    xw, sv, yw = _bind(eng, d, C)
    assert xw.shape[1] == eng.L and np.all(xw[:, Lc:] == 0) and np.all(sv[Lc:] == 0) and np.all(yw[:, Lc:] == 0)
    _per_lv(sv[:Lc], want['sv'], 0, TOL_R, 'singvals')
    _per_lv(xw[:, :Lc], want['U'], 1, TOL_R, 'x_weights')
    assert np.abs(yw[:, :Lc] - want['V']).max() <= 1e-15
    out = dict(xw=xw, sv=sv)
    if perms:
        sp = eng.perm(d['perms'], rotate=True)
        assert np.all(sp[Lc:] == 0)
        _per_lv(sp[:Lc], want['sp'], 0, TOL_R, 'perm_singval')
        assert np.array_equal(np.sum(sp[:Lc] > sv[:Lc, None], axis=1), want['counts'])
        assert np.array_equal(eng.perm(d['perms'], rotate=False), sp), '`rotate` must be ignored'
        out['sp'] = sp
    if boots:
        us, uq, dist = eng.boot(d['boots'])
        us, uq = us.cpu().numpy(), uq.cpu().numpy()
        assert np.all(us[:, Lc:] == 0) and np.all(uq[:, Lc:] == 0)
        _per_lv(dist[:, :Lc], want['dist'], 1, TOL_DIST, 'distrib')
        _per_lv(us[:, :Lc], want['us'], 1, TOL_SUM, 'sum of U_b')
        _per_lv(uq[:, :Lc], want['uq'], 1, TOL_SUM, 'sum of U_b^2')
        n = d['boots'].shape[1]
        if n > 1:
            bs = want['U'] * want['sv']
            _, se_w = nr.ref.boot_rel(bs, want['us'], want['uq'], n)
            _, se_g = nr.ref.boot_rel(bs, us[:, :Lc], uq[:, :Lc], n)
            _per_lv(se_g, se_w, 1, TOL_SUM, 'standard error')
        out.update(us=us, uq=uq, dist=dist)
    return out


# (method, groups, n_cond, T, covariance, mean_centering, B, Lc): T' in {1, 4, 5, 16, 17, 64, 65, 72, 360},
# B in {1, 15, 16, 17, 129, 200, 1003} (partial last tile, partial last chunk of 32 tiles, two chunks), Lc in {1, 16, 17, T'}
ABI_CASES = {
    'mc0_tp4_b15_l1': ('meancentered', [7, 6], 2, 0, False, 0, 15, 1),
    'corr_tp1_b17_l1': ('behavioral', [12], 1, 1, False, 0, 17, 1),
    'cov_tp5_b16_lTp': ('behavioral', [14], 1, 5, True, 0, 16, 5),
    'corr_tp16_b129_l16': ('behavioral', [10, 9], 2, 4, False, 0, 129, 16),
    'mc1_tp17_b1003_l17': ('meancentered', [3] * 17, 1, 0, False, 1, 1003, 17),
    'corr_tp64_b129_l17': ('behavioral', [12, 12], 2, 16, False, 0, 129, 17),
    'cov_tp65_b200_lTp': ('behavioral', [8] * 5, 1, 13, True, 0, 200, 65),
    'mc2_tp72_b129_l16': ('meancentered', [4] * 36, 2, 0, False, 2, 129, 16),
    'corr_tp360_b200_l17': ('behavioral', [8, 8], 2, 90, False, 0, 200, 17),
    'corr_tp4_b1_l1': ('behavioral', [9, 8], 1, 2, False, 0, 1, 1),
    'cov_tp16_b1003_l1': ('behavioral', [10, 9], 2, 4, True, 0, 1003, 1),
}


@pytest.mark.parametrize('case', sorted(ABI_CASES))
def test_c_abi_against_the_expectation(case):
    method, groups, n_cond, T, cov, mc, B, Lc = ABI_CASES[case]
    d = _make(method, groups, n_cond, T, B, seed=len(case), covariance=cov, mean_centering=mc)
    C = _contrasts(d['Tp'], Lc, seed=B)
    _check_all(_engine(), d, C, _expect(d, C))


@pytest.mark.parametrize('case', ['corr_tp16_b129_l16', 'mc0_tp4_b15_l1'])
def test_batch_sizes_around_a_launch_group(case):
    """n = 1, one short of the resamples one cross-product group holds, one over it: prefixes of ONE expectation."""
    method, groups, n_cond, T, cov, mc, B, Lc = ABI_CASES[case]
    eng = _engine(no_dual_perm=1)
    probe = _make(method, groups, n_cond, T, B, seed=3, covariance=cov, mean_centering=mc, n_perm=1, n_boot=1)
    C = _contrasts(probe['Tp'], Lc, seed=B)
    _bind(eng, probe, C)
    eng.boot(probe['boots'])
    per_group = int(eng.last_timing()['resamples_per_group'])
    assert per_group >= 1
    n_max = per_group + 1
    d = _make(method, groups, n_cond, T, B, seed=3, covariance=cov, mean_centering=mc, n_perm=n_max, n_boot=n_max)
    spec, X, Y = d['spec'], d['X'], d['Y']
    U, sv, V = nr.original(spec, X, Y, C)
    sp = nr.perm_singvals(spec, X, Y, V, d['perms'])
    _bind(eng, d, C)
    for n in sorted({1, max(per_group - 1, 1), per_group + 1}):
        got = eng.perm(d['perms'][:, :n])
        _per_lv(got[:Lc], sp[:, :n], 0, TOL_R, 'perm_singval, n = {}'.format(n))
        us_w, uq_w, dist_w = nr.boot_sums(spec, X, Y, V, U, d['boots'][:, :n])
        us, uq, dist = eng.boot(d['boots'][:, :n])
        _per_lv(dist[:, :Lc], dist_w, 1, TOL_DIST, 'distrib, n = {}'.format(n))
        _per_lv(us.cpu().numpy()[:, :Lc], us_w, 1, TOL_SUM, 'sum of U_b, n = {}'.format(n))
        _per_lv(uq.cpu().numpy()[:, :Lc], uq_w, 1, TOL_SUM, 'sum of U_b^2, n = {}'.format(n))


def test_every_permutation_route():
    """Dual (v^T G_p v), fixed-X feature pass, gathered feature pass (no_fixed_x): each against the expectation and
    against each other at 1e-9; the route is read back from the engine, and no Gram pass / small solve ran."""
    d = _make('behavioral', [11, 10], 2, 3, 300, seed=5, n_perm=40, n_boot=1)
    C = _contrasts(d['Tp'], 3, seed=7)
    want = _expect(d, C)
    got = {}
    for name, opts in (('dual', {}), ('fixed_x', {'no_dual_perm': 1}), ('gathered', {'no_dual_perm': 1, 'no_fixed_x': 1})):
        eng = _engine(**opts)
        eng.set_timing(True)
        got[name] = _check_all(eng, d, C, want, boots=False)['sp'][:3]
        kt, lt = eng.kernel_timing(), eng.last_timing()
        eng.set_timing(False)
        assert bool(lt['dual_perm']) == (name == 'dual'), (name, lt)
        assert 'k_contrast' in kt and 'k_small' not in kt, (name, kt)
        if name != 'dual':
            assert 'k_gram' not in kt, (name, kt)
    for a in got:
        for b in got:
            _per_lv(got[a], got[b], 0, 1e-9, 'perm_singval {} vs {}'.format(a, b))


@pytest.mark.parametrize('mode', ['corr', 'cov', 'mc'])
def test_every_bootstrap_route(mode):
    """Scaled mode: compact and dense blocks (two-pass with k_urot).  Unscaled modes: single-pass, two_pass_boot, the
    quadratic-form series forced on and off.  Each against the expectation and each other at 1e-9."""
    if mode == 'mc':
        d = _make('meancentered', [9, 8, 8], 2, 0, 260, seed=8, mean_centering=0, n_perm=1, n_boot=40)
    else:
        d = _make('behavioral', [11, 10], 2, 3, 260, seed=9, covariance=(mode == 'cov'), n_perm=1, n_boot=40)
    C = _contrasts(d['Tp'], 3, seed=11)
    want = _expect(d, C)
    eng = _engine()
    routes = [('compact', {'compact_boot_always': 1}), ('dense', {'no_compact_boot': 1})] if mode == 'corr' else \
        [('single_pass', {'quad_sums': -1}), ('two_pass', {'two_pass_boot': 1}), ('quad', {'quad_sums': 1})]
    got = {}
    for name, opts in routes:
        for key, val in opts.items():
            eng.set_option(key, val)
        try:
            _bind(eng, d, C)
            assert eng.boot_begin(40) == (1 if name == 'quad' else 0), name
            eng.set_timing(True)
            got[name] = _check_all(eng, d, C, want, perms=False)
            kt, lt = eng.kernel_timing(), eng.last_timing()
            eng.set_timing(False)
        finally:
            for key in opts:
                eng.set_option(key, 0)
        assert 'k_contrast' in kt and 'k_small' not in kt, (name, kt)
        if name in ('compact', 'dense', 'two_pass'):
            assert 'k_gram' not in kt and 'k_urot' in kt, (name, kt)
        if mode == 'corr':
            assert (lt['compact_row_fraction'] > 0) == (name == 'compact'), (name, lt)
    names = sorted(got)
    for a in names:
        for b in names:
            for key in ('us', 'uq', 'dist'):
                _per_lv(got[a][key][:, :3], got[b][key][:, :3], 1, 1e-9, '{} {} vs {}'.format(key, a, b))


def test_same_bits_whatever_the_scratch_budget():
    """The chunking of k_contrast_norms follows B alone: three budgets (three batch sizes), the same bits."""
    d = _make('behavioral', [11, 10], 2, 3, 1003, seed=12, n_perm=70, n_boot=1)
    C = _contrasts(d['Tp'], 3, seed=13)
    got = []
    for gb in (0.002, 0.02, 1.0):
        eng = _engine(no_dual_perm=1, scratch_gb=gb)
        _bind(eng, d, C)
        got.append((eng.perm(d['perms']), int(eng.last_timing()['superbatch'])))
    assert len({g[1] for g in got}) > 1, 'the budgets did not change the batch size: ' + str([g[1] for g in got])
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][0], got[2][0])


def test_contrast_orthogonal_to_the_data():
    """All-ones over the cells with mean_centering=2 (the grand mean is removed): a singular value <= 1e-12 of the
    largest, a finite zero-or-unit weight column, no NaN anywhere."""
    d = _make('meancentered', [6, 6], 2, 0, 129, seed=14, mean_centering=2)
    C = np.stack([np.ones(4), np.array([1.0, -1.0, 1.0, -1.0])], axis=1)
    # (cells of equal size: the grand mean is the mean of the cell means, so the rows of R sum to zero)
    R = nr.ref.gen_covcorr(d['spec'], d['X'], d['Y'], d['spec'].dummy)
    assert np.abs(R.sum(axis=0)).max() <= 1e-13 * np.abs(R).max(), 'fixture: the cell means do not sum to zero'
    eng = _engine()
    xw, sv, yw = _bind(eng, d, C)
    assert sv[0] <= 1e-12 * sv[1]
    norm0 = np.sqrt((xw[:, 0] ** 2).sum())
    assert np.all(np.isfinite(xw)) and (norm0 == 0 or abs(norm0 - 1) <= 1e-12)
    sp = eng.perm(d['perms'])
    us, uq, dist = eng.boot(d['boots'])
    for a in (sp, us.cpu().numpy(), uq.cpu().numpy(), dist):
        assert np.all(np.isfinite(a))
    V = nr.ref.normalize(C)
    want_sp = nr.perm_singvals(d['spec'], d['X'], d['Y'], V, d['perms'])
    _per_lv(sp[1:2], want_sp[1:2], 0, TOL_R, 'perm_singval of the live contrast')


def test_small_contrast_leaves_the_dual_route():
    """A contrast whose singular value lies below 1e-3 of the largest: the binding takes the feature pass (as a graded
    spectrum does) and every LV still meets 1e-10 of its own scale."""
    d = _make('behavioral', [11, 10], 2, 3, 300, seed=15, covariance=True, n_perm=12, n_boot=12)
    spec = d['spec']
    R = nr.ref.gen_covcorr(spec, d['X'], d['Y'], spec.dummy)
    u, s, _ = np.linalg.svd(R, full_matrices=False)
    C = np.stack([u[:, 0], u[:, -1]], axis=1)
    # covariance mode is linear in X: X <- X - (1 - eps) (X z) z^T with z = normalize(R^T c_2) scales what the second
    # contrast sees by eps and leaves the first alone (R^T c_1 is orthogonal to z for singular vectors)
    z = R.T @ C[:, 1]
    z /= np.sqrt(z @ z)
    eps = 5e-4 * s[0] / s[-1]
    d['X'] = d['X'] - (1 - eps) * np.outer(d['X'] @ z, z)
    want = _expect(d, C)
    ratio = want['sv'][1] / want['sv'][0]
    assert 1e-4 < ratio < 1e-3, 'fixture: the second contrast is not below the threshold: {}'.format(ratio)
    eng = _engine()
    _bind(eng, d, C)
    eng.perm(d['perms'])
    assert not bool(eng.last_timing()['dual_perm'])
    _check_all(eng, d, C, want)
    # ... while the same design with both contrasts of ordinary size stays on the dual route
    d2 = _make('behavioral', [11, 10], 2, 3, 300, seed=15, covariance=True, n_perm=2, n_boot=1)
    _bind(eng, d2, C)
    eng.perm(d2['perms'])
    assert bool(eng.last_timing()['dual_perm'])


# ---- public calls -----------------------------------------------------------------------------------------------

def _public(g, method, **kw):
    import pypyls_amd as pls
    base = dict(groups=list(g['groups']), n_cond=int(g['n_cond']), verbose=False)
    base.update(kw)
    if method == 'behavioral':
        return pls.behavioral_pls(g['X'], g['Y'], covariance=bool(g.get('covariance', False)), **base)
    return pls.meancentered_pls(g['X'], mean_centering=int(g.get('mean_centering', 0)), **base)


def _compare_public(res, want, method, Lc):
    _per_lv(res['singvals'], want['singvals'], 0, TOL_R, 'singvals')
    for key in ('x_weights', 'x_scores', 'y_scores'):
        _per_lv(res[key], want[key], 1, TOL_R, key)
    assert np.abs(res['y_weights'] - want['y_weights']).max() <= 1e-15
    _per_lv(res['varexp'], want['varexp'], 0, TOL_R, 'varexp')
    _per_lv(res['permres']['perm_singval'], want['permres']['perm_singval'], 0, TOL_R, 'perm_singval')
    n_perm = want['permres']['perm_singval'].shape[1]
    assert np.array_equal(np.rint(res['permres']['pvals'] * (n_perm + 1)).astype(int) - 1, want['permres']['counts'])
    bw, bg = want['bootres'], res['bootres']
    boot_key = 'y_loadings_boot' if method == 'behavioral' else 'contrast_boot'
    ci_key = 'y_loadings_ci' if method == 'behavioral' else 'contrast_ci'
    assert bg[boot_key].shape == bw[boot_key].shape and bg[boot_key].shape[1] == Lc
    _per_lv(bg[boot_key], bw[boot_key], 1, TOL_DIST, boot_key)
    _per_lv(bg[ci_key], bw[ci_key], 1, TOL_DIST, ci_key)
    _per_lv(bg['x_weights_stderr'], bw['x_weights_stderr'], 1, TOL_SUM, 'x_weights_stderr')
    _per_lv(bg['x_weights_normed'], bw['x_weights_normed'], 1, TOL_SUM, 'x_weights_normed')
    if method == 'behavioral':
        _per_lv(res['y_loadings'], want['y_loadings'], 1, TOL_DIST, 'y_loadings')
    else:
        _per_lv(bg['contrast'], bw['contrast'], 1, TOL_DIST, 'contrast')


@pytest.mark.parametrize('name,method', [('bpls_2g2c', 'behavioral'), ('bpls_2g2c_cov', 'behavioral'),
                                         ('mpls_3g2c_mc0', 'meancentered'), ('mpls_3g2c_mc2', 'meancentered')])
def test_public_call_against_the_expectation(name, method):
    g = load_golden(name)
    Tp = g['ref_y_weights'].shape[0]
    C = _contrasts(Tp, 3, seed=Tp) * np.array([1.0, 5.0, 0.2])           # (the scale is normalised away)
    perms, boots = g['ref_permres__permsamples'], g['ref_bootres__bootsamples']
    want = nr.run_nonrotated(g['X'], g.get('Y'), contrasts=C, method=method, groups=list(g['groups']),
                             n_cond=int(g['n_cond']), covariance=bool(g.get('covariance', False)),
                             mean_centering=int(g.get('mean_centering', 0)), permsamples=perms, bootsamples=boots)
    assert nr.closest_tie(want['singvals'], want['permres']['perm_singval']) > 1e-6
    res = _public(g, method, contrasts=C, permsamples=perms, bootsamples=boots, n_perm=perms.shape[1],
                  n_boot=boots.shape[1], n_split=0)
    _compare_public(res, want, method, 3)
    assert np.array_equal(res.inputs['contrasts'], C)
    assert not res['cvres']._filled() and not res['splitres']._filled()
    # the team of two contexts on one device: the permuted statistics carry the same bits, the rest the same values
    two = _public(g, method, contrasts=C, permsamples=perms, bootsamples=boots, n_perm=perms.shape[1],
                  n_boot=boots.shape[1], n_split=0, device_ids=[0, 0])
    assert np.array_equal(two['permres']['perm_singval'], res['permres']['perm_singval'])
    assert np.array_equal(two['singvals'], res['singvals'])
    _compare_public(two, want, method, 3)


def test_public_pre_permuted_y_stacks():
    g = load_golden('bpls_2g2c')
    C = _contrasts(16, 2, seed=21)
    perms = g['ref_permres__permsamples'][:, :10]
    ystack = np.stack([g['Y'][perms[:, i]] for i in range(perms.shape[1])])
    want = nr.run_nonrotated(g['X'], g['Y'], contrasts=C, groups=list(g['groups']), n_cond=int(g['n_cond']),
                             ystack=ystack)
    assert nr.closest_tie(want['singvals'], want['permres']['perm_singval']) > 1e-6
    res = _public(g, 'behavioral', contrasts=C, permsamples=ystack, permindices=False, n_perm=10, n_boot=0)
    _per_lv(res['permres']['perm_singval'], want['permres']['perm_singval'], 0, TOL_R, 'perm_singval')
    assert np.array_equal(np.rint(res['permres']['pvals'] * 11).astype(int) - 1, want['permres']['counts'])


def test_seeded_draws_do_not_move_and_the_plain_call_keeps_its_bits():
    import pypyls_amd as pls
    g = load_golden('bpls_2g2c')
    C = _contrasts(16, 2, seed=22)
    kw = dict(seed=1234, n_perm=20, n_boot=20)
    before = _public(g, 'behavioral', **kw)                                  # (cross-validation on: its masks come last)
    none = _public(g, 'behavioral', contrasts=None, **kw)
    with_c = _public(g, 'behavioral', contrasts=C, **kw)
    after = _public(g, 'behavioral', **kw)                                   # the shared engine, right after a contrast call
    assert np.array_equal(with_c['permres']['permsamples'], before['permres']['permsamples'])
    assert np.array_equal(with_c['bootres']['bootsamples'], before['bootres']['bootsamples'])
    assert 'contrasts' not in none.inputs and 'contrasts' not in before.inputs
    assert not with_c['cvres']._filled() and before['cvres']._filled()
    for other in (none, after):
        for key in ('x_weights', 'singvals', 'y_weights', 'x_scores'):
            assert np.array_equal(other[key], before[key]), key
        assert np.array_equal(other['permres']['perm_singval'], before['permres']['perm_singval'])
        assert np.array_equal(other['bootres']['x_weights_normed'], before['bootres']['x_weights_normed'])
        assert np.array_equal(other['cvres']['pearson_r'], before['cvres']['pearson_r'])
    with pytest.raises(ValueError, match='n_split'):
        _public(g, 'behavioral', contrasts=C, n_split=4, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                        # orthonormal contrasts: no warning
        pls.meancentered_pls(load_golden('mpls_3g2c_mc0')['X'], groups=[9, 9, 9], n_cond=2, n_perm=0, n_boot=0,
                             contrasts=_contrasts(6, 2, seed=23), verbose=False)


def test_entries_that_are_not_built_refuse():
    from pypyls_amd.engine import PlsxError
    d = _make('behavioral', [11, 10], 2, 3, 60, seed=16, n_perm=2, n_boot=2)
    eng = _engine()
    _bind(eng, d, _contrasts(d['Tp'], 2, seed=17))
    masks = np.random.RandomState(0).rand(d['X'].shape[0], 3) < 0.5
    with pytest.raises(PlsxError, match='-2'):
        eng.split_half(masks)
    with pytest.raises(PlsxError, match='-2'):
        eng.crossval(masks)
    eng.set_contrasts(None)                                                    # back to SVD mode: the entries work again
    xw, sv, yw = eng.decompose()
    eng.set_original(xw, sv, yw)
    eng.crossval(masks)
