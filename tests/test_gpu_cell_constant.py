"""Cell-constant features on every scaling site of the device ("Cell-constant features").

A feature whose rows in a (resample, cell) hold bit-identical values gets scale 0: the T rows of R that belong to the
cell are exactly 0.0 in its column, nothing is NaN or inf, and everything else is what it would be without the feature.
The expectation is oracle.cpu_ref under tests/cell_constant_expect.contract(); the data are its armed sets, on which the
kernels' former `var > 0` rules return a scale for a third of the constant cells and more
(tests/test_cell_constant_host.py).  Every case says which kernel route it pins, from Engine.last_timing /
kernel_timing / split_route, and prints its figures before it asserts.

Sites (pypyls_amd/csrc) and the case that reaches them:
  k_cell_scale (plsx_k_prep.h)                  test_fixed_x_routes: dual (K = Xn Xn^T), projected, fixed (R read back)
  k_xprod in-block moments (plsx_k_xprod.h)     test_bootstrap_routes[inblock], test_crossval (with the moment export)
  k_xprod EPI 4, moment-only blocks             test_bootstrap_routes[sepmom, compact2_table, compact4_table]
  k_xprod_compact moment rows, 2 / 4 col tiles  test_bootstrap_routes[compact2, compact4]
  k_xprod split epilogue (dense fused)          test_split_half_routes[dense]
  k_xprod_compact EPI 5                         test_split_half_routes[compact5, two_readers]
  k_split_colconst, k_cell_sd (one-pass reader) test_split_half_routes[one_pass, reader8]
  two-pass split route (masked resamples)       test_split_half_routes[two_pass]
Tolerances are those of tests/test_gpu_kernels.py for the same quantities: R 1e-10, permuted singular values 1e-8,
bootstrap sums and distrib 1e-7, split-half correlations 1e-7.
"""
import functools

import numpy as np
import pytest

from conftest import assert_close
from oracle import cpu_ref as ref
import cell_constant_expect as cc

pytestmark = pytest.mark.gpu

SHAPES = [('2g', 70), ('2g', 130), ('3c', 70), ('3c', 130), ('1g', 70), ('1g', 130)]
N_PERM = 5


def _engine(a, X=None, Y=None, **options):
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    eng = Engine(options=options)
    eng.set_data(a.X if X is None else X, a.Y if Y is None else Y, rsmp.cell_of_row(a.groups, a.n_cond),
                 len(a.groups), a.n_cond, 0)
    eng.set_timing(True)
    return eng


@functools.lru_cache(maxsize=None)
def _case(design, B, T=3):
    """Armed data of one shape, its resampling arrays and the contract's expectations -- computed once, read-only."""
    from pypyls_amd import resampling as rsmp
    a = cc.armed(design, B, T, seed=cc.SEEDS[(sorted(cc.DESIGNS).index(design) + (B > 100) + (T > 3)) % len(cc.SEEDS)])
    spec, X, Y = a.spec, a.X, a.Y
    J = len(a.cells)
    a.perms = rsmp.gen_permsamp(a.groups, a.n_cond, N_PERM, seed=1)
    # ordinary draws, then explicit ones that miss / hit the non-zero row of the sparse column cell by cell
    a.boots = np.hstack([rsmp.gen_bootsamp(a.groups, a.n_cond, 3, seed=2), cc.sparse_bootstraps(a, 2 ** J, seed=3)])
    nb = a.boots.shape[1]
    with cc.contract():
        a.R0 = ref.gen_covcorr(spec, X, Y, spec.dummy)
        a.Rp = [ref.gen_covcorr(spec, X, Y[a.perms[:, i]], spec.dummy) for i in range(N_PERM)]
        a.Rb = [ref.gen_covcorr(spec, X[a.boots[:, i]], Y[a.boots[:, i]], spec.dummy) for i in range(nb)]
        a.U, a.d, a.V = ref.decompose(spec, X, Y)
        a.perm = {}
        for rotate in (True, False):
            spec.rotate = rotate
            a.perm[rotate] = np.stack([ref.single_perm(spec, X, Y, a.perms[:, i], a.V)[0] for i in range(N_PERM)], -1)
        spec.rotate = True
        sb = [ref.single_boot(spec, X, Y, a.boots[:, i], a.U, a.d) for i in range(nb)]
    a.usum, a.usq = sum(s[1] for s in sb), sum(s[1] ** 2 for s in sb)
    a.dist = np.stack([s[0] for s in sb], -1)
    a.const0 = cc.constant_cells(spec, X)
    a.constb = [cc.constant_cells(spec, X[a.boots[:, i]]) for i in range(nb)]
    assert any(c[:, a.sparse].any() for c in a.constb) and not all(c[:, a.sparse].all() for c in a.constb)
    for v in (a.X, a.Y, a.R0, a.usum, a.usq, a.dist, a.U, a.d, a.V):
        v.setflags(write=False)
    return a


def _check_R(got, want, const, T, what):
    """Constant entries exactly 0.0, nothing non-finite, the rest against the contract at 1e-10."""
    mask = np.repeat(const, T, axis=0)
    assert not want[mask].any()
    finite = bool(np.all(np.isfinite(got)))
    nz = int(np.count_nonzero(got[mask])) if finite else -1
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want))) if finite else np.inf
    print('{}: {} constant entries, {} non-zero (largest {:.3e}), rel err {:.3e}'.format(
        what, int(mask.sum()), nz, float(np.max(np.abs(got[mask]))) if finite else np.nan, err))
    assert finite, what + ': non-finite entries'
    assert nz == 0, what + ': {} constant entries are not 0.0'.format(nz)
    assert_close(got, want, 1e-10, what=what)


# ---------------------------------------------------------------------------------------------------------------------
# R itself and the bootstrap chain on every layout of the moment arithmetic
# ---------------------------------------------------------------------------------------------------------------------

BOOT_ROUTES = {
    'inblock': dict(inblock_moments=1, no_compact_boot=1),
    'sepmom': dict(sepmom_always=1, no_compact_boot=1),
    'compact2': dict(compact_boot_always=1, crosscov_sparse=1, no_compact_wide=1),
    'compact4': dict(compact_boot_always=1, crosscov_sparse=1, compact_wide_always=1),
    'compact2_table': dict(compact_boot_always=1, crosscov_sparse=1, no_compact_wide=1, no_moment_rows=1),
    'compact4_table': dict(compact_boot_always=1, crosscov_sparse=1, compact_wide_always=1, no_moment_rows=1),
}


def _pin_boot_route(route, eng, what):
    tm, kt = eng.last_timing(), eng.kernel_timing()
    print(what, 'route', {k: tm[k] for k in ('compact_row_fraction', 'moment_rows', 'compact_col_tiles')}, sorted(kt))
    assert 'k_xprod' in kt, what
    if route == 'inblock':
        assert tm['compact_row_fraction'] == 0.0 and 'k_xprod_moments' not in kt, what
    elif route == 'sepmom':
        assert tm['compact_row_fraction'] == 0.0 and 'k_xprod_moments' in kt, what
    else:
        assert tm['compact_row_fraction'] > 0.0 and 'k_xprod_moments' in kt, what
        assert tm['compact_col_tiles'] == (4 if route.startswith('compact4') else 2), what
        assert tm['moment_rows'] == (0 if route.endswith('_table') else 1), what


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '{}-B{}'.format(*s))
@pytest.mark.parametrize('route', sorted(BOOT_ROUTES))
def test_bootstrap_routes(route, shape):
    # (the separate-moments layout keeps the scale tile of a block's resamples in 48 KB of LDS: no such layout below
    # four behaviours per cell)
    a = _case(*shape, T=4 if route == 'sepmom' else 3)
    T, nb = a.Y.shape[1], a.boots.shape[1]
    what = 'R {} {}'.format(route, shape)
    got = {}
    for key, X in (('all', a.X), ('kept', a.X[:, a.keep])):
        eng = _engine(a, X=X, **BOOT_ROUTES[route])
        try:
            if key == 'all':
                _check_R(eng.crosscov(n=1)[0], a.R0, a.const0, T, what + ' original')
                Rp = eng.crosscov(ysrc=a.perms)
                for i in range(N_PERM):
                    _check_R(Rp[i], a.Rp[i], a.const0, T, what + ' permutation %d' % i)
                eng.set_timing(True)
                Rb = eng.crosscov(xsrc=a.boots, ysrc=a.boots)
                _pin_boot_route(route, eng, what + ' crosscov')
                for i in range(nb):
                    _check_R(Rb[i], a.Rb[i], a.constb[i], T, what + ' bootstrap %d' % i)
            eng.set_original(a.U if key == 'all' else a.U[a.keep], np.diag(a.d), a.V)
            eng.set_timing(True)
            usum, usq, dist = eng.boot(a.boots)
            _pin_boot_route(route, eng, what + ' boot')
            got[key] = (usum.cpu().numpy(), usq.cpu().numpy(), dist)
        finally:
            eng.close()
    usum, usq, dist = got['all']
    assert all(np.all(np.isfinite(g)) for g in got['all'])
    assert not usum[a.dead].any() and not usq[a.dead].any(), 'sums of a feature that is constant in every cell'
    assert_close(usum, a.usum, 1e-7, what='u_sum vs contract')
    assert_close(usq, a.usq, 1e-7, what='u_square vs contract')
    assert_close(dist, a.dist, 1e-7, what='distrib vs contract')
    for g, k, name in zip((usum[a.keep], usq[a.keep], dist), got['kept'], ('u_sum', 'u_square', 'distrib')):
        assert_close(g, k, 1e-7, what=name + ' vs the data without the constant columns')


# ---------------------------------------------------------------------------------------------------------------------
# the fixed-X routes: Xn = Xc * scale (k_cell_scale)
# ---------------------------------------------------------------------------------------------------------------------

PERM_ROUTES = {
    'dual': dict(),
    'projected': dict(no_dual_perm=1),
    'fixed': dict(no_dual_perm=1, no_perm_project=1),
    'general': dict(no_fixed_x=1, no_dual_perm=1),
}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '{}-B{}'.format(*s))
@pytest.mark.parametrize('route', sorted(PERM_ROUTES))
def test_fixed_x_routes(route, shape):
    a = _case(*shape)
    T = a.Y.shape[1]
    what = 'perm {} {}'.format(route, shape)
    got = {}
    for key, X in (('all', a.X), ('kept', a.X[:, a.keep])):
        eng = _engine(a, X=X, **PERM_ROUTES[route])
        try:
            eng.set_original(a.U if key == 'all' else a.U[a.keep], np.diag(a.d), a.V)
            for rotate in (True, False):
                got[key, rotate] = eng.perm(a.perms, rotate=rotate)
                tm = eng.last_timing()
                assert bool(tm['dual_perm']) == (route == 'dual'), (what, tm)
                assert bool(tm['perm_projected']) == (route == 'projected' and rotate), (what, tm)
            if key == 'all' and route == 'fixed':
                # the scratch holds R_p = A_p Xn of the last batch (rotate=False): k_cell_scale's zeros, exactly
                Tp = eng.Tp
                for i in range(N_PERM):
                    _check_R(eng.scratch_rows(i)[:Tp, :eng.B], a.Rp[i], a.const0, T, what + ' R of permutation %d' % i)
        finally:
            eng.close()
    for rotate in (True, False):
        g = got['all', rotate]
        print(what, 'rotate', rotate, 'largest', float(np.max(np.abs(g))),
              'rel err', float(np.max(np.abs(g - a.perm[rotate])) / np.max(np.abs(a.perm[rotate]))))
        assert np.all(np.isfinite(g)), what
        assert_close(g, a.perm[rotate], 1e-8, what=what + ' vs contract, rotate=%s' % rotate)
        assert_close(g, got['kept', rotate], 1e-8, what=what + ' vs the data without the constant columns')


# ---------------------------------------------------------------------------------------------------------------------
# split-half
# ---------------------------------------------------------------------------------------------------------------------

# options, T, split_blocks, split_reader.  T = 5: the fused epilogue exists for 24-tile blocks only, and below five
# behaviours per cell plan_groups prefers 16-tile blocks (the two-pass route would run whatever the options say)
SPLIT_ROUTES = {
    'two_pass': (dict(no_split_fuse=1), 5, 0, 0),
    'dense': (dict(split_inblock=1), 5, 1, 0),
    'compact5': (dict(), 5, 5, 0),
    'two_readers': (dict(split_two_readers=1), 10, 5, 0),
    'one_pass': (dict(), 10, 8, 12),
    'reader8': (dict(split_reader8=1), 10, 8, 8),
}


@functools.lru_cache(maxsize=None)
def _split_case(design, B, T):
    from pypyls_amd import resampling as rsmp
    a = _case(design, B, T)
    ns, n_arr = 5, 2
    masks = np.stack([rsmp.gen_splits(a.groups, a.n_cond, ns, seed=40 + i) for i in range(1 + n_arr)])
    perms = a.perms[:, :n_arr]
    want = []
    with cc.contract():
        for p in range(1 + n_arr):
            Yp = a.Y if p == 0 else a.Y[perms[:, p - 1]]
            U, d, V = ref.decompose(a.spec, a.X, Yp)
            di = np.linalg.inv(d)
            uv = [ref.split_half(a.spec, a.X, Yp, U @ di, V @ di, masks[p][:, [i]]) for i in range(ns)]
            want.append((np.stack([u for u, _ in uv], -1), np.stack([v for _, v in uv], -1)))
    return a, masks, perms, want


# the one-pass reader starts at T'pp = 20: [20, 20] x 1 with T = 10
SPLIT_CASES = [(r, d, 70) for r in ('two_pass', 'dense', 'compact5') for d in ('2g', '3c', '1g')] + \
    [('two_readers', '2g', 70), ('one_pass', '2g', 130), ('reader8', '2g', 70)]


@pytest.mark.parametrize('route,design,B', SPLIT_CASES, ids=lambda v: str(v))
def test_split_half_routes(route, design, B):
    options, T, blocks, reader = SPLIT_ROUTES[route]
    a, masks, perms, want = _split_case(design, B, T)
    what = 'split-half {} {} B={} T={}'.format(route, design, B, T)
    got = {}
    for key, X in (('all', a.X), ('kept', a.X[:, a.keep])):
        eng = _engine(a, X=X, **options)
        try:
            o = eng.split_half(masks[0])
            tm = eng.last_timing()
            print(what, key, 'split_blocks', tm['split_blocks'], 'split_reader', tm['split_reader'], 'route', eng.split_route())
            assert (tm['split_blocks'], tm['split_reader'] % 100) == (blocks, reader), (what, tm)
            assert eng.split_route() == (1 if blocks == 8 else 0)
            p = eng.split_half(masks[1:], perms=perms)
            got[key] = [(o[0][0], o[1][0])] + [(p[0][i], p[1][i]) for i in range(perms.shape[1])]
        finally:
            eng.close()
    for p, ((uc, vc), (wu, wv), (_, kv)) in enumerate(zip(got['all'], want, got['kept'])):
        print(what, 'arrangement', p, 'ucorr err', float(np.max(np.abs(uc - wu))), 'vcorr err', float(np.max(np.abs(vc - wv))))
        assert np.all(np.isfinite(uc)) and np.all(np.isfinite(vc)), what
        assert_close(uc, wu, 1e-7, what=what + ' ucorr vs contract')
        assert_close(vc, wv, 1e-7, what=what + ' vcorr vs contract')
        # (ucorr is a correlation over the features, zero entries included: only vcorr is that of the data without them)
        assert_close(vc, kv, 1e-7, what=what + ' vcorr vs the data without the constant columns')


# ---------------------------------------------------------------------------------------------------------------------
# cross-validation: a feature that is constant on a training cell maps the cell's test rows to 0
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [('2g', 70), ('3c', 130), ('1g', 70)], ids=lambda s: '{}-B{}'.format(*s))
def test_crossval(shape):
    a = _case(*shape)
    m = 4
    train = np.ones((len(a.X), m), bool)
    for i in range(m):
        for j, rows in enumerate(a.cells):
            train[rows[i::4], i] = False
            if i == j:
                train[a.sparse_rows[j], i] = False        # the sparse column: constant on this training cell only
    with cc.contract():
        want_r, want_r2 = ref.crossval(a.spec, a.X, a.Y, train)
        kept_r, kept_r2 = ref.crossval(a.spec, a.X[:, a.keep], a.Y, train)
    assert np.all(np.isfinite(want_r)) and np.allclose(want_r, kept_r, rtol=0, atol=1e-10)
    eng = _engine(a)
    try:
        r, r2 = eng.crossval(train)
        kt = eng.kernel_timing()
    finally:
        eng.close()
    print('crossval', shape, sorted(kt), 'r err', float(np.max(np.abs(r - want_r))), 'r2 err', float(np.max(np.abs(r2 - want_r2))))
    assert 'k_xprod' in kt and 'k_xprod_moments' not in kt        # in-block moments with the training mean / scale export
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(r2))
    assert np.max(np.abs(r - want_r)) <= 1e-7
    assert np.all(np.abs(r2 - want_r2) <= 1e-7 * np.maximum(1.0, np.abs(want_r2)))


# ---------------------------------------------------------------------------------------------------------------------
# one public call
# ---------------------------------------------------------------------------------------------------------------------

def _arrays(res, prefix=''):
    for k, v in res.items():
        if k == 'inputs':
            continue
        if hasattr(v, 'items'):
            for item in _arrays(v, prefix + k + '.'):
                yield item
        elif isinstance(v, np.ndarray) and v.dtype.kind == 'f':
            yield prefix + k, v


def test_public_call_with_a_group_indicator_column():
    import pypyls_amd as pls
    a = _case('2g', 70)
    live = np.setdiff1d(a.keep, [a.sparse] + [b for b, _ in a.partial])
    cols = np.sort(np.r_[live, a.indicator])
    others = cols != a.indicator
    kw = dict(groups=a.groups, n_perm=40, n_boot=40, n_split=6, test_split=5, seed=7, verbose=False)
    res = pls.behavioral_pls(a.X[:, cols], a.Y, **kw)
    ref_res = pls.behavioral_pls(a.X[:, live], a.Y, **kw)
    for name, v in _arrays(res):
        assert np.all(np.isfinite(v)), name
    n = kw['n_perm'] + 1
    assert np.array_equal(np.rint(res.permres.pvals * n), np.rint(ref_res.permres.pvals * n))
    assert_close(res.permres.perm_singval, ref_res.permres.perm_singval, 1e-8, what='perm_singval')
    assert_close(res.singvals, ref_res.singvals, 1e-9, what='singvals')
    assert not res.x_weights[~others].any() and not res.bootres.x_weights_normed[~others].any()
    assert_close(res.bootres.x_weights_normed[others], ref_res.bootres.x_weights_normed, 1e-7, what='bootstrap ratios')
    assert_close(res.bootres.x_weights_stderr[others], ref_res.bootres.x_weights_stderr, 1e-7, what='standard errors')
    assert_close(res.bootres.y_loadings_boot, ref_res.bootres.y_loadings_boot, 1e-7, what='y_loadings_boot')
    assert_close(res.splitres.vcorr, ref_res.splitres.vcorr, 1e-7, what='vcorr')
    assert np.array_equal(np.rint(res.splitres.vcorr_pvals * n), np.rint(ref_res.splitres.vcorr_pvals * n))
    assert_close(res.cvres.pearson_r, ref_res.cvres.pearson_r, 1e-7, what='cross-validated r')


# ---------------------------------------------------------------------------------------------------------------------
# the other side of the threshold: a nearly constant feature keeps its value
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', sorted(BOOT_ROUTES) + ['fixed'])
def test_small_coefficient_of_variation_keeps_its_value(route):
    """Within-cell coefficient of variation 1e-3 (std over the root mean square of the globally centred values): the
    raw-moment routes may lose 4 (n + 1) 2^-53 / CV^2 of the entry -- the rounding bound of m2 - m1^2 / n, which is also
    the rule's threshold -- and the two-pass fixed-X route nothing beyond the 1e-10 of every other entry."""
    from pypyls_amd import resampling as rsmp
    groups, n_cond = cc.DESIGNS['2g']
    spec = ref.Spec('behavioral', groups, n_cond)
    rs = np.random.RandomState(11)
    S, B, T, b = 40, 70, 4 if route == 'sepmom' else 3, 33
    X = rs.randn(S, B) + 3.0 * rs.rand(1, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    X[:, b] = np.repeat([1000.0, -1000.0], 20) + rs.randn(S)
    cells = [np.flatnonzero(c) for c in spec.dummy.T.astype(bool)]
    boots = rsmp.gen_bootsamp(groups, n_cond, 6, seed=2)
    perms = rsmp.gen_permsamp(groups, n_cond, 3, seed=1)
    Xc = X[:, b] - X[:, b].mean()

    def bound(rows):
        x = Xc[rows]
        cv2 = np.sum((x - x.mean()) ** 2) / np.sum(x * x)
        assert 2e-7 < cv2 < 5e-6                          # (CV about 1e-3, whatever rows the resample draws)
        return 4.0 * (len(rows) + 1) * 2.0 ** -53 / cv2

    class A(object):
        pass
    a = A()
    a.X, a.Y, a.groups, a.n_cond = X, Y, groups, n_cond
    others = np.arange(B) != b
    if route == 'fixed':
        eng = _engine(a, **PERM_ROUTES['fixed'])
        try:
            U, d, V = ref.decompose(spec, X, Y)
            eng.set_original(U, np.diag(d), V)
            eng.perm(perms, rotate=False)
            assert not eng.last_timing()['dual_perm']
            got = [eng.scratch_rows(i)[:eng.Tp, :B] for i in range(3)]
        finally:
            eng.close()
        for i in range(3):
            want = ref.gen_covcorr(spec, X, Y[perms[:, i]], spec.dummy)
            print('cv 1e-3 fixed', i, float(np.max(np.abs(got[i][:, b] - want[:, b])) / np.max(np.abs(want[:, b]))))
            assert_close(got[i], want, 1e-10, what='two-pass route')
            assert_close(got[i][:, b], want[:, b], 1e-10, what='two-pass route, the nearly constant feature')
        return
    eng = _engine(a, **BOOT_ROUTES[route])
    try:
        eng.set_timing(True)
        got = eng.crosscov(xsrc=boots, ysrc=boots)
        _pin_boot_route(route, eng, 'cv 1e-3 ' + route)
    finally:
        eng.close()
    for i in range(boots.shape[1]):
        want = ref.gen_covcorr(spec, X[boots[:, i]], Y[boots[:, i]], spec.dummy)
        assert_close(got[i][:, others], want[:, others], 1e-10, what='the other features')
        for j, rows in enumerate(cells):
            g, w = got[i][j * T:(j + 1) * T, b], want[j * T:(j + 1) * T, b]
            lim = bound(boots[rows, i])
            print('cv 1e-3', route, 'bootstrap', i, 'cell', j, 'rel err', float(np.max(np.abs(g - w)) / np.max(np.abs(w))), 'bound', lim)
            assert np.all(g != 0.0) and np.max(np.abs(g - w)) <= lim * np.max(np.abs(w))
