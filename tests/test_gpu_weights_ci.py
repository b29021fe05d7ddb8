"""behavioral_pls / meancentered_pls(weights_ci=m) on the device (plsx_boot_keep / plsx_boot_weights_ci: k_keep_M,
k_weights_W, k_weights_scale, k_weights_prod + the selection kernels): the public call against the oracle, every
bootstrap route, the closing entry alone against numpy across tile and cell-segment edges, chunking, cell-constant
features, ties, the limits, what must not move, a team.

Gates: RTOL = 1e-5 through conftest.assert_close against the oracle, ROUTES = 1e-9 between routes and teams, bit
equality across chunkings.  The closing entry alone is compared with numpy on the SAME stack and index rows.  In the
unscaled modes both sides are fp64 sums of S <= 1000 products and an order statistic is a continuous function of its
series: 1e-10, the derivation of tests/test_gpu_regression_coef_ci.py.  In correlation mode the device scales by
1 / std from raw moments and numpy by a two-pass z-score: whichever is larger of that bar and
cell_constant_expect.raw_moment_bound(n, cv) for the smallest within-cell coefficient of variation of the rows the
bootstraps draw.  Every figure is printed before it is asserted; no element is left out of a comparison."""
import re

import numpy as np
import pytest

from conftest import assert_close
import cell_constant_expect as cc
import weights_ci_expect as wx

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROUTES = 1e-9
NUMPY = 1e-10


def _engine(options=None, **kw):
    from pypyls_amd.engine import Engine
    return Engine(options=options or {}, **kw)


def max_rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = np.max(np.abs(b)) if b.size else 1.0
    return float(np.max(np.abs(a - b)) / scale) if b.size else 0.0


def _check(got, want, what, tol=RTOL):
    err = max_rel(got, want)
    print('{}: x_weights_ci max err / scale {:.3e} (gate {:.3e})'.format(what, err, tol))
    assert not np.isnan(got).any(), what + ': NaN'
    assert_close(got, want, rtol=tol, what=what)
    assert np.all(got[..., 0] <= got[..., 1]), what + ': lower above upper'
    return err


def _same(a, b, tol, what):
    err = max_rel(a, b)
    print('{}: x_weights_ci max diff / scale {:.3e}'.format(what, err))
    assert err <= tol, (what, err)


def _data(S, B, T, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B) + 2.0 * rs.rand(1, B)
    Y = rs.randn(S, T)
    k = min(T, B)
    Y[:, :k] += 0.5 * X[:, :k]
    return X, Y


# ---------------------------------------------------------------------------------------------------------------------
# the public call against the oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('covariance', [False, True])
@pytest.mark.parametrize('B', [150, 385])
@pytest.mark.parametrize('groups,n_cond', [([24], 1), ([13, 18], 2), ([40], 3)])
def test_public_call_against_the_oracle(groups, n_cond, B, covariance):
    """One cell, four cells whose segment edges (13, 26, 44) are no multiple of the 4-subject k-step, three equal cells;
    B below and above one 128-feature block and no multiple of it."""
    import pypyls_amd as pls
    S, T, n_boot = sum(groups) * n_cond, 3, 70
    X, Y = _data(S, B, T, seed=S + B)
    kw = dict(groups=groups, n_cond=n_cond, n_perm=0, n_boot=n_boot, test_split=0, covariance=covariance, seed=7,
              verbose=False)
    res = pls.behavioral_pls(X, Y, weights_ci=True, **kw)
    L = min(len(groups) * n_cond * T, B)
    got = res.bootres.x_weights_ci
    assert got.shape == (B, L, 2) and res.inputs.weights_ci is True
    spec = wx.spec_of('behavioral', groups, n_cond, covariance=covariance)
    want = wx.weights_ci_expected(spec, X, Y, res.bootres.bootsamples)
    _check(got, want, 'behavioral {}x{} B={} cov={} vs oracle'.format(groups, n_cond, B, covariance))
    two = pls.behavioral_pls(X, Y, weights_ci=2, **kw)
    assert two.bootres.x_weights_ci.shape == (B, 2, 2) and two.inputs.weights_ci == 2
    assert np.array_equal(two.bootres.x_weights_ci, got[:, :2]), 'weights_ci=2 is not [:, :2] of weights_ci=True'


@pytest.mark.parametrize('mean_centering', [0, 2])
def test_meancentered_public_call_against_the_oracle(mean_centering):
    import pypyls_amd as pls
    groups, n_cond, B = [11, 14, 9], 2, 150
    X, _ = _data(sum(groups) * n_cond, B, 1, seed=11 + mean_centering)
    X += np.repeat(np.random.RandomState(5).randn(6, B), np.repeat(groups, n_cond), axis=0)      # (cell effects)
    kw = dict(groups=groups, n_cond=n_cond, mean_centering=mean_centering, n_perm=0, n_boot=70, seed=3, verbose=False)
    res = pls.meancentered_pls(X, weights_ci=True, **kw)
    got = res.bootres.x_weights_ci
    assert got.shape == (B, 6, 2)
    spec = wx.spec_of('meancentered', groups, n_cond, mean_centering=mean_centering)
    want = wx.weights_ci_expected(spec, X, None, res.bootres.bootsamples)
    _check(got, want, 'meancentered mc={} vs oracle'.format(mean_centering))
    two = pls.meancentered_pls(X, weights_ci=2, **kw)
    assert np.array_equal(two.bootres.x_weights_ci, got[:, :2])


# ---------------------------------------------------------------------------------------------------------------------
# every bootstrap route keeps the same M
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('covariance,routes', [
    (False, [{}, {'no_compact_boot': 1}, {'compact_boot_always': 1}, {'two_pass_boot': 1}]),
    (True, [{}, {'quad_sums': -1}, {'quad_sums': 1}, {'two_pass_boot': 1}]),
])
def test_every_bootstrap_route_keeps_the_same_rotation_operands(covariance, routes):
    import pypyls_amd as pls
    groups, n_cond, B, T = [13, 18], 2, 385, 3
    X, Y = _data(sum(groups) * n_cond, B, T, seed=21)
    spec = wx.spec_of('behavioral', groups, n_cond, covariance=covariance)
    runs, want = [], None
    for opts in routes:
        eng = _engine(opts)
        try:
            res = pls.behavioral_pls(X, Y, groups=groups, n_cond=n_cond, n_perm=0, n_boot=70, test_split=0,
                                     covariance=covariance, seed=9, verbose=False, weights_ci=True, _engine=eng)
        finally:
            eng.close()
        if want is None:
            want = wx.weights_ci_expected(spec, X, Y, res.bootres.bootsamples)
        _check(res.bootres.x_weights_ci, want, 'cov={} route {} vs oracle'.format(covariance, opts))
        runs.append(res.bootres.x_weights_ci)
    for opts, other in zip(routes, runs):
        _same(runs[0], other, ROUTES, 'cov={} default vs {}'.format(covariance, opts))


@pytest.mark.parametrize('S,T', [(100, 72), (130, 104)])
def test_the_householder_solver_keeps_its_rotation_operands(S, T):
    """T' = 72 > 64: k_small_ql, five 16-column tiles of L in fragment order; T' = 104: seven tiles, so a second chunk
    of the rotation operand (PLSX_LT_CHUNK = 6)."""
    import pypyls_amd as pls
    B = 150
    X, Y = _data(S, B, T, seed=31)
    res = pls.behavioral_pls(X, Y, n_perm=0, n_boot=24, test_split=0, seed=2, verbose=False, weights_ci=True)
    got = res.bootres.x_weights_ci
    assert got.shape == (B, T, 2)
    want = wx.weights_ci_expected(wx.spec_of('behavioral', [S]), X, Y, res.bootres.bootsamples)
    _check(got, want, "T' = {} vs oracle".format(T))


# ---------------------------------------------------------------------------------------------------------------------
# the closing entry alone
# ---------------------------------------------------------------------------------------------------------------------

def _cells_for(S, Tp, unequal):
    """(groups, T) with len(groups) * T == T': one cell, or J cells of unequal size whose edges are no multiple of 4
    (J the smallest divisor of T' above 1).  T' = 1 is one row of R and so one cell: that shape has no second layout."""
    if not unequal or Tp == 1:
        return [S], Tp
    J = 2 if Tp % 2 == 0 else 3
    assert Tp % J == 0
    groups = [S // 2 - 2, S - (S // 2 - 2)] if J == 2 else [S // 3 - 3, S // 3 + 1, S - 2 * (S // 3) + 2]
    assert sum(groups) == S and min(groups) >= 2 and all(e % 4 for e in np.cumsum(groups)[:-1])
    return groups, Tp // J


def _bind(eng, spec, X, Y):
    from pypyls_amd import resampling
    cells = resampling.cell_of_row(spec.groups, spec.n_cond)
    eng.set_data(X, Y, cells, len(spec.groups), spec.n_cond, 0 if spec.method == 'behavioral' else 1,
                 mean_centering=spec.mean_centering, covariance=spec.covariance)


def _closing(eng, rows, M, ci):
    lo, hi = eng.boot_weights_ci(eng.rows_tensor(rows), eng._dev(M, np.float64), ci=ci)
    eng.sync()
    return np.stack([lo.cpu().numpy(), hi.cpu().numpy()], -1)


def _cv_bound(spec, X, rows):
    """raw_moment_bound for the least favourable (bootstrap, cell, feature) of the rows drawn."""
    Xc = X - X.mean(axis=0)
    worst = 0.0
    for c in spec.dummy.T.astype(bool):
        idx = np.flatnonzero(c)
        G = Xc[rows[:, idx]]                                               # (n, n_c, B)
        cv = G.std(axis=1, ddof=1) / np.sqrt((G ** 2).mean(axis=1))
        worst = max(worst, cc.raw_moment_bound(len(idx), float(cv.min())))
    return worst


@pytest.mark.parametrize('covariance', [False, True])
@pytest.mark.parametrize('unequal', [False, True])
@pytest.mark.parametrize('S,B,Tp,m,n', [(37, 150, 3, 3, 70), (5, 17, 1, 1, 1), (130, 129, 2, 2, 2), (33, 257, 1, 1, 3),
                                        (64, 128, 2, 1, 64), (31, 385, 20, 17, 65)])
def test_closing_entry_alone_against_numpy_across_tile_edges(S, B, Tp, m, n, unequal, covariance):
    """A random stack (not orthogonal) and random within-cell index rows, no solver: B, n, S on and off the multiples of
    128 / 64 / 32 / 4 the tiles are made of; odd S takes the unaligned loads of the stack; with two cells the segment edge
    falls inside a k-step and inside an LDS stage."""
    groups, T = _cells_for(S, Tp, unequal)
    spec = wx.spec_of('behavioral', groups, 1, covariance=covariance)
    rs = np.random.RandomState(S + B + n + 7 * unequal)
    X, Y = _data(S, B, T, seed=S * B + n)
    rows = wx.within_cell_rows(spec, n, rs)
    M = rs.randn(n, m, Tp)
    eng = _engine()
    try:
        _bind(eng, spec, X, Y)
        assert eng.Tp == Tp
        tol = NUMPY if covariance else max(NUMPY, _cv_bound(spec, X, rows))
        for ci in (95, 80):
            got = _closing(eng, rows, M, ci)
            assert got.shape == (B, m, 2)
            _check(got, wx.stack_ci(spec, X, Y, rows, M, ci),
                   'closing S={} B={} T\'={} m={} n={} cells={} cov={} ci={}'.format(S, B, Tp, m, n, groups, covariance, ci),
                   tol=tol)
    finally:
        eng.close()


@pytest.mark.parametrize('mean_centering', [0, 1, 2])
def test_closing_entry_alone_meancentered(mean_centering):
    groups, n_cond, B, n = [11, 14, 9], 2, 150, 33
    spec = wx.spec_of('meancentered', groups, n_cond, mean_centering=mean_centering)
    rs = np.random.RandomState(40 + mean_centering)
    X, _ = _data(68, B, 1, seed=41)
    rows = wx.within_cell_rows(spec, n, rs)
    M = rs.randn(n, 4, 6)
    eng = _engine()
    try:
        _bind(eng, spec, X, None)
        got = _closing(eng, rows, M, 95)
        _check(got, wx.stack_ci(spec, X, None, rows, M, 95), 'closing meancentered mc={}'.format(mean_centering), tol=NUMPY)
    finally:
        eng.close()


def test_chunking_leaves_every_bit_where_it_is():
    """S = 200, B = 600, T' = 10, m = 10, n = 2000 in correlation mode: one chunk under the default budget, five chunks
    of one 128-feature block under the smallest budget the entry admits (it names its need, and refuses one byte
    below), and the full sort: the same bits; k_weights_prod is launched once per chunk."""
    from pypyls_amd.engine import PlsxError
    S, B, T, m, n = 200, 600, 10, 10, 2000
    spec = wx.spec_of('behavioral', [S], 1)
    rs = np.random.RandomState(77)
    X, Y = _data(S, B, T, seed=78)
    rows = wx.within_cell_rows(spec, n, rs)
    M = rs.randn(n, m, T)

    def run(**kw):
        eng = _engine(**kw)
        try:
            _bind(eng, spec, X, Y)
            eng.set_timing(True)
            out = _closing(eng, rows, M, 95)
            return out, eng.kernel_timing()['k_weights_prod'][1]
        finally:
            eng.close()

    with pytest.raises(PlsxError, match=r'status -2') as exc:
        run(scratch_gb=1e-6)
    need = int(re.search(r'need (\d+) bytes', str(exc.value)).group(1))
    print('smallest budget: {} bytes; refusal: {}'.format(need, exc.value))
    assert need > 8 * n * m * (T + S)
    with pytest.raises(PlsxError, match=r'status -2.*need {} bytes'.format(need)):
        run(scratch_gb=(need - 1) / 2.0 ** 30)
    whole, launches = run()
    small, launches_small = run(scratch_gb=need / 2.0 ** 30)
    sort, _ = run(options={'percentile_sort': 1})
    print('k_weights_prod launches: default budget {}, smallest budget {}'.format(launches, launches_small))
    assert launches == 1 and launches_small == -(-B // 128)
    assert np.array_equal(whole, small), 'chunking moved bits'
    assert np.array_equal(whole, sort), 'the full sort moved bits'
    assert not np.isnan(whole).any() and np.all(whole[..., 0] <= whole[..., 1])


# ---------------------------------------------------------------------------------------------------------------------
# cell-constant features, ties
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('design', ['2g', '3c', '1g'])
def test_cell_constant_features_scale_to_zero(design):
    import pypyls_amd as pls
    a = cc.armed(design, 150, 3, seed=0)
    boots = cc.sparse_bootstraps(a, 48, seed=1)
    res = pls.behavioral_pls(a.X, a.Y, groups=a.groups, n_cond=a.n_cond, n_perm=0, n_boot=48, bootsamples=boots,
                             test_split=0, seed=1, verbose=False, weights_ci=True)
    got = res.bootres.x_weights_ci
    with cc.contract():
        want = wx.weights_ci_expected(a.spec, a.X, a.Y, boots)
    _check(got, want, 'armed {} vs the contract'.format(design))
    print('armed {}: dead columns max |bound| {:.3e}'.format(design, np.abs(got[a.dead]).max()))
    assert np.all(got[a.dead] == 0.0), 'a column that is dead in every cell has a non-zero interval'


def test_ties_and_replication_at_the_batch_geometry():
    """2400 bootstraps that are 6 distinct samples, replicated with unequal counts, the first and last positions
    permuted: every series is six values with heavy ties."""
    import pypyls_amd as pls
    groups, n_cond, B, T = [13, 18], 2, 150, 3
    X, Y = _data(sum(groups) * n_cond, B, T, seed=51)
    spec = wx.spec_of('behavioral', groups, n_cond)
    rs = np.random.RandomState(52)
    six = wx.within_cell_rows(spec, 6, rs).T                               # (S, 6)
    counts = np.array([700, 1, 399, 800, 300, 200])
    which = np.repeat(np.arange(6), counts)
    which[[0, -1]] = which[[-1, 0]]
    boots = six[:, which]
    for ci in (95, 80):
        res = pls.behavioral_pls(X, Y, groups=groups, n_cond=n_cond, n_perm=0, n_boot=2400, bootsamples=boots,
                                 test_split=0, ci=ci, seed=1, verbose=False, weights_ci=True)
        U, d = wx.original(spec, X, Y)
        want = wx.ci_of(wx.weights_boot(spec, X, Y, six, U, d), ci=ci, weights=counts)
        _check(res.bootres.x_weights_ci, want, 'replicated bootstraps ci={}'.format(ci))


# ---------------------------------------------------------------------------------------------------------------------
# limits, what must not move, a team
# ---------------------------------------------------------------------------------------------------------------------

def test_limits_and_state_errors_leave_the_context_usable():
    import torch
    from pypyls_amd.engine import PlsxError
    S, B, T = 24, 40, 2
    spec = wx.spec_of('behavioral', [S], 1)
    rs = np.random.RandomState(61)
    X, Y = _data(S, B, T, seed=62)
    eng = _engine()
    try:
        _bind(eng, spec, X, Y)
        rows = wx.within_cell_rows(spec, 8, rs)
        big = np.tile(rows, (2049, 1))[:16385]
        M = rs.randn(16385, 1, T)
        with pytest.raises(PlsxError, match=r'status -2.*16384'):
            _closing(eng, big, M, 95)
        got = _closing(eng, big[:16384], M[:16384], 95)                     # n = 16384 runs, on the refused context
        assert got.shape == (B, 1, 2) and not np.isnan(got).any() and np.all(got[..., 0] <= got[..., 1])
        _check(_closing(eng, rows, M[:8], 95), wx.stack_ci(spec, X, Y, rows, M[:8], 95), 'after the refusal',
               tol=max(NUMPY, _cv_bound(spec, X, rows)))
        # argument errors of the C entry
        d_rows, d_M = eng.rows_tensor(rows), eng._dev(M[:8], np.float64)
        lo, hi = eng._empty((B, 1)), eng._empty((B, 1))
        for n, m, i_lo, i_hi in ((0, 1, 0, 0), (8, 0, 0, 7), (8, 3, 0, 7), (8, 1, -1, 7), (8, 1, 0, 8)):
            rc = eng.lib.plsx_boot_weights_ci(eng.ctx, d_rows.data_ptr(), d_M.data_ptr(), n, m, i_lo, 0.0, i_hi, 0.0,
                                              lo.data_ptr(), hi.data_ptr(), eng._stream())
            assert rc == -1, (n, m, i_lo, i_hi, rc)
        assert eng.lib.plsx_boot_weights_ci(eng.ctx, None, d_M.data_ptr(), 8, 1, 0, 0.0, 7, 0.0, lo.data_ptr(),
                                            hi.data_ptr(), eng._stream()) == -1
        # keeping needs a set original
        stack = eng._zeros((3, 2, T))
        with pytest.raises(PlsxError, match='status -4'):
            eng.boot_keep(stack)
        d_xw, d_sv, d_yw = eng.decompose_dev()
        eng.svd_flip(d_xw, d_yw)
        eng.set_original(d_xw, d_sv, d_yw)
        with pytest.raises(PlsxError, match='status -1'):
            eng.boot_keep(eng._zeros((3, 3, T)))                            # m = 3 > L = 2
        eng.boot_keep(stack)
        usum, usq, dist = eng._zeros((B, 2)), eng._zeros((B, 2)), eng._zeros((5, T, 2))
        with pytest.raises(PlsxError, match='status -1'):
            eng.boot_into(eng.rows_tensor(rows[:5]), usum, usq, dist)       # 5 bootstraps, room for 3
        eng.sync()
        for t in (usum, usq, dist, stack):
            assert not bool(torch.any(t != 0).item()), 'the refused batch computed something'
        eng.boot_into(eng.rows_tensor(rows[:3]), usum, usq, dist[:3])       # the context is usable, the stack fills
        eng.sync()
        kept = stack.cpu().numpy()
        assert np.all(np.abs(kept).sum(axis=(1, 2)) > 0)
        # ... and the kept operands reproduce the sums the batch added
        series = wx.stack_series(spec, X, Y, rows[:3], kept)
        assert_close(series.sum(axis=-1), usum.cpu().numpy(), rtol=RTOL, what='kept M vs usum')
        # ending the keeping: a later batch leaves the stack alone
        eng.boot_keep(None)
        eng.boot_into(eng.rows_tensor(rows[3:8]), usum, usq, dist)
        eng.sync()
        assert np.array_equal(stack.cpu().numpy(), kept)
        # contrasts: not kept
        eng.set_contrasts(np.linalg.qr(rs.randn(T, 1))[0])
        with pytest.raises(PlsxError, match='status -2'):
            eng.boot_keep(stack)
        # regression data: no PLS-C data bound
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), 2)
        with pytest.raises(PlsxError, match='status -4'):
            eng._check(eng.lib.plsx_boot_keep(eng.ctx, stack.data_ptr(), 3, 2))
        rc = eng.lib.plsx_boot_weights_ci(eng.ctx, d_rows.data_ptr(), d_M.data_ptr(), 8, 1, 0, 0.0, 7, 0.0,
                                          lo.data_ptr(), hi.data_ptr(), eng._stream())
        assert rc == -4
    finally:
        eng.close()
    # multiblock data: refused by both entries
    eng = _engine()
    try:
        from pypyls_amd import resampling
        eng.set_data(X, Y, resampling.cell_of_row([12, 12], 1), 2, 1, 3)
        with pytest.raises(PlsxError, match='status -2'):
            eng.boot_weights_ci(eng.rows_tensor(rows), eng._dev(rs.randn(8, 1, eng.Tp), np.float64))
    finally:
        eng.close()


def _flatten(res, prefix=''):
    out = {}
    for key, val in res.items():
        if key == 'inputs':
            continue
        if isinstance(val, dict):
            out.update(_flatten(val, prefix + key + '.'))
        elif val is not None:
            out[prefix + key] = np.asarray(val)
    return out


def test_nothing_else_moves_and_the_call_is_reproducible():
    import pypyls_amd as pls
    groups, n_cond, B, T = [13, 18], 2, 150, 3
    X, Y = _data(sum(groups) * n_cond, B, T, seed=71)
    kw = dict(groups=groups, n_cond=n_cond, n_perm=20, n_boot=30, n_split=4, test_split=5, seed=1234, verbose=False)
    off = _flatten(pls.behavioral_pls(X, Y, **kw))
    on = _flatten(pls.behavioral_pls(X, Y, weights_ci=True, **kw))
    again = _flatten(pls.behavioral_pls(X, Y, weights_ci=True, **kw))
    assert set(on) - set(off) == {'bootres.x_weights_ci'} and set(off) <= set(on), sorted(set(on) ^ set(off))
    for key in sorted(off):
        same = np.array_equal(off[key], on[key], equal_nan=True)
        print('{}: {}'.format(key, 'same bits' if same else 'MOVED'))
        assert same, key
    for key in sorted(on):
        assert np.array_equal(on[key], again[key], equal_nan=True), key + ' differs between two runs'
    for method_kw in (dict(mean_centering=0), dict(mean_centering=2)):
        mkw = dict(groups=groups, n_cond=n_cond, n_perm=10, n_boot=30, seed=5, verbose=False, **method_kw)
        off = _flatten(pls.meancentered_pls(X, **mkw))
        on = _flatten(pls.meancentered_pls(X, weights_ci=2, **mkw))
        assert set(on) - set(off) == {'bootres.x_weights_ci'}
        for key in sorted(off):
            assert np.array_equal(off[key], on[key], equal_nan=True), key


@pytest.mark.parametrize('covariance', [False, True])
def test_a_team_of_two_agrees_with_one_device(covariance):
    import pypyls_amd as pls
    groups, n_cond, B, T = [13, 18], 2, 385, 3
    X, Y = _data(sum(groups) * n_cond, B, T, seed=81)
    kw = dict(groups=groups, n_cond=n_cond, n_perm=0, n_boot=70, test_split=0, covariance=covariance, seed=4,
              verbose=False, weights_ci=True)
    one = pls.behavioral_pls(X, Y, **kw)
    team = pls.behavioral_pls(X, Y, device_ids=[0, 0], **kw)
    assert np.array_equal(one.bootres.bootsamples, team.bootres.bootsamples)
    _same(one.bootres.x_weights_ci, team.bootres.x_weights_ci, ROUTES, 'team of two vs one device cov={}'.format(covariance))
    spec = wx.spec_of('behavioral', groups, n_cond, covariance=covariance)
    _check(team.bootres.x_weights_ci, wx.weights_ci_expected(spec, X, Y, team.bootres.bootsamples),
           'team of two vs oracle cov={}'.format(covariance))
