"""pls_regression(coef_components=c, coef_ci=True) on the device (plsx_simpls_coef_keep / plsx_simpls_coef_ci,
k_coef_prod + the selection kernels): the reference fixtures through the public call, the oracle on both solver routes
and both routes of the weights, the closing entry alone against numpy (tile edges, the timed geometry, chunking, the
full sort), the limits, batch geometry with heavy ties, what must not move, reproducibility, a team, a cohort past the
on-chip bound.

Gates: RTOL = 1e-5 through conftest.assert_close against reference and oracle, 1e-9 between routes -- the bars of
tests/test_gpu_regression_coef.py.  The closing entry alone is compared with numpy on the SAME stack: both sides are
fp64 sums of S <= 1000 products (rounding <= S 2^-53 sum |x a|, about 1e-12 of the largest bound for these inputs) and
an order statistic is a continuous function of its series, so that comparison is held to 1e-10.  Every figure is
printed before it is asserted; no element is left out of a comparison."""
import numpy as np
import pytest

from conftest import load_golden, assert_close
from regression_coef_expect import coef_expected, max_rel, packed_bootsamples
from regression_coef_ci_expect import coef_boot, ci_of, coef_ci_expected, stack_ci

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROUTES = 1e-9
NUMPY = 1e-10


def _engine(glob=False, quad=0, sort=False, **kw):
    from pypyls_amd.engine import Engine
    opts = {}
    if glob:
        opts['simpls_global'] = 1
    if quad:
        opts['quad_sums'] = quad
    if sort:
        opts['percentile_sort'] = 1
    return Engine(options=opts, **kw)


def _case(tag):
    g = load_golden('simpls_coef_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    third = g.get('third')
    bs = g['bootsamples'] if third is None else packed_bootsamples(g['bootsamples'], third)
    kw = dict(n_components=k, n_perm=0, n_boot=g['bootsamples'].shape[1], bootsamples=bs, aggfunc=aggfunc, seed=1,
              verbose=False)
    return g, k, c, aggfunc, third, kw


def _check(got, want, what, tol=RTOL):
    err = max_rel(got, want)
    print('{}: coefs_ci max err / scale {:.3e}'.format(what, err))
    assert_close(got, want, rtol=tol, what=what)
    assert np.all(got[..., 0] <= got[..., 1]), what + ': lower above upper'
    return err


def _same(a, b, tol, what):
    err = max_rel(a, b)
    print('{}: coefs_ci max diff / scale {:.3e}'.format(what, err))
    assert err <= tol, (what, err)


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_fixtures_through_the_public_call(tag):
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case(tag)
    f = load_golden('simpls_coef_ci_' + tag)
    B, T = g['X'].shape[1], g['Y'].shape[1]
    for i, level in enumerate(f['ci']):
        res = pls.pls_regression(g['X'], g['Y'], coef_components=c, coef_ci=True, ci=float(level), **kw)
        got = res.bootres.coefs_ci
        assert got.shape == (B, T, 2)
        _check(got, f['ref_ci'][i], 'simpls_coef_ci_{} ci={:g} vs reference'.format(tag, level))
        assert res.inputs.coef_ci is True and res.inputs.coef_components == c


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_oracle_on_both_solver_routes_and_both_weight_routes(tag):
    """c < k and c = k; on-chip and global solver route; weights in place (quad_sums = -1) and through the quadratic
    form (quad_sums = 1): the kept stack, and so the intervals, are the same under all of them."""
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case(tag)
    for cc in sorted({c, k} | ({2} if k > 2 else set())):
        want = coef_ci_expected(g['X'], g['Y'], g['bootsamples'], k, cc, aggfunc=aggfunc, third=third)
        runs = {}
        for glob in (False, True):
            for quad in (-1, 1):
                eng = _engine(glob, quad)
                try:
                    res = pls.pls_regression(g['X'], g['Y'], coef_components=cc, coef_ci=True, _engine=eng, **kw)
                finally:
                    eng.close()
                name = '{} c={} {} quad_sums={}'.format(tag, cc, 'global' if glob else 'on-chip', quad)
                _check(res.bootres.coefs_ci, want, name + ' vs oracle')
                runs[(glob, quad)] = res.bootres.coefs_ci
        for key, other in runs.items():
            _same(runs[(False, -1)], other, ROUTES, '{} c={} on-chip/-1 vs {}'.format(tag, cc, key))


def _bind(eng, S, B, T, k, seed):
    rs = np.random.RandomState(seed)
    X, Y = rs.randn(S, B), rs.randn(S, T)
    Xc = X - X.mean(axis=0)
    eng.set_data_regression(Xc, Y - Y.mean(axis=0), k)
    return Xc - Xc.mean(axis=0), rs                    # (the device centres what it is given once more)


def _closing(eng, stack, ci):
    lo, hi = eng.simpls_coef_ci(eng._dev(stack, np.float64), ci=ci)
    eng.sync()
    return np.stack([lo.cpu().numpy(), hi.cpu().numpy()], -1)


@pytest.mark.parametrize('S,B,T,n', [(37, 150, 3, 70), (5, 17, 1, 1), (130, 129, 2, 2), (33, 257, 1, 3),
                                     (64, 128, 2, 64), (31, 385, 4, 65)])
def test_closing_entry_alone_against_numpy_across_tile_edges(S, B, T, n):
    """A random stack, no solver: B, n, S on and off the multiples of 128 / 64 / 16 / 4 the tiles are made of, one to
    three bootstraps, one behaviour; odd S takes the unaligned loads of the stack."""
    eng = _engine()
    try:
        Xc, rs = _bind(eng, S, B, T, 1, seed=S + B + n)
        stack = rs.randn(n, T, S)
        for ci in (95, 80):
            got = _closing(eng, stack, ci)
            assert got.shape == (B, T, 2)
            err = _check(got, stack_ci(Xc, stack, ci), 'closing S={} B={} T={} n={} ci={}'.format(S, B, T, n, ci), tol=NUMPY)
            assert err <= NUMPY
    finally:
        eng.close()


def test_closing_entry_at_the_timed_geometry_chunked_unchunked_and_sorted():
    """S = 1000, T = 20, n = 5000, B = 600: 0.8 GB of stack, 0.48 GB of series.  A 1 GB scratch budget leaves room for
    256 features per chunk (three chunks); percentile_sort = 1 takes the full sort.  Each entry is one block's
    contraction whatever the chunk: all three results have the same bits."""
    S, B, T, n = 1000, 600, 20, 5000
    rs = np.random.RandomState(5)
    stack = rs.randn(n, T, S)
    stack[:, 3] = np.round(stack[:, 3])                # one behaviour full of ties
    want = None
    got = {}
    for name, kw in (('default', {}), ('scratch 1 GB', dict(scratch_gb=1.0)), ('percentile_sort', dict(sort=True))):
        eng = _engine(**kw)
        try:
            Xc, _ = _bind(eng, S, B, T, 2, seed=6)
            if want is None:
                want = stack_ci(Xc, stack, 95)
            eng.set_timing(True)
            got[name] = _closing(eng, stack, 95)
            kt = eng.kernel_timing()
            print('{}: {}'.format(name, {key: kt[key] for key in ('k_coef_prod', 'k_percentile')}))
            launches = kt['k_coef_prod'][1]
            assert launches == (3 if name == 'scratch 1 GB' else 1), (name, launches)
            assert kt['k_percentile'][1] == launches
        finally:
            eng.close()
        _check(got[name], want, 'timed geometry, {} vs numpy'.format(name), tol=NUMPY)
    for name in ('scratch 1 GB', 'percentile_sort'):
        assert np.array_equal(got['default'], got[name]), name


def test_limits_and_refusals_leave_the_context_usable():
    from pypyls_amd.engine import PlsxError
    S, B, T = 64, 100, 2
    eng = _engine()
    try:
        Xc, rs = _bind(eng, S, B, T, 2, seed=9)
        stack = rs.randn(16385, T, S)
        d_stack = eng._dev(stack, np.float64)
        with pytest.raises(PlsxError, match='status -2.*16384'):
            eng.simpls_coef_ci(d_stack, ci=95)
        got = _closing(eng, stack[:16384], 95)         # the largest series the kernels take; the context still works
        _check(got, stack_ci(Xc, stack[:16384], 95), 'n = 16384', tol=NUMPY)
        with pytest.raises(PlsxError, match='status -1'):
            eng._check(eng.lib.plsx_simpls_coef_ci(eng.ctx, d_stack.data_ptr(), 10, 10, 0.0, 3, 0.0, d_stack.data_ptr(),
                                                   d_stack.data_ptr(), None))          # index outside 0 .. n - 1
        with pytest.raises(PlsxError, match='status -1'):
            eng._check(eng.lib.plsx_simpls_coef_ci(eng.ctx, None, 10, 1, 0.0, 3, 0.0, d_stack.data_ptr(),
                                                   d_stack.data_ptr(), None))
        # keeping needs an open series; a batch that would overflow the kept stack is refused before it computes
        d_W, _, _ = eng.simpls_decompose_dev()
        eng.simpls_set_original_dev(d_W)
        keep = eng._zeros((3, T, S))
        with pytest.raises(PlsxError, match='status -4'):
            eng.simpls_coef_keep(keep)
        eng.simpls_coef_begin(2)
        eng.simpls_coef_keep(keep)
        boots = rs.randint(0, S, size=(S, 5))
        usum, usq, yl = eng._zeros((B, 2)), eng._zeros((B, 2)), eng._zeros((5, T, 2))
        with pytest.raises(PlsxError, match='status -1.*kept'):
            eng.simpls_boot_into(eng.rows_tensor(boots.T), usum, usq, yl)
        assert float(usum.abs().sum()) == 0.0 and float(keep.abs().sum()) == 0.0
        eng.simpls_boot_into(eng.rows_tensor(boots.T[:3]), usum, usq, yl[:3])
        bsum, bsq = eng._zeros((B, T)), eng._zeros((B, T))
        eng.simpls_coef_finish(bsum, bsq)
        eng.sync()
        # what was kept is the series' own A_b: Xc^T A_b summed is what _finish adds up
        kept = keep.cpu().numpy()
        boot = np.einsum('sf,nts->nft', Xc, kept)
        assert_close(boot.sum(axis=0), bsum.cpu().numpy(), rtol=ROUTES, what='kept stack vs coefficient sums')
        assert_close((boot ** 2).sum(axis=0), bsq.cpu().numpy(), rtol=ROUTES, what='kept stack vs sums of squares')
        with pytest.raises(PlsxError, match='status -4'):
            eng.simpls_coef_keep(keep)                 # _finish ended the keeping with the series
    finally:
        eng.close()
    # a stack that cannot fit the scratch budget: refused the same way, asked through a small budget
    eng = _engine(scratch_gb=0.25)
    try:
        Xc, rs = _bind(eng, 1000, 300, 20, 2, seed=10)
        with pytest.raises(PlsxError, match='status -2.*scratch budget'):
            eng.simpls_coef_ci(eng._empty((2000, 20, 1000)), ci=95)                  # 0.32 GB of stack
        stack = rs.randn(50, 20, 1000)
        _check(_closing(eng, stack, 95), stack_ci(Xc, stack, 95), 'after the refusal', tol=NUMPY)
    finally:
        eng.close()
    eng = _engine()                                    # nothing bound: PLSX_ERR_STATE
    try:
        t = eng._zeros((64,))
        with pytest.raises(PlsxError, match='status -4'):
            eng._check(eng.lib.plsx_simpls_coef_ci(eng.ctx, t.data_ptr(), 4, 0, 0.0, 3, 0.0, t.data_ptr(), t.data_ptr(),
                                                   None))
    finally:
        eng.close()


def _c5_class(B=600, seed=4):
    rs = np.random.RandomState(seed)
    S, T, k = 1000, 20, 15
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    return X, Y, S, T, k, rs


def test_batch_geometry_2400_bootstraps_heavy_ties():
    """The geometry of test_batch_geometry_2400_bootstraps_and_small_scratch: 2400 bootstraps as 6 distinct samples
    replicated, so every series holds 6 distinct values 400 times each: the oracle's 6 coefficient matrices repeated by
    their counts.  n = 2400 is sorted whole; heavy ties are legitimate input to it."""
    import pypyls_amd as pls
    X, Y, S, T, k, rs = _c5_class()
    n, nd = 2400, 6
    distinct = rs.randint(0, S, size=(S, nd))
    which = np.arange(n) % nd
    which[[0, 1, n - 2, n - 1]] = [4, 2, 5, 0]
    boots = np.ascontiguousarray(distinct[:, which])
    counts = np.bincount(which, minlength=nd)
    for cc in (7, k):
        want = ci_of(coef_boot(X, Y, distinct, k, cc), ci=95, weights=counts)
        res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=n, bootsamples=boots, coef_components=cc,
                                 coef_ci=True, seed=1, verbose=False)
        _check(res.bootres.coefs_ci, want, 'S=1000 T=20 k=15 c={} n_boot=2400'.format(cc))
        ref_se = coef_expected(X, Y, distinct, k, cc, weights=counts)
        assert_close(res.bootres.coefs_stderr, ref_se['stderr'], rtol=RTOL, what='coefs_stderr next to the intervals')


def test_past_the_onchip_bound_s21000():
    import pypyls_amd as pls
    rs = np.random.RandomState(21)
    S, B, T, k, n = 21000, 200, 2, 2, 6
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    boots = rs.randint(0, S, size=(S, n))
    for cc in (1, 2):
        want = coef_ci_expected(X, Y, boots, k, cc)
        res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=n, bootsamples=boots, coef_components=cc,
                                 coef_ci=True, seed=1, verbose=False)
        _check(res.bootres.coefs_ci, want, 'S=21000 c={}'.format(cc))


def _flat(res):
    out = {}
    for key, val in res.items():
        if key == 'inputs':
            continue
        if isinstance(val, dict):
            for k2, v2 in val.items():
                out[key + '.' + k2] = v2
        else:
            out[key] = val
    return out


@pytest.mark.parametrize('quad', [-1, 1])
def test_nothing_else_moves_and_results_are_bit_reproducible(quad):
    """Every other array of a seeded call (coefs_stderr / coefs_normed and the drawn samples included) is
    np.array_equal with and without the keyword; two runs with it give the same bits in coefs_ci."""
    import pypyls_amd as pls
    rs = np.random.RandomState(8)
    X = rs.randn(90, 400)
    Y = rs.randn(90, 6) + 0.5 * X[:, :6]
    kw = dict(n_components=5, n_perm=20, n_boot=300, test_split=4, coef_components=3, seed=4321, verbose=False)
    runs = []
    for flag in (False, True, True):
        eng = _engine(quad=quad)
        try:
            runs.append(pls.pls_regression(X, Y, coef_ci=flag, _engine=eng, **kw))
        finally:
            eng.close()
    without, a, b = runs
    fw, fa = _flat(without), _flat(a)
    assert set(fa) - set(fw) == {'bootres.coefs_ci'}
    assert 'coef_ci' not in without.inputs and a.inputs.coef_ci is True
    for key, val in fw.items():
        va, vb = np.asarray(val), np.asarray(fa[key])
        assert np.array_equal(va, vb, equal_nan=va.dtype.kind == 'f'), key
    for key in ('bootres.coefs_stderr', 'bootres.coefs_normed', 'bootres.bootsamples', 'cvres.cvsamples'):
        assert key in fw, key
    assert a.bootres.coefs_ci.shape == (400, 6, 2)
    assert np.array_equal(a.bootres.coefs_ci, b.bootres.coefs_ci)
    # the intervals belong to the bootstraps the ratios come from: every interval is finite and ordered
    assert np.isfinite(a.bootres.coefs_ci).all() and np.all(a.bootres.coefs_ci[..., 0] <= a.bootres.coefs_ci[..., 1])


def test_team_of_two_contexts_agrees_with_one_device():
    """Each rank keeps its chunk-cyclic share; the stacks meet in the one collective and the lead rank closes the pass
    over all of them: the same series in another order, so agreement to rounding and beyond."""
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case('a')
    f = load_golden('simpls_coef_ci_a')
    kw = dict(kw, n_perm=6)
    one = pls.pls_regression(g['X'], g['Y'], coef_components=c, coef_ci=True, **kw)
    two = pls.pls_regression(g['X'], g['Y'], coef_components=c, coef_ci=True, device_ids=[0, 0], **kw)
    _same(one.bootres.coefs_ci, two.bootres.coefs_ci, ROUTES, 'one device vs team of two')
    _check(two.bootres.coefs_ci, f['ref_ci'][0], 'team of two vs reference')
