"""pls_regression(vip_components=c) on the device (plsx_simpls_vip_keep / plsx_simpls_vip_ci: k_sd_vip, k_vip_prod,
k_vip_moments + the selection kernels): the reference fixtures through the public call, the oracle on both solver routes
and both routes of the weights, the kept stack itself, the closing entry alone against numpy (tile edges, chunking, the
full sort), the limits, what must not move, batch geometry with heavy ties, a team.

Gates: RTOL = 1e-5 through conftest.assert_close against reference and oracle, 1e-9 between routes -- the bars of
tests/test_gpu_regression_coef_ci.py.  The closing entry alone is compared with numpy on the SAME stack at 1e-10: by
Cauchy-Schwarz the error of sqrt(sum_a w_a^2) is at most the norm of the errors of the c contractions, each an fp64 sum
of S <= 1000 products (rounding <= S 2^-53 sum |x g|), so about sqrt(c) S 2^-53 sum |x g| -- 1e-12 of the largest value
for these inputs; the standard deviation and an order statistic are continuous functions of their series.  Every figure
is printed before it is asserted; no element is left out of a comparison."""
import numpy as np
import pytest

from conftest import load_golden, assert_close
from oracle import cpu_ref as ref
from regression_coef_expect import coef_expected, max_rel, packed_bootsamples
from regression_coef_ci_expect import coef_ci_expected
from regression_vip_expect import _fits, stack_boot, stack_vip, summary, vip_boot, vip_expected, vip_of

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
    print('{}: max err / scale {:.3e}'.format(what, err))
    assert_close(got, want, rtol=tol, what=what)
    return err


def _check_all(res, want, what, tol=RTOL):
    B = len(want['vip'])
    assert res.vip.shape == (B,) and res.bootres.vip_stderr.shape == (B,) and res.bootres.vip_ci.shape == (B, 2)
    _check(res.vip, want['vip'], what + ': vip', tol)
    _check(res.bootres.vip_stderr, want['stderr'], what + ': vip_stderr', tol)
    _check(res.bootres.vip_ci, want['ci'], what + ': vip_ci', tol)
    assert np.all(res.bootres.vip_ci[:, 0] <= res.bootres.vip_ci[:, 1]), what + ': lower above upper'
    inv = abs(float((res.vip ** 2).sum()) - B) / B
    print('{}: sum vip^2 off B by {:.3e} relative'.format(what, inv))
    assert inv <= 1e-12


def _same(a, b, tol, what):
    err = max_rel(a, b)
    print('{}: max diff / scale {:.3e}'.format(what, err))
    assert err <= tol, (what, err)


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_fixtures_through_the_public_call(tag):
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case(tag)
    f = load_golden('simpls_vip_' + tag)
    for i, level in enumerate(f['ci']):
        res = pls.pls_regression(g['X'], g['Y'], vip_components=c, ci=float(level), **kw)
        _check_all(res, dict(vip=f['ref_vip'], stderr=f['ref_stderr'], ci=f['ref_ci'][i]),
                   'simpls_vip_{} ci={:g} vs reference'.format(tag, level))
        assert res.inputs.vip_components == c and 'coef_components' not in res.inputs
        assert np.array_equal(pls.vip(res), res.vip)


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_oracle_on_both_solver_routes_and_both_weight_routes(tag):
    """c < k and c = k; on-chip and global solver route; weights in place (quad_sums = -1) and through the quadratic
    form (quad_sums = 1): the kept stack, and so the series, are the same under all of them."""
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case(tag)
    for cc in sorted({1, c, k}):
        want = vip_expected(g['X'], g['Y'], g['bootsamples'], k, cc, aggfunc=aggfunc, third=third)
        runs = {}
        for glob in (False, True):
            for quad in (-1, 1):
                eng = _engine(glob, quad)
                try:
                    res = pls.pls_regression(g['X'], g['Y'], vip_components=cc, _engine=eng, **kw)
                finally:
                    eng.close()
                _check_all(res, want, '{} c={} {} quad_sums={} vs oracle'.format(tag, cc, 'global' if glob else 'on-chip',
                                                                                 quad))
                runs[(glob, quad)] = res.bootres
        for key, other in runs.items():
            _same(runs[(False, -1)].vip_ci, other.vip_ci, ROUTES, '{} c={} vip_ci on-chip/-1 vs {}'.format(tag, cc, key))
            _same(runs[(False, -1)].vip_stderr, other.vip_stderr, ROUTES,
                  '{} c={} vip_stderr on-chip/-1 vs {}'.format(tag, cc, key))


@pytest.mark.parametrize('glob', [False, True])
def test_kept_stack_reproduces_the_bootstrap_vip(glob):
    """plsx_simpls_vip_keep alone: the stack the batches leave, through numpy's closing pass (stack_boot), is every
    bootstrap's VIP of the oracle, and sums to B; two batches append; a coefficient series alongside changes no bit."""
    g, k, c, aggfunc, third, kw = _case('a')
    X, Y, boots = g['X'], g['Y'], g['bootsamples']
    S, B, T, n = X.shape[0], X.shape[1], Y.shape[1], boots.shape[1]
    Xc = X - X.mean(axis=0)
    stacks = {}
    for with_coef in (False, True):
        eng = _engine(glob)
        try:
            eng.set_data_regression(X, Y - Y.mean(axis=0), k)
            d_W, _, _ = eng.simpls_decompose_dev()
            eng.simpls_set_original_dev(d_W)
            if with_coef:
                eng.simpls_coef_begin(c)
            keep = eng._zeros((n, c, S))
            eng.simpls_vip_keep(keep)
            usum, usq, yl = eng._zeros((B, k)), eng._zeros((B, k)), eng._zeros((n, T, k))
            rows = np.ascontiguousarray(boots.T)
            eng.simpls_boot_into(eng.rows_tensor(rows[:15]), usum, usq, yl[:15])
            eng.simpls_boot_into(eng.rows_tensor(rows[15:]), usum, usq, yl[15:])
            if with_coef:
                eng.simpls_coef_finish(eng._zeros((B, T)), eng._zeros((B, T)))
            eng.sync()
            stacks[with_coef] = keep.cpu().numpy()
        finally:
            eng.close()
    got = stack_boot(Xc, stacks[False])
    _check(got, vip_boot(X, Y, boots, k, c), 'kept stack ({}) vs oracle vip_boot'.format('global' if glob else 'on-chip'))
    inv = float(np.max(np.abs((got ** 2).sum(axis=1) - B)) / B)
    print('kept stack: sum VIP^2 off B by {:.3e} relative'.format(inv))
    assert inv <= 1e-9
    assert np.array_equal(stacks[False], stacks[True])


def _bind(eng, S, B, T, k, seed):
    rs = np.random.RandomState(seed)
    X, Y = rs.randn(S, B), rs.randn(S, T)
    Xc = X - X.mean(axis=0)
    eng.set_data_regression(Xc, Y - Y.mean(axis=0), k)
    return Xc - Xc.mean(axis=0), rs                    # (the device centres what it is given once more)


def _closing(eng, stack, ci):
    sd, lo, hi = eng.simpls_vip_ci(stack if hasattr(stack, 'data_ptr') else eng._dev(stack, np.float64), ci=ci)
    eng.sync()
    return sd.cpu().numpy(), np.stack([lo.cpu().numpy(), hi.cpu().numpy()], -1)


def _check_closing(got, want, what):
    (sd, iv), (wsd, wiv) = got, want
    assert sd.shape == wsd.shape and iv.shape == wiv.shape
    err = _check(iv, wiv, what + ': interval', tol=NUMPY)
    assert err <= NUMPY and np.all(iv[:, 0] <= iv[:, 1])
    if np.isnan(wsd).all():
        assert np.isnan(sd).all(), what + ': one bootstrap has no spread'
    else:
        assert _check(sd, wsd, what + ': stderr', tol=NUMPY) <= NUMPY


@pytest.mark.parametrize('S,B,c,n', [(37, 150, 3, 70), (5, 17, 1, 1), (130, 129, 2, 2), (33, 257, 5, 3),
                                     (64, 128, 4, 65)])
def test_closing_entry_alone_against_numpy_across_tile_edges(S, B, c, n):
    """A random stack, no solver: B, n, S on and off the multiples of 128 / 64 / 32 / 4 the tiles are made of; one
    bootstrap (stderr NaN); odd S takes the unaligned loads of the stack; c > 4; B exactly one block with n one past a
    bootstrap tile."""
    eng = _engine()
    try:
        Xc, rs = _bind(eng, S, B, 2, 1, seed=S + B + n)
        stack = rs.randn(n, c, S)
        for ci in (95, 80):
            _check_closing(_closing(eng, stack, ci), stack_vip(Xc, stack, ci),
                           'closing S={} B={} c={} n={} ci={}'.format(S, B, c, n, ci))
    finally:
        eng.close()


def _normalised_stack(Xc, rs, n, c):
    """A stack as k_sd_vip leaves it: rows a_a sqrt(ssq_a / (|Xc^T a_a|^2 sum ssq)), so that sum_f VIP_b[f]^2 = B."""
    A = rs.randn(n, c, Xc.shape[0])
    wn = (np.einsum('sf,nas->naf', Xc, A, optimize=True) ** 2).sum(axis=-1)
    ssq = rs.rand(n, c) + 0.1
    return A * np.sqrt(ssq / (wn * ssq.sum(axis=1, keepdims=True)))[:, :, None]


def test_chunked_unchunked_and_sorted_give_the_same_bits_and_the_invariant():
    """S = 200, c = 3, n = 1000, B = 5000: 4.8 MB of stack, 40 MB of series.  A 0.02 GB scratch budget leaves room for
    2048 features per chunk (three chunks); percentile_sort = 1 takes the full sort.  Each entry is one block's work
    whatever the chunk and every reduction has one order: all three results have the same bits.  One bootstrap at a
    time the interval is the series itself: sum_f of its squares is B, for every bootstrap, chunked or not."""
    S, B, c, n = 200, 5000, 3, 1000
    want = stack = None
    got = {}
    for name, kw in (('default', {}), ('scratch 0.02 GB', dict(scratch_gb=0.02)), ('percentile_sort', dict(sort=True))):
        eng = _engine(**kw)
        try:
            Xc, rs = _bind(eng, S, B, 2, 2, seed=6)
            if want is None:
                stack = _normalised_stack(Xc, rs, n, c)
                stack[n // 2:n // 2 + 300] = stack[:300]           # (ties: 300 bootstraps twice in every series)
                want = stack_vip(Xc, stack, 95)
            d_stack = eng._dev(stack, np.float64)
            eng.set_timing(True)
            got[name] = _closing(eng, d_stack, 95)
            kt = eng.kernel_timing()
            print('{}: {}'.format(name, {key: kt[key] for key in ('k_coef_prod', 'k_percentile')}))
            launches = kt['k_coef_prod'][1]
            assert launches == (3 if name == 'scratch 0.02 GB' else 1), (name, launches)
            assert kt['k_percentile'][1] == launches
            eng.set_timing(False)
            if name != 'percentile_sort':
                series = np.stack([_closing(eng, d_stack[b:b + 1], 95)[1] for b in range(n)])      # (n, B, 2)
                assert np.array_equal(series[..., 0], series[..., 1])
                inv = float(np.max(np.abs((series[..., 0] ** 2).sum(axis=1) - B)) / B)
                print('{}: sum_f VIP_b[f]^2 off B by {:.3e} relative at worst over {} bootstraps'.format(name, inv, n))
                assert inv <= 1e-12
                got[name + ' series'] = series
        finally:
            eng.close()
        _check_closing(got[name], want, '{} vs numpy'.format(name))
    for name in ('scratch 0.02 GB', 'percentile_sort'):
        assert np.array_equal(got['default'][0], got[name][0]), name + ': stderr'
        assert np.array_equal(got['default'][1], got[name][1]), name + ': interval'
    assert np.array_equal(got['default series'], got['scratch 0.02 GB series'])


def test_limits_and_refusals_leave_the_context_usable():
    from pypyls_amd.engine import PlsxError
    S, B, T, c = 64, 128, 2, 2
    eng = _engine()
    try:
        Xc, rs = _bind(eng, S, B, T, 2, seed=9)
        stack = rs.randn(16385, c, S)
        d_stack = eng._dev(stack, np.float64)
        with pytest.raises(PlsxError, match='status -2.*16384'):
            eng.simpls_vip_ci(d_stack, ci=95)
        p = d_stack.data_ptr()
        with pytest.raises(PlsxError, match='status -1'):           # index outside 0 .. n - 1
            eng._check(eng.lib.plsx_simpls_vip_ci(eng.ctx, p, 10, c, 10, 0.0, 3, 0.0, p, p, p, None))
        with pytest.raises(PlsxError, match='status -1'):           # null stack
            eng._check(eng.lib.plsx_simpls_vip_ci(eng.ctx, None, 10, c, 1, 0.0, 3, 0.0, p, p, p, None))
        with pytest.raises(PlsxError, match='status -1'):           # c < 1
            eng._check(eng.lib.plsx_simpls_vip_ci(eng.ctx, p, 10, 0, 1, 0.0, 3, 0.0, p, p, p, None))
        # keeping needs the original fit; c within 1 .. k; a batch that would overflow the stack is refused before it
        # computes anything
        keep = eng._zeros((3, c, S))
        with pytest.raises(PlsxError, match='status -4'):
            eng.simpls_vip_keep(keep)
        d_W, _, _ = eng.simpls_decompose_dev()
        eng.simpls_set_original_dev(d_W)
        with pytest.raises(PlsxError, match='status -1.*n_components'):
            eng.simpls_vip_keep(eng._zeros((3, 3, S)))
        eng.simpls_vip_keep(keep)
        boots = rs.randint(0, S, size=(S, 5))
        usum, usq, yl = eng._zeros((B, 2)), eng._zeros((B, 2)), eng._zeros((5, T, 2))
        with pytest.raises(PlsxError, match='status -1.*kept VIP'):
            eng.simpls_boot_into(eng.rows_tensor(boots.T), usum, usq, yl)
        assert float(usum.abs().sum()) == 0.0 and float(keep.abs().sum()) == 0.0
        eng.simpls_boot_into(eng.rows_tensor(boots.T[:3]), usum, usq, yl[:3])
        eng.sync()
        kept = stack_boot(Xc, keep.cpu().numpy())
        assert np.isfinite(kept).all() and float(np.max(np.abs((kept ** 2).sum(axis=1) - B))) <= 1e-9 * B
        with pytest.raises(PlsxError, match='status -1.*kept VIP'):
            eng.simpls_boot_into(eng.rows_tensor(boots.T[:1]), usum, usq, yl[:1])      # the stack is full now
        eng.simpls_set_original_dev(d_W)               # ends the keeping: batches run again, the stack stays as it was
        before = keep.clone()
        eng.simpls_boot_into(eng.rows_tensor(boots.T[:1]), usum, usq, yl[:1])
        eng.sync()
        assert bool((keep == before).all())
        # after all the refusals: the largest series the kernels take, B exactly one block
        _check_closing(_closing(eng, d_stack[:16384], 95), stack_vip(Xc, stack[:16384], 95), 'n = 16384, B = 128')
    finally:
        eng.close()
    # a stack that cannot fit the scratch budget: refused the same way, asked through a small budget
    eng = _engine(scratch_gb=0.25)
    try:
        Xc, rs = _bind(eng, 1000, 300, 20, 2, seed=10)
        with pytest.raises(PlsxError, match='status -2.*scratch budget'):
            eng.simpls_vip_ci(eng._empty((2000, 20, 1000)), ci=95)                   # 0.32 GB of stack
        stack = rs.randn(50, 4, 1000)
        _check_closing(_closing(eng, stack, 95), stack_vip(Xc, stack, 95), 'after the refusal')
    finally:
        eng.close()
    eng = _engine()                                    # nothing bound: PLSX_ERR_STATE
    try:
        t = eng._zeros((64,))
        p = t.data_ptr()
        with pytest.raises(PlsxError, match='status -4'):
            eng._check(eng.lib.plsx_simpls_vip_ci(eng.ctx, p, 4, 1, 0, 0.0, 3, 0.0, p, p, p, None))
        with pytest.raises(PlsxError, match='status -4'):
            eng._check(eng.lib.plsx_simpls_vip_keep(eng.ctx, 1, p, 4))
    finally:
        eng.close()


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
    """Every other array of a seeded call (the drawn samples included) is np.array_equal with and without the keyword,
    alone and next to coef_components / coef_ci -- whose arrays do not move either, nor do they move the VIP's; two runs
    give the same bits."""
    import pypyls_amd as pls
    rs = np.random.RandomState(8)
    X = rs.randn(90, 400)
    Y = rs.randn(90, 6) + 0.5 * X[:, :6]
    kw = dict(n_components=5, n_perm=10, n_boot=200, test_split=2, seed=4321, verbose=False)
    coef = dict(coef_components=3, coef_ci=True)
    runs = []
    for extra in ({}, dict(vip_components=4), coef, dict(coef, vip_components=4), dict(coef, vip_components=4)):
        eng = _engine(quad=quad)
        try:
            runs.append(pls.pls_regression(X, Y, _engine=eng, **dict(kw, **extra)))
        finally:
            eng.close()
    plain, vip_only, coef_only, both, again = runs
    new = {'vip', 'bootres.vip_stderr', 'bootres.vip_ci'}
    for without, with_ in ((plain, vip_only), (coef_only, both)):
        fw, fa = _flat(without), _flat(with_)
        assert set(fa) - set(fw) == new
        assert 'vip_components' not in without.inputs and with_.inputs.vip_components == 4
        for key, val in fw.items():
            va, vb = np.asarray(val), np.asarray(fa[key])
            assert np.array_equal(va, vb, equal_nan=va.dtype.kind == 'f'), key
    for key in ('bootres.coefs_stderr', 'bootres.coefs_ci', 'bootres.bootsamples', 'cvres.cvsamples'):
        assert key in _flat(coef_only), key
    for key in new:
        assert np.array_equal(_flat(vip_only)[key], _flat(both)[key]), key      # a coefficient series moves no bit of it
        assert np.array_equal(_flat(both)[key], _flat(again)[key]), key
    assert both.bootres.vip_ci.shape == (400, 2) and np.isfinite(both.bootres.vip_ci).all()
    assert np.all(both.bootres.vip_ci[:, 0] <= both.bootres.vip_ci[:, 1]) and np.all(both.bootres.vip_stderr > 0)


def test_batch_geometry_2400_bootstraps_heavy_ties():
    """The geometry of the coefficient intervals' test of that name: S = 1000, T = 20, k = 15, 2400 bootstraps as 6
    distinct samples replicated, through one solver batch: every series holds 6 distinct values 400 times each, the
    oracle's 6 VIP maps repeated by their counts."""
    import pypyls_amd as pls
    rs = np.random.RandomState(4)
    S, T, k, B = 1000, 20, 15, 600
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    n, nd = 2400, 6
    distinct = rs.randint(0, S, size=(S, nd))
    which = np.arange(n) % nd
    which[[0, 1, n - 2, n - 1]] = [4, 2, 5, 0]
    boots = np.ascontiguousarray(distinct[:, which])
    counts = np.bincount(which, minlength=nd)
    fits = list(_fits(X, Y, distinct, k, 'mean', None, ref.simpls, ref.get_mask))          # fitted once, for both c
    for cc in (7, k):
        sd, iv = summary(np.stack([vip_of(f, cc) for f in fits[1:]]), ci=95, weights=counts)
        res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=n, bootsamples=boots, vip_components=cc,
                                 seed=1, verbose=False)
        _check_all(res, dict(vip=vip_of(fits[0], cc), stderr=sd, ci=iv), 'S=1000 T=20 k=15 c={} n_boot=2400'.format(cc))


def test_team_of_two_contexts_agrees_with_one_device():
    """Each rank keeps its chunk-cyclic share; the stacks meet in the one collective and the lead rank closes the pass
    over all of them: the same series in another order -- the same order statistics, the standard deviation to
    rounding."""
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case('a')
    f = load_golden('simpls_vip_a')
    kw = dict(kw, n_perm=6)
    one = pls.pls_regression(g['X'], g['Y'], vip_components=c, **kw)
    two = pls.pls_regression(g['X'], g['Y'], vip_components=c, device_ids=[0, 0], **kw)
    assert np.array_equal(one.bootres.vip_ci, two.bootres.vip_ci)
    assert np.array_equal(one.vip, two.vip)
    _same(one.bootres.vip_stderr, two.bootres.vip_stderr, ROUTES, 'vip_stderr: one device vs team of two')
    _check_all(two, dict(vip=f['ref_vip'], stderr=f['ref_stderr'], ci=f['ref_ci'][0]), 'team of two vs reference')
