"""pls_regression(coef_components=c) on the device (plsx_simpls_coef_begin / _finish, k_sd_coef): the reference
fixtures through the public call, the oracle on both solver routes and both routes of the weights, batch geometry, a
cohort past the on-chip bound, the refusal, what must not move, reproducibility and a team.

Gate: RTOL = 1e-5 through conftest.assert_close, the project's parity bar for regression.  Every figure is printed
before it is asserted.  The inputs keep the oracle's own |coefs_normed| below 1e3 and every coefs_stderr above 1e-8 of
the largest (asserted in regression_coef_expect.coef_expected); no element is left out of a comparison."""
import numpy as np
import pytest

from conftest import load_golden, assert_close
from regression_coef_expect import coef_expected, max_rel, packed_bootsamples

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ROUTES = 1e-9
NEW = ('coefs', 'intercept', 'coefs_stderr', 'coefs_normed')


def _engine(glob=False, quad=0, **kw):
    from pypyls_amd.engine import Engine
    opts = {}
    if glob:
        opts['simpls_global'] = 1
    if quad:
        opts['quad_sums'] = quad
    return Engine(options=opts, **kw)


def _new(res):
    return dict(coefs=res['coefs'], intercept=res['intercept'], coefs_stderr=res.bootres['coefs_stderr'],
                coefs_normed=res.bootres['coefs_normed'])


def _check(res, want, what, tol=RTOL):
    got = _new(res)
    pairs = dict(coefs=want['coefs'], intercept=want['intercept'], coefs_stderr=want['stderr'],
                 coefs_normed=want['normed'])
    errs = {key: max_rel(got[key], pairs[key]) for key in NEW}
    print('{}: max err / scale  '.format(what) + '  '.join('{} {:.3e}'.format(k_, errs[k_]) for k_ in NEW))
    for key in NEW:
        assert_close(got[key], pairs[key], rtol=tol, what='{} {}'.format(what, key))
    return errs


def _same(a, b, tol, what):
    a, b = _new(a), _new(b)
    errs = {key: max_rel(a[key], b[key]) for key in NEW}
    print('{}: max diff / scale  '.format(what) + '  '.join('{} {:.3e}'.format(k_, errs[k_]) for k_ in NEW))
    assert max(errs.values()) <= tol, (what, errs)


def _case(tag):
    g = load_golden('simpls_coef_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    third = g.get('third')
    bs = g['bootsamples'] if third is None else packed_bootsamples(g['bootsamples'], third)
    kw = dict(n_components=k, n_perm=0, n_boot=g['bootsamples'].shape[1], bootsamples=bs, aggfunc=aggfunc, seed=1,
              verbose=False)
    return g, k, c, aggfunc, third, kw


def _reference_values(g, c):
    """What the fixture pins: beta of the reference on the original data, its sums over the bootstraps; boot_rel with
    the original added back."""
    from oracle import cpu_ref as ref
    n = g['bootsamples'].shape[1]
    normed, se = ref.boot_rel(g['ref_coefs'], g['ref_bsum'] + g['ref_coefs'], g['ref_bsq'] + g['ref_coefs'] ** 2, n + 1)
    return dict(coefs=g['ref_coefs'], intercept=g['ref_intercept'], stderr=se, normed=normed)


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_fixtures_through_the_public_call(tag):
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case(tag)
    res = pls.pls_regression(g['X'], g['Y'], coef_components=c, **kw)
    _check(res, _reference_values(g, c), 'simpls_coef_{} vs reference'.format(tag))
    assert res.coefs.shape == (g['X'].shape[1], g['Y'].shape[1]) and res.intercept.shape == (g['Y'].shape[1],)
    assert res.inputs.coef_components == c
    # predict from the device result: [1, x] @ beta of the reference
    X_new = np.random.RandomState(3).randn(5, g['X'].shape[1])
    assert_close(pls.predict(res, X_new), g['ref_intercept'] + X_new @ g['ref_coefs'], rtol=RTOL, what='predict')


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_oracle_on_both_solver_routes_and_both_weight_routes(tag):
    """c < k and c = k; on-chip and global solver route; weights in place (quad_sums = -1) and through the quadratic
    form (quad_sums = 1): the coefficient series gives the same result under all of them."""
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case(tag)
    for cc in sorted({c, k} | ({2} if k > 2 else set())):
        want = coef_expected(g['X'], g['Y'], g['bootsamples'], k, cc, aggfunc=aggfunc, third=third)
        runs = {}
        for glob in (False, True):
            for quad in (-1, 1):
                eng = _engine(glob, quad)
                try:
                    res = pls.pls_regression(g['X'], g['Y'], coef_components=cc, _engine=eng, **kw)
                finally:
                    eng.close()
                name = '{} c={} {} quad_sums={}'.format(tag, cc, 'global' if glob else 'on-chip', quad)
                _check(res, want, name + ' vs oracle')
                runs[(glob, quad)] = res
        base = runs[(False, -1)]
        for key, other in runs.items():
            _same(base, other, ROUTES, '{} c={} on-chip/-1 vs {}'.format(tag, cc, key))
        # the weights themselves agree across their two routes as they always did
        assert_close(runs[(False, 1)].bootres.x_weights_normed, base.bootres.x_weights_normed, rtol=1e-7,
                     what='x_weights_normed across quad_sums')


def _c5_class(B=600, seed=4):
    rs = np.random.RandomState(seed)
    S, T, k = 1000, 20, 15
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    return X, Y, S, T, k, rs


def test_batch_geometry_2400_bootstraps_and_small_scratch():
    """S 1000, T 20, k 15 (c5's solver shape class, B reduced): 2400 bootstraps -- more than the 2304 of one
    three-waves-per-SIMD batch, and more than the front-end's first chunk, so the series crosses solver batches -- as 6
    distinct samples replicated; the oracle's sums are weighted by the replication counts.  A 2 GB scratch budget
    then forces solver batches of a few hundred."""
    import pypyls_amd as pls
    X, Y, S, T, k, rs = _c5_class()
    n, nd = 2400, 6
    distinct = rs.randint(0, S, size=(S, nd))
    which = np.arange(n) % nd
    which[[0, 1, n - 2, n - 1]] = [4, 2, 5, 0]
    boots = np.ascontiguousarray(distinct[:, which])
    counts = np.bincount(which, minlength=nd)
    for cc in (7, k):
        want = coef_expected(X, Y, distinct, k, cc, weights=counts)
        assert want['n'] == n
        kw = dict(n_components=k, n_perm=0, n_boot=n, bootsamples=boots, coef_components=cc, seed=1, verbose=False)
        res = pls.pls_regression(X, Y, **kw)
        _check(res, want, 'S=1000 T=20 k=15 c={} n_boot=2400'.format(cc))
        if cc == k:
            eng = _engine(scratch_gb=2.0)
            try:
                small = pls.pls_regression(X, Y, _engine=eng, **kw)
            finally:
                eng.close()
            _check(small, want, 'S=1000 T=20 k=15 c={} scratch 2 GB'.format(cc))
            _same(res, small, ROUTES, 'default scratch vs 2 GB')


def test_past_the_onchip_bound_s21000():
    """S = 21 000 (the on-chip slice holds S <= 20 200 at this T, k), small B and T: 8 T S^2 = 7 GB."""
    import pypyls_amd as pls
    rs = np.random.RandomState(21)
    S, B, T, k, n = 21000, 200, 2, 2, 6
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    boots = rs.randint(0, S, size=(S, n))
    for cc in (1, 2):
        want = coef_expected(X, Y, boots, k, cc)
        res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=n, bootsamples=boots, coef_components=cc,
                                 seed=1, verbose=False)
        _check(res, want, 'S=21000 c={}'.format(cc))


def test_refusal_leaves_the_context_usable():
    """A series whose T S^2 accumulator does not fit the memory budget is refused with PLSX_ERR_UNSUPPORTED (-2); the
    context goes on working without it.  Asked through a tiny scratch budget, not by exhausting the device."""
    import pypyls_amd as pls
    from pypyls_amd.engine import PlsxError
    g, k, c, aggfunc, third, kw = _case('a')
    X, Y, S, T, k5, rs = _c5_class(B=300)
    kw5 = dict(n_components=k5, n_perm=0, n_boot=24, seed=2, verbose=False)
    eng = _engine(scratch_gb=0.25)                       # the accumulators of S = 1000, T = 20 need 0.16 + 0.33 GB
    try:
        with pytest.raises(PlsxError, match='status -2.*coefficient series'):
            pls.pls_regression(X, Y, coef_components=3, _engine=eng, **kw5)
        plain = pls.pls_regression(X, Y, _engine=eng, **kw5)
        # a series cannot be opened before plsx_simpls_set_original
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k5)
        with pytest.raises(PlsxError, match='status -4'):
            eng.simpls_coef_begin(1)
    finally:
        eng.close()
    ref_run = pls.pls_regression(X, Y, **kw5)
    assert np.array_equal(plain.bootres.bootsamples, ref_run.bootres.bootsamples)
    assert_close(plain.bootres.x_weights_normed, ref_run.bootres.x_weights_normed, rtol=1e-7, what='after the refusal')
    eng = _engine()
    try:
        eng.set_data_regression(g['X'] - g['X'].mean(axis=0), g['Y'] - g['Y'].mean(axis=0), k)
        d_W, _, _ = eng.simpls_decompose_dev()
        eng.simpls_set_original_dev(d_W)
        for bad in (0, k + 1):
            with pytest.raises(PlsxError, match='status -1'):
                eng.simpls_coef_begin(bad)
        with pytest.raises(PlsxError, match='status -4'):
            eng.simpls_coef_finish(eng._zeros((g['X'].shape[1], g['Y'].shape[1])),
                                   eng._zeros((g['X'].shape[1], g['Y'].shape[1])))
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
    """Every other array of a seeded call (drawn permsamples / bootsamples / cvsamples included) is np.array_equal
    with and without the keyword; two runs with it give the same bits in the four new arrays."""
    import pypyls_amd as pls
    rs = np.random.RandomState(8)
    X = rs.randn(90, 400)
    Y = rs.randn(90, 6) + 0.5 * X[:, :6]
    kw = dict(n_components=5, n_perm=20, n_boot=300, test_split=4, seed=4321, verbose=False)
    runs = []
    for cc in (None, 3, 3):
        eng = _engine(quad=quad)
        try:
            runs.append(pls.pls_regression(X, Y, coef_components=cc, _engine=eng, **kw))
        finally:
            eng.close()
    without, a, b = runs
    fw, fa = _flat(without), _flat(a)
    assert set(fa) - set(fw) == {'coefs', 'intercept', 'bootres.coefs_stderr', 'bootres.coefs_normed'}
    assert 'coef_components' not in without.inputs and a.inputs.coef_components == 3
    for key, val in fw.items():
        va, vb = np.asarray(val), np.asarray(fa[key])
        assert np.array_equal(va, vb, equal_nan=va.dtype.kind == 'f'), key
    for key in ('permres.permsamples', 'bootres.bootsamples', 'cvres.cvsamples'):
        assert key in fw, key
    for key in NEW:
        assert np.array_equal(_new(a)[key], _new(b)[key]), key


def test_team_of_two_contexts_agrees_with_one_device():
    """Each rank closes its own series; the partial sums are added in rank order in the one collective: agreement to
    rounding (1e-9), not bit for bit."""
    import pypyls_amd as pls
    g, k, c, aggfunc, third, kw = _case('a')
    kw = dict(kw, n_perm=6)
    one = pls.pls_regression(g['X'], g['Y'], coef_components=c, **kw)
    two = pls.pls_regression(g['X'], g['Y'], coef_components=c, device_ids=[0, 0], **kw)
    _same(one, two, ROUTES, 'one device vs team of two')
    assert np.array_equal(one.coefs, two.coefs) and np.array_equal(one.intercept, two.intercept)
    _check(two, _reference_values(g, c), 'team of two vs reference')
