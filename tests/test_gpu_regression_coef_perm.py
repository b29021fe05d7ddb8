"""pls_regression(coef_components=c, coef_perm=True) on the device (plsx_simpls_coef_perm_test / _begin / _end:
k_coef_perm_prod, k_coef_perm_max, k_col_sd, k_sd_coef along the permutation batches): the stateless entry against
numpy across the tile edges, the series along plsx_simpls_perm_batch, the reference fixtures through the public call
(one device and a team of two), the global solver route.

Gates: RTOL = 1e-5 through conftest.assert_close against the reference fixtures -- the bar
tests/test_gpu_regression_coef.py holds ``coefs`` to.  The stateless entry is compared with numpy on the SAME stack:
both sides are fp64 sums of S <= 64 products, and a maximum is a continuous function of its arguments, so the maxima
are held to the 1e-10 of the stack test of tests/test_gpu_regression_coef_ci.py.  Counts are integers and are compared
for EXACT equality everywhere: the fixtures keep every |b_p| at least 1e-8 |b| away from |b| (their generator refuses
anything closer), and for the random stacks a tie within the 1e-12 of the two sides' rounding has probability 1e-8 or
so over all entries.  Every figure is printed before it is asserted; no entry is left out of a comparison."""
import numpy as np
import pytest

from conftest import load_golden, assert_close
from regression_coef_expect import max_rel
from regression_coef_perm_expect import stack_test

pytestmark = pytest.mark.gpu
RTOL = 1e-5
NUMPY = 1e-10
KEYS = ('coefs_pvals', 'coefs_max', 'coefs_pvals_fwe')


def _engine(glob=False, **kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1} if glob else {}, **kw)


def _bind(eng, S, B, T, k, seed):
    rs = np.random.RandomState(seed)
    X, Y = rs.randn(S, B), rs.randn(S, T)
    Xc = X - X.mean(axis=0)
    eng.set_data_regression(Xc, Y - Y.mean(axis=0), k)
    return Xc - Xc.mean(axis=0), rs                    # (the device centres what it is given once more)


def _stateless(eng, stack, obs, standardise, count=None):
    import torch
    B, T = obs.shape
    if count is None:
        count = torch.zeros((B, T), dtype=torch.int32, device=eng.device)
    dmax = eng._zeros((stack.shape[0], T))
    eng.simpls_coef_perm_test(eng._dev(stack, np.float64), eng._dev(obs, np.float64), count, dmax, standardise=standardise)
    eng.sync()
    return count, dmax.cpu().numpy()


@pytest.mark.parametrize('n', [70, 1])
@pytest.mark.parametrize('B', [150, 300])
@pytest.mark.parametrize('S', [37, 64])
def test_stateless_entry_against_numpy_across_tile_edges(S, B, n):
    """S = 37: the unaligned pair loads of the stack and a partial last stage; B = 150 / 300: a partial last feature
    block, three blocks; n = 70: a partial second permutation tile.  One stack entry is planted so that the maximum of
    (permutation n - 1, behaviour 1) sits in the last, partial feature block.  A second call on the same counts doubles
    them."""
    T = 3
    eng = _engine()
    try:
        Xc, rs = _bind(eng, S, B, T, 1, seed=S + B + n)
        stack, obs = rs.randn(n, T, S), rs.randn(B, T) * np.sqrt(S)
        stack[n - 1, 1] = 50.0 * Xc[:, B - 1] / np.linalg.norm(Xc[:, B - 1])
        for std in (0, 1):
            want_count, want_max = stack_test(Xc, stack, obs, std)
            count, got_max = _stateless(eng, stack, obs, std)
            got_count = count.cpu().numpy()
            err = max_rel(got_max, want_max)
            print('S={} B={} n={} standardise={}: maxima err / scale {:.3e}, counts {} .. {}, differing counts {}'.format(
                S, B, n, std, err, got_count.min(), got_count.max(), int((got_count != want_count).sum())))
            assert got_max.shape == (n, T) and got_count.shape == (B, T)
            assert err <= NUMPY
            assert_close(got_max, want_max, rtol=NUMPY, what='maxima')
            assert np.array_equal(got_count, want_count)
            coef = np.einsum('sf,s->f', Xc, stack[n - 1, 1]) * (Xc.std(axis=0, ddof=1) if std else 1.0)
            assert np.argmax(np.abs(coef)) == B - 1 and abs(got_max[n - 1, 1] - abs(coef[B - 1])) <= NUMPY * abs(coef[B - 1])
            count2, again = _stateless(eng, stack, obs, std, count=count)
            assert np.array_equal(count2.cpu().numpy(), 2 * want_count) and np.array_equal(again, got_max)
    finally:
        eng.close()


def test_stateless_entry_gives_the_same_bits_when_the_features_go_in_chunks():
    """S = 64, B = 300, T = 3, n = 12 000: 18.43 MB of stack, 288 KB of partial maxima per feature block.  A scratch
    budget of the stack plus 500 KB leaves room for one block per chunk (three chunks instead of one)."""
    S, B, T, n = 64, 300, 3, 12000
    stack_bytes = 8 * n * T * S
    got = {}
    want = None
    for name, kw in (('default', {}), ('three chunks', dict(scratch_gb=(stack_bytes + 500e3) / 2 ** 30))):
        eng = _engine(**kw)
        try:
            Xc, rs = _bind(eng, S, B, T, 1, seed=11)
            stack, obs = rs.randn(n, T, S), rs.randn(B, T) * np.sqrt(S)
            if want is None:
                want = stack_test(Xc, stack, obs, 1)
            eng.set_timing(True)
            count, dmax = _stateless(eng, stack, obs, 1)
            launches = eng.kernel_timing()['k_coef_prod'][1]
            print('{}: {} timed brackets of the feature pass'.format(name, launches))
            assert launches == (1 if name == 'default' else 3) + 1, (name, launches)       # (+ 1: k_col_sd)
            got[name] = (count.cpu().numpy(), dmax)
        finally:
            eng.close()
        err = max_rel(got[name][1], want[1])
        print('{}: maxima err / scale {:.3e}'.format(name, err))
        assert err <= NUMPY and np.array_equal(got[name][0], want[0])
    assert np.array_equal(got['default'][0], got['three chunks'][0])
    assert np.array_equal(got['default'][1], got['three chunks'][1])


@pytest.mark.parametrize('S', [37, 64])
def test_the_three_feature_passes_share_one_contraction_bit_for_bit(S):
    """k_coef_prod, k_coef_perm_prod and k_vip_prod contract the same tile through the same pieces (plsx_k_coefci.h), so
    a product is the same bits whichever of them forms it and wherever its resample sits in a tile.  S = 37: unaligned
    pair loads, the odd tail, a partial stage; S = 64: the aligned path, two full stages; B = 150: a partial second
    feature block; n = 70: a partial second resample tile.  P[b] (B, T) comes from plsx_simpls_coef_ci on the
    one-resample stack stack[b:b+1] (a series of one value: lo = hi = the product).  The permutation pass over the whole
    stack must then give max_f |P[b][f, t]| and sum_b (|P[b]| >= |obs|) exactly, and plsx_simpls_vip_ci on the
    one-component, one-resample stack stack[b:b+1, t:t+1] must give sqrt(B . P[b][:, t]^2) bit-equal to numpy's.
    That is what the three separate kernels gave before they shared their code (0 ulp at every b tried, both S), and
    what the number formats promise: the device's fp64 multiply and sqrt are correctly rounded (0 + p p, fused or not,
    is the rounded product), and numpy rounds in the same order -- p p first, then the product with B, then the root.
    The largest distance in ulp is printed before it is asserted to be zero."""
    import torch
    B, T, n, t_vip = 150, 3, 70, 1
    eng = _engine()
    try:
        _, rs = _bind(eng, S, B, T, 1, seed=S)
        stack, obs = rs.randn(n, T, S), rs.randn(B, T) * np.sqrt(S)
        d_stack = eng._dev(stack, np.float64)
        P = np.empty((n, B, T))
        for b in range(n):
            lo, hi = eng.simpls_coef_ci(d_stack[b:b + 1])
            assert torch.equal(lo, hi)
            P[b] = lo.cpu().numpy()
        assert np.all(np.isfinite(P)) and np.abs(P).min() > 0.0
        count, dmax = _stateless(eng, stack, obs, 0)
        want_count = (np.abs(P) >= np.abs(obs)[None]).sum(axis=0)
        differing = int((dmax != np.abs(P).max(axis=1)).sum())
        print('S={}: maxima differing in any bit {} of {}, counts differing {}'.format(
            S, differing, dmax.size, int((count.cpu().numpy() != want_count).sum())))
        assert np.array_equal(dmax, np.abs(P).max(axis=1))
        assert np.array_equal(count.cpu().numpy(), want_count)
        for b in (0, 63, 64, n - 1):
            sd, lo, hi = eng.simpls_vip_ci(d_stack[b:b + 1, t_vip:t_vip + 1].contiguous())
            want = np.sqrt(B * (P[b][:, t_vip] * P[b][:, t_vip]))
            got = lo.cpu().numpy()
            ulp = np.max(np.abs(got - want) / np.spacing(want))
            print('S={} b={}: VIP differs from numpy by at most {} ulp'.format(S, b, ulp))
            assert torch.equal(lo, hi)
            assert np.array_equal(got, want)
    finally:
        eng.close()


def _series_setup(eng, S, B, T, k, c, seed, n):
    import torch
    Xc, rs = _bind(eng, S, B, T, k, seed)
    d_W, _, _ = eng.simpls_decompose_dev()
    eng.simpls_set_original_dev(d_W)
    eng.sync()
    obs = rs.randn(B, T) * 0.05
    perms = np.stack([rs.permutation(S) for _ in range(n)], axis=1).astype(np.int32)
    return Xc, eng._dev(obs, np.float64), eng.rows_tensor(perms.T), torch


def _run_series(eng, c, d_obs, idx, pieces, torch, open_series=True):
    n, B, T = idx.shape[0], d_obs.shape[0], d_obs.shape[1]
    out = eng._zeros((n, eng.k))
    count = torch.zeros((B, T), dtype=torch.int32, device=eng.device)
    dmax = eng._zeros((n, T))
    if open_series:
        eng.simpls_coef_perm_begin(c, d_obs, count, dmax)
    for a, b in pieces:
        eng.simpls_perm_into(idx[a:b], out[a:b])
    if open_series:
        eng.simpls_coef_perm_end()
    eng.sync()
    return out.cpu().numpy(), count.cpu().numpy(), dmax.cpu().numpy()


def test_series_along_the_permutation_batches():
    """S = 1000, B = 300, T = 3, k = 4, c = 2, 70 permutations.  pctvar has the same bits with the series open; counts
    and maxima are the sum / concatenation of two half-size calls, also under a 0.02 GB scratch budget -- half of it
    takes 37 permutations of 264 392 bytes of solver state plus 24 048 of A_p and y-loadings, so the solver batches are
    37 + 33 --; a batch that would pass the capacity is refused with nothing computed."""
    from pypyls_amd.engine import PlsxError
    S, B, T, k, c, n = 1000, 300, 3, 4, 2, 70
    runs = {}
    for name, kw in (('default', {}), ('0.02 GB', dict(scratch_gb=0.02))):
        eng = _engine(**kw)
        try:
            Xc, d_obs, idx, torch = _series_setup(eng, S, B, T, k, c, 17, n)
            plain = _run_series(eng, c, d_obs, idx, [(0, n)], torch, open_series=False)
            eng.set_timing(True)
            whole = _run_series(eng, c, d_obs, idx, [(0, n)], torch)
            batches = eng.kernel_timing()['k_sd_coef'][1]
            eng.set_timing(False)
            halves = _run_series(eng, c, d_obs, idx, [(0, 35), (35, n)], torch)
            print('scratch {}: {} solver batches; counts {} .. {}'.format(name, batches, whole[1].min(), whole[1].max()))
            assert batches == (1 if name == 'default' else 2)
            assert np.array_equal(plain[0], whole[0]), 'pctvar moved with the series open'
            assert not plain[1].any() and not plain[2].any()
            for i, what in enumerate(('pctvar', 'counts', 'maxima')):
                assert np.array_equal(whole[i], halves[i]), (name, what)
            assert 0 < whole[1].min() + whole[1].max() and np.isfinite(whole[2]).all() and (whole[2] > 0).all()
            runs[name] = whole
            # capacity: a series of 35 takes 35, then refuses one more before it computes anything
            out = eng._zeros((n, eng.k))
            count = torch.zeros((B, T), dtype=torch.int32, device=eng.device)
            dmax = eng._zeros((35, T))
            eng.simpls_coef_perm_begin(c, d_obs, count, dmax)
            eng.simpls_perm_into(idx[:35], out[:35])
            eng.sync()
            before = count.clone()
            with pytest.raises(PlsxError, match='status -1.*coefficient series'):
                eng.simpls_perm_into(idx[35:36], out[35:36])
            eng.sync()
            assert float(out[35:].abs().sum()) == 0.0 and torch.equal(before, count)
            assert np.array_equal(dmax.cpu().numpy(), whole[2][:35])
            eng.simpls_coef_perm_end()
            with pytest.raises(PlsxError, match='status -1'):
                eng.simpls_coef_perm_begin(k + 1, d_obs, count, dmax)
        finally:
            eng.close()
    for i, what in enumerate(('pctvar', 'counts', 'maxima')):
        assert np.array_equal(runs['default'][i], runs['0.02 GB'][i]), what


def test_series_needs_the_original_fit_and_regression_data():
    import torch
    from pypyls_amd.engine import PlsxError
    eng = _engine()
    try:
        Xc, rs = _bind(eng, 40, 60, 2, 2, seed=3)
        obs, count, dmax = eng._zeros((60, 2)), torch.zeros((60, 2), dtype=torch.int32, device=eng.device), eng._zeros((4, 2))
        with pytest.raises(PlsxError, match='status -4'):
            eng.simpls_coef_perm_begin(1, obs, count, dmax)
        with pytest.raises(PlsxError, match='status -1'):
            eng._check(eng.lib.plsx_simpls_coef_perm_test(eng.ctx, None, 4, obs.data_ptr(), 1, count.data_ptr(),
                                                          dmax.data_ptr(), None))
        with pytest.raises(PlsxError, match='status -1'):
            eng._check(eng.lib.plsx_simpls_coef_perm_test(eng.ctx, obs.data_ptr(), 0, obs.data_ptr(), 1, count.data_ptr(),
                                                          dmax.data_ptr(), None))
    finally:
        eng.close()


def _case(tag):
    g, f = load_golden('simpls_coef_' + tag), load_golden('simpls_coef_perm_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    kw = dict(n_components=k, n_perm=f['permsamples'].shape[1], permsamples=f['permsamples'], n_boot=0, aggfunc=aggfunc,
              coef_components=c, seed=1, verbose=False)
    return g, f, kw


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


def _others_keep_their_bits(without, with_):
    fw, fa = _flat(without), _flat(with_)
    assert set(fa) - set(fw) == {'permres.' + key for key in KEYS}
    for key, val in fw.items():
        va, vb = np.asarray(val), np.asarray(fa[key])
        if va.dtype == object:
            continue
        assert np.array_equal(va, vb, equal_nan=va.dtype.kind == 'f'), key


@pytest.mark.parametrize('tag', ['a', 'nan', 'y3d'])
def test_fixtures_through_the_public_call_one_device_and_a_team_of_two(tag):
    import pypyls_amd as pls
    g, f, kw = _case(tag)
    B, T, n = g['X'].shape[1], g['Y'].shape[1], f['permsamples'].shape[1]
    without = pls.pls_regression(g['X'], g['Y'], **kw)
    res = pls.pls_regression(g['X'], g['Y'], coef_perm=True, **kw)
    pr = res.permres
    assert pr.coefs_pvals.shape == (B, T) and pr.coefs_max.shape == (T, n) and pr.coefs_pvals_fwe.shape == (B, T)
    err = max_rel(pr.coefs_max, f['ref_max'])
    count = np.rint(pr.coefs_pvals * (n + 1) - 1).astype(int)
    print('simpls_coef_perm_{}: coefs_max err / scale {:.3e}; differing counts {}; differing maxT p-values {}'.format(
        tag, err, int((count != f['ref_count']).sum()), int((pr.coefs_pvals_fwe != f['ref_pvals_fwe']).sum())))
    assert_close(pr.coefs_max, f['ref_max'], rtol=RTOL, what='coefs_max vs reference')
    assert np.array_equal(count, f['ref_count'])
    assert np.array_equal(pr.coefs_pvals, f['ref_pvals'])
    assert np.array_equal(pr.coefs_pvals_fwe, f['ref_pvals_fwe'])
    assert res.inputs.coef_perm is True and 'coef_perm' not in without.inputs
    _others_keep_their_bits(without, res)
    two = pls.pls_regression(g['X'], g['Y'], coef_perm=True, device_ids=[0, 0], **kw)
    for key in KEYS:
        assert np.array_equal(two.permres[key], pr[key]), 'team of two: ' + key


def test_next_to_every_other_option_nothing_else_moves():
    """coef_ci, vip_components, test_split and cv_perm in the same seeded call, drawn permutations: every other array is
    np.array_equal with and without the keyword, and two runs with it give the same bits."""
    import pypyls_amd as pls
    rs = np.random.RandomState(8)
    X = rs.randn(90, 400)
    Y = rs.randn(90, 6) + 0.5 * X[:, :6]
    kw = dict(n_components=5, n_perm=50, n_boot=60, test_split=4, cv_perm=5, coef_components=3, coef_ci=True,
              vip_components=2, seed=4321, verbose=False)
    without = pls.pls_regression(X, Y, **kw)
    a = pls.pls_regression(X, Y, coef_perm=True, **kw)
    b = pls.pls_regression(X, Y, coef_perm=True, **kw)
    _others_keep_their_bits(without, a)
    for key in KEYS:
        assert np.array_equal(a.permres[key], b.permres[key]), key
    n = 50
    assert a.permres.coefs_pvals.min() >= 1 / (n + 1) and a.permres.coefs_pvals.max() <= 1
    assert np.all(a.permres.coefs_pvals_fwe >= a.permres.coefs_pvals)


def test_global_route_gives_the_bits_of_the_on_chip_route():
    """Fixture `a` on Engine(options={'simpls_global': 1}) against the on-chip route: the three arrays bit-equal.  The
    feature pass is the same kernel on both routes and k_sd_coef's two scatters write identical vectors; what could move
    a bit is the solver's products with K (k_nt_gemm against its strip form), which the maxima inherit.  The differences
    are printed before they are asserted."""
    import pypyls_amd as pls
    g, f, kw = _case('a')
    runs = []
    for glob in (False, True):
        eng = _engine(glob)
        try:
            runs.append(pls.pls_regression(g['X'], g['Y'], coef_perm=True, _engine=eng, **kw))
        finally:
            eng.close()
    for key in KEYS:
        a, b = runs[0].permres[key], runs[1].permres[key]
        print('{}: on-chip vs global max diff / scale {:.3e}'.format(key, max_rel(b, a)))
    for key in KEYS:
        assert np.array_equal(runs[0].permres[key], runs[1].permres[key]), key
