"""pls_regression(vip_components=c, vip_perm=True) on the device (plsx_simpls_vip_perm_test / _begin / _end:
k_vip_perm_prod, k_coef_perm_max, k_sd_vip along the permutation batches): the stateless entry against numpy across the
tile edges, its bits against k_vip_prod's, the chunking of the features, the series along plsx_simpls_perm_batch (alone
and next to the coefficient series), the reference fixtures through the public call (one device and a team of two), the
global solver route, every other option, a constant feature, pls_da, confounds.

Gates: RTOL = 1e-5 through conftest.assert_close against the reference fixtures -- the bar
tests/test_gpu_regression_vip.py holds ``vip`` to.  The stateless entry is compared with numpy on the SAME stack: both
sides are fp64 sums of c S <= 260 products under a square root, and a maximum is a continuous function of its
arguments, so the maxima are held to the 1e-10 of the stack test of tests/test_gpu_regression_vip.py.  Counts are
integers and are compared for EXACT equality everywhere: the fixtures keep every vip_p at least 1e-8 vip away from vip
(their generator refuses anything closer); for the random stacks the observed scores are placed half way between two
neighbouring order statistics of numpy's own series, whose relative spacing is asserted to exceed 1e-9 before the device
is asked; the confounds case asserts its own gap of 1e-6.  Every figure is printed before it is asserted; no entry is
left out of a comparison."""
import numpy as np
import pytest

from conftest import load_golden, assert_close
from regression_coef_expect import max_rel
from regression_vip_perm_expect import stack_series, stack_test, vip_perm_expected, min_rel_gap

pytestmark = pytest.mark.gpu
RTOL = 1e-5
NUMPY = 1e-10
KEYS = ('vip_pvals', 'vip_max', 'vip_pvals_fwe')
CKEYS = ('coefs_pvals', 'coefs_max', 'coefs_pvals_fwe')


def _engine(glob=False, **kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1} if glob else {}, **kw)


def _bind(eng, S, B, T, k, seed):
    """Bind random data; the last feature is four times the scale of the others, so that a stack row along it puts a
    permutation's maximum there.  Returns the centred X as the device holds it, and the stream."""
    rs = np.random.RandomState(seed)
    X, Y = rs.randn(S, B), rs.randn(S, T)
    X[:, B - 1] *= 4.0
    Xc = X - X.mean(axis=0)
    eng.set_data_regression(Xc, Y - Y.mean(axis=0), k)
    return Xc - Xc.mean(axis=0), rs                    # (the device centres what it is given once more)


def _obs_between(series, rs):
    """Observed scores (B,) whose exceedance counts over the finite rows of ``series`` (n, B) span 0 .. n: feature f sits
    half way between two neighbouring order statistics of its own column (rank drawn), feature 0 above all of its
    column, feature 1 at zero.  The smallest relative distance to a value of the column is returned with them."""
    v = np.sort(series[np.isfinite(series).all(axis=1)], axis=0)
    m, B = v.shape
    obs = np.empty(B)
    for f in range(B):
        r = rs.randint(0, m + 1)
        obs[f] = 0.5 * v[0, f] if r == 0 else (2.0 * v[-1, f] if r == m else 0.5 * (v[r - 1, f] + v[r, f]))
    obs[0] = 2.0 * v[-1, 0]
    if B > 1:
        obs[1] = 0.0
    nz = obs > 0
    gap = float((np.abs(v[:, nz] - obs[nz][None]) / obs[nz][None]).min())
    return obs, gap


def _stateless(eng, stack, obs, count=None):
    import torch
    if count is None:
        count = torch.zeros((obs.shape[0],), dtype=torch.int32, device=eng.device)
    dmax = eng._zeros((stack.shape[0],))
    eng.simpls_vip_perm_test(eng._dev(stack, np.float64), eng._dev(obs, np.float64), count, dmax)
    eng.sync()
    return count, dmax.cpu().numpy()


@pytest.mark.parametrize('S,B,c,n', [(37, 150, 3, 70), (64, 300, 2, 70), (5, 17, 1, 1), (130, 129, 2, 2)])
def test_stateless_entry_against_numpy_across_tile_edges(S, B, c, n):
    """(37, 150, 3, 70): the unaligned pair loads of the stack, a partial last stage, a partial last feature block, a
    partial second permutation tile; (64, 300, 2, 70): the aligned path, three feature blocks; (5, 17, 1, 1): one
    partial stage, one permutation; (130, 129, 2, 2): five stages, one live feature in the second block.  One stack row
    is planted so that the maximum of the last permutation sits in the last, partial feature block; where n >= 3 the rows
    of permutation 1 are all NaN: it leaves maximum 0 and adds to no count.  A second call on the same counts doubles them
    and repeats the maxima bit for bit."""
    eng = _engine()
    try:
        Xc, rs = _bind(eng, S, B, 2, c, seed=S + B + n)
        stack = rs.randn(n, c, S)
        stack[n - 1, 0] = 50.0 * Xc[:, B - 1] / np.linalg.norm(Xc[:, B - 1])
        if n >= 3:
            stack[1] = np.nan
        series = stack_series(Xc, stack)
        obs, gap = _obs_between(series, rs)
        want_count, want_max = stack_test(Xc, stack, obs)
        assert gap > 1e-9 and want_count.min() == 0 and want_count.max() == n - (1 if n >= 3 else 0)
        assert np.argmax(series[n - 1]) == B - 1                 # (the planted maximum, by numpy)
        count, got_max = _stateless(eng, stack, obs)
        got_count = count.cpu().numpy()
        err = max_rel(got_max, want_max)
        print('S={} B={} c={} n={}: maxima err / scale {:.3e}, counts {} .. {}, differing counts {}, gap {:.1e}'.format(
            S, B, c, n, err, got_count.min(), got_count.max(), int((got_count != want_count).sum()), gap))
        assert got_max.shape == (n,) and got_count.shape == (B,)
        assert err <= NUMPY
        assert_close(got_max, want_max, rtol=NUMPY, what='maxima')
        assert np.array_equal(got_count, want_count)
        assert abs(got_max[n - 1] - series[n - 1, B - 1]) <= NUMPY * series[n - 1, B - 1]
        if n >= 3:
            assert got_max[1] == 0.0 and np.all(got_max[np.arange(n) != 1] > 0.0)
        count2, again = _stateless(eng, stack, obs, count=count)
        assert np.array_equal(count2.cpu().numpy(), 2 * want_count) and np.array_equal(again, got_max)
    finally:
        eng.close()


@pytest.mark.parametrize('S', [37, 64])
def test_the_permutation_pass_has_the_bits_of_k_vip_prod(S):
    """k_vip_perm_prod runs k_vip_prod's loop over k_vip_prod's pieces, so a score is the same bits whichever of them
    forms it and wherever its resample sits in a tile.  B = 150, c = 3, n = 70.  The series comes from
    plsx_simpls_vip_ci on the one-resample stacks stack[b:b+1] (a series of one value: lo = hi = the score); the
    permutation pass over the whole stack must then give max_f series[b] and sum_b (series[b] >= obs) exactly.  The
    number of differing values is printed before it is asserted to be zero."""
    import torch
    B, c, n = 150, 3, 70
    eng = _engine()
    try:
        _, rs = _bind(eng, S, B, 2, c, seed=S)
        stack = rs.randn(n, c, S)
        d_stack = eng._dev(stack, np.float64)
        series = np.empty((n, B))
        for b in range(n):
            _, lo, hi = eng.simpls_vip_ci(d_stack[b:b + 1])
            assert torch.equal(lo, hi)
            series[b] = lo.cpu().numpy()
        assert np.all(np.isfinite(series)) and series.min() > 0.0
        obs = np.median(series, axis=0) * (0.5 + rs.rand(B))
        obs[:n] = series[np.arange(n), np.arange(n)]              # exact ties with k_vip_prod's own bits must count
        count, dmax = _stateless(eng, stack, obs)
        want_count = (series >= obs[None]).sum(axis=0)
        differing = int((dmax != series.max(axis=1)).sum())
        print('S={}: maxima differing in any bit {} of {}, counts differing {} of {}'.format(
            S, differing, dmax.size, int((count.cpu().numpy() != want_count).sum()), B))
        assert differing == 0 and np.array_equal(dmax, series.max(axis=1))
        assert np.array_equal(count.cpu().numpy(), want_count)
    finally:
        eng.close()


def test_stateless_entry_gives_the_same_bits_when_the_features_go_in_chunks():
    """S = 64, B = 300, c = 2, n = 12 000: 12.29 MB of stack, 96 KB of partial maxima per feature block.  A scratch
    budget of the stack plus 150 KB leaves room for one block per chunk (three chunks instead of one)."""
    S, B, c, n = 64, 300, 2, 12000
    stack_bytes = 8 * n * c * S
    got = {}
    want = None
    for name, kw in (('default', {}), ('three chunks', dict(scratch_gb=(stack_bytes + 150e3) / 2 ** 30))):
        eng = _engine(**kw)
        try:
            Xc, rs = _bind(eng, S, B, 2, c, seed=11)
            stack = rs.randn(n, c, S)
            if want is None:
                series = stack_series(Xc, stack)
                obs, gap = _obs_between(series, rs)
                want = stack_test(Xc, stack, obs)
                assert gap > 1e-9
            eng.set_timing(True)
            count, dmax = _stateless(eng, stack, obs)
            launches = eng.kernel_timing()['k_coef_prod'][1]
            print('{}: {} timed brackets of the feature pass'.format(name, launches))
            assert launches == (1 if name == 'default' else 3), (name, launches)
            got[name] = (count.cpu().numpy(), dmax)
        finally:
            eng.close()
        err = max_rel(got[name][1], want[1])
        print('{}: maxima err / scale {:.3e}, gap {:.1e}'.format(name, err, gap))
        assert err <= NUMPY and np.array_equal(got[name][0], want[0])
    assert np.array_equal(got['default'][0], got['three chunks'][0])
    assert np.array_equal(got['default'][1], got['three chunks'][1])


def _series_setup(eng, S, B, T, k, seed, n):
    import torch
    Xc, rs = _bind(eng, S, B, T, k, seed)
    d_W, _, _ = eng.simpls_decompose_dev()
    eng.simpls_set_original_dev(d_W)
    eng.sync()
    vobs = 0.5 + rs.rand(B)                                      # (VIP scores scatter around 1)
    cobs = rs.randn(B, T) * 0.05
    perms = np.stack([rs.permutation(S) for _ in range(n)], axis=1).astype(np.int32)
    return eng._dev(vobs, np.float64), eng._dev(cobs, np.float64), eng.rows_tensor(perms.T), torch


def _run_series(eng, c, d_vobs, d_cobs, idx, pieces, torch, vip=True, coef=False):
    """(pctvar, VIP counts, VIP maxima, coefficient counts, coefficient maxima) of the permutations ``idx`` submitted in
    ``pieces``, with the VIP series and / or the coefficient series open."""
    n, B, T = idx.shape[0], d_cobs.shape[0], d_cobs.shape[1]
    out = eng._zeros((n, eng.k))
    vcount, vmax = torch.zeros((B,), dtype=torch.int32, device=eng.device), eng._zeros((n,))
    ccount, cmax = torch.zeros((B, T), dtype=torch.int32, device=eng.device), eng._zeros((n, T))
    if coef:
        eng.simpls_coef_perm_begin(c, d_cobs, ccount, cmax)
    if vip:
        eng.simpls_vip_perm_begin(c, d_vobs, vcount, vmax)
    for a, b in pieces:
        eng.simpls_perm_into(idx[a:b], out[a:b])
    if vip:
        eng.simpls_vip_perm_end()
    if coef:
        eng.simpls_coef_perm_end()
    eng.sync()
    return tuple(t.cpu().numpy() for t in (out, vcount, vmax, ccount, cmax))


def test_series_along_the_permutation_batches():
    """S = 1000, B = 300, T = 3, k = 4, c = 2, 70 permutations.  pctvar has the same bits with the series open; counts
    and maxima are the sum / concatenation of two half-size calls, also under a 0.02 GB scratch budget -- half of it
    takes 38 permutations of 264 392 bytes of solver state plus 16 000 of scaled dual weights, so the solver batches are
    38 + 32 --; the coefficient series and the VIP series open together give what each gives alone; a batch that would
    pass the capacity is refused with nothing computed."""
    from pypyls_amd.engine import PlsxError
    S, B, T, k, c, n = 1000, 300, 3, 4, 2, 70
    runs = {}
    for name, kw in (('default', {}), ('0.02 GB', dict(scratch_gb=0.02))):
        eng = _engine(**kw)
        try:
            d_vobs, d_cobs, idx, torch = _series_setup(eng, S, B, T, k, 17, n)
            plain = _run_series(eng, c, d_vobs, d_cobs, idx, [(0, n)], torch, vip=False)
            eng.set_timing(True)
            whole = _run_series(eng, c, d_vobs, d_cobs, idx, [(0, n)], torch)
            batches = eng.kernel_timing()['k_sd_coef'][1]           # (k_sd_vip is filed with k_sd_coef: one per batch)
            eng.set_timing(False)
            halves = _run_series(eng, c, d_vobs, d_cobs, idx, [(0, 35), (35, n)], torch)
            print('scratch {}: {} solver batches; counts {} .. {}, maxima {:.3f} .. {:.3f}'.format(
                name, batches, whole[1].min(), whole[1].max(), whole[2].min(), whole[2].max()))
            assert batches == (1 if name == 'default' else 2)
            assert np.array_equal(plain[0], whole[0]), 'pctvar moved with the series open'
            assert not plain[1].any() and not plain[2].any()
            for i, what in enumerate(('pctvar', 'counts', 'maxima')):
                assert np.array_equal(whole[i], halves[i]), (name, what)
            assert 0 < whole[1].max() and whole[1].min() < n and np.isfinite(whole[2]).all() and (whole[2] >= 1.0).all()
            # both series open: each gives what it gives alone
            conly = _run_series(eng, c, d_vobs, d_cobs, idx, [(0, n)], torch, vip=False, coef=True)
            both = _run_series(eng, c, d_vobs, d_cobs, idx, [(0, 35), (35, n)], torch, vip=True, coef=True)
            assert conly[3].any() and (conly[4] > 0).all()
            for i, what in enumerate(('pctvar', 'VIP counts', 'VIP maxima')):
                assert np.array_equal(both[i], whole[i]), (name, 'both open', what)
            for i, what in ((3, 'coefficient counts'), (4, 'coefficient maxima')):
                assert np.array_equal(both[i], conly[i]), (name, 'both open', what)
            runs[name] = whole
            # capacity: a series of 35 takes 35, then refuses one more before it computes anything
            out = eng._zeros((n, eng.k))
            count = torch.zeros((B,), dtype=torch.int32, device=eng.device)
            dmax = eng._zeros((35,))
            eng.simpls_vip_perm_begin(c, d_vobs, count, dmax)
            eng.simpls_perm_into(idx[:35], out[:35])
            eng.sync()
            before = count.clone()
            with pytest.raises(PlsxError, match='status -1.*VIP series'):
                eng.simpls_perm_into(idx[35:36], out[35:36])
            eng.sync()
            assert float(out[35:].abs().sum()) == 0.0 and torch.equal(before, count)
            assert np.array_equal(dmax.cpu().numpy(), whole[2][:35])
            eng.simpls_vip_perm_end()
            for bad in (0, k + 1):
                with pytest.raises(PlsxError, match='status -1'):
                    eng.simpls_vip_perm_begin(bad, d_vobs, count, dmax)
        finally:
            eng.close()
    for i, what in enumerate(('pctvar', 'counts', 'maxima')):
        assert np.array_equal(runs['default'][i], runs['0.02 GB'][i]), what


def test_series_needs_the_original_fit_and_valid_arguments():
    import torch
    from pypyls_amd.engine import PlsxError
    eng = _engine()
    try:
        _bind(eng, 40, 60, 2, 2, seed=3)
        obs, count, dmax = eng._zeros((60,)), torch.zeros((60,), dtype=torch.int32, device=eng.device), eng._zeros((4,))
        stack = eng._zeros((4, 2, 40))
        with pytest.raises(PlsxError, match='status -4'):
            eng.simpls_vip_perm_begin(1, obs, count, dmax)
        lib, ptr = eng.lib, lambda t: t.data_ptr()
        for args in ((None, 4, 2, ptr(obs), ptr(count), ptr(dmax)), (ptr(stack), 4, 2, None, ptr(count), ptr(dmax)),
                     (ptr(stack), 4, 2, ptr(obs), None, ptr(dmax)), (ptr(stack), 4, 2, ptr(obs), ptr(count), None),
                     (ptr(stack), 0, 2, ptr(obs), ptr(count), ptr(dmax)), (ptr(stack), 4, 0, ptr(obs), ptr(count), ptr(dmax)),
                     (ptr(stack), 4, 3, ptr(obs), ptr(count), ptr(dmax))):
            with pytest.raises(PlsxError, match='status -1'):
                eng._check(lib.plsx_simpls_vip_perm_test(eng.ctx, *args, None))
        d_W, _, _ = eng.simpls_decompose_dev()
        eng.simpls_set_original_dev(d_W)
        eng.sync()
        for args in ((1, None, ptr(count), ptr(dmax), 4), (1, ptr(obs), None, ptr(dmax), 4),
                     (1, ptr(obs), ptr(count), None, 4), (1, ptr(obs), ptr(count), ptr(dmax), 0)):
            with pytest.raises(PlsxError, match='status -1'):
                eng._check(lib.plsx_simpls_vip_perm_begin(eng.ctx, *args))
        eng.simpls_vip_perm_begin(2, obs, count, dmax)
        eng.simpls_vip_perm_end()
        eng.sync()
        assert not count.any() and not dmax.any()
    finally:
        eng.close()


def _case(tag):
    g, p, f = load_golden('simpls_coef_' + tag), load_golden('simpls_coef_perm_' + tag), load_golden('simpls_vip_perm_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    kw = dict(n_components=k, n_perm=p['permsamples'].shape[1], permsamples=p['permsamples'], n_boot=0, aggfunc=aggfunc,
              vip_components=c, seed=1, verbose=False)
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
    B, n = g['X'].shape[1], kw['n_perm']
    without = pls.pls_regression(g['X'], g['Y'], **kw)
    res = pls.pls_regression(g['X'], g['Y'], vip_perm=True, **kw)
    pr = res.permres
    assert pr.vip_pvals.shape == (B,) and pr.vip_max.shape == (n,) and pr.vip_pvals_fwe.shape == (B,)
    err = max_rel(pr.vip_max, f['ref_max'])
    count = np.rint(pr.vip_pvals * (n + 1) - 1).astype(int)
    print('simpls_vip_perm_{}: vip_max err / scale {:.3e}; differing counts {}; differing maxT p-values {}'.format(
        tag, err, int((count != f['ref_count']).sum()), int((pr.vip_pvals_fwe != f['ref_pvals_fwe']).sum())))
    assert_close(pr.vip_max, f['ref_max'], rtol=RTOL, what='vip_max vs reference')
    assert np.array_equal(count, f['ref_count'])
    assert np.array_equal(pr.vip_pvals, f['ref_pvals'])
    assert np.array_equal(pr.vip_pvals_fwe, f['ref_pvals_fwe'])
    assert res.inputs.vip_perm is True and 'vip_perm' not in without.inputs
    _others_keep_their_bits(without, res)
    two = pls.pls_regression(g['X'], g['Y'], vip_perm=True, device_ids=[0, 0], **kw)
    for key in KEYS:
        assert np.array_equal(two.permres[key], pr[key]), 'team of two: ' + key


def test_global_route_gives_the_bits_of_the_on_chip_route():
    """Fixture `a` on Engine(options={'simpls_global': 1}) against the on-chip route: the three arrays bit-equal.  The
    feature pass is the same kernel on both routes and k_sd_vip's two scatters write identical vectors; what could move
    a bit is the solver's products with K (k_nt_gemm against its strip form), which the maxima inherit.  The differences
    are printed before they are asserted."""
    import pypyls_amd as pls
    g, f, kw = _case('a')
    runs = []
    for glob in (False, True):
        eng = _engine(glob)
        try:
            runs.append(pls.pls_regression(g['X'], g['Y'], vip_perm=True, _engine=eng, **kw))
        finally:
            eng.close()
    for key in KEYS:
        a, b = runs[0].permres[key], runs[1].permres[key]
        print('{}: on-chip vs global max diff / scale {:.3e}'.format(key, max_rel(b, a)))
    for key in KEYS:
        assert np.array_equal(runs[0].permres[key], runs[1].permres[key]), key


def test_next_to_every_other_option_nothing_else_moves():
    """coef_perm, coef_ci, test_split, cv_perm and bootstraps in the same seeded call, drawn permutations: every other
    array is np.array_equal with and without the keyword, and two runs with it give the same bits."""
    import pypyls_amd as pls
    rs = np.random.RandomState(8)
    X = rs.randn(90, 400)
    Y = rs.randn(90, 6) + 0.5 * X[:, :6]
    n = 50
    kw = dict(n_components=5, n_perm=n, n_boot=60, test_split=4, cv_perm=5, coef_components=3, coef_ci=True,
              coef_perm=True, vip_components=2, seed=4321, verbose=False)
    without = pls.pls_regression(X, Y, **kw)
    a = pls.pls_regression(X, Y, vip_perm=True, **kw)
    b = pls.pls_regression(X, Y, vip_perm=True, **kw)
    _others_keep_their_bits(without, a)
    for key in KEYS + CKEYS:
        assert np.array_equal(a.permres[key], b.permres[key]), key
    print('vip_pvals {:.4f} .. {:.4f}, vip_pvals_fwe {:.4f} .. {:.4f}'.format(
        a.permres.vip_pvals.min(), a.permres.vip_pvals.max(), a.permres.vip_pvals_fwe.min(), a.permres.vip_pvals_fwe.max()))
    for key in ('vip_pvals', 'vip_pvals_fwe'):
        assert a.permres[key].min() >= 1 / (n + 1) and a.permres[key].max() <= 1
    assert np.all(a.permres.vip_pvals_fwe >= a.permres.vip_pvals)
    assert np.isfinite(a.permres.vip_max).all() and a.permres.vip_max.min() >= 1.0


def test_a_constant_feature_has_p_one_in_both_arrays():
    """Two features without variance, one constant at 3 and one at 0 (S = 32: the column mean of the first is exact in
    any order of summation, so its centred column is exactly zero): VIP 0 under every arrangement, p = 1 in both
    arrays; the others vary."""
    import pypyls_amd as pls
    rs = np.random.RandomState(5)
    X, Y = rs.randn(32, 200), rs.randn(32, 2)
    X[:, 6] = 3.0
    X[:, 150] = 0.0
    res = pls.pls_regression(X, Y, n_components=3, n_perm=12, n_boot=0, vip_components=2, vip_perm=True, seed=2,
                             verbose=False)
    for f in (6, 150):
        assert res.vip[f] == 0.0 and res.permres.vip_pvals[f] == 1.0 and res.permres.vip_pvals_fwe[f] == 1.0
    assert res.permres.vip_pvals.min() < 1.0 and np.isfinite(res.permres.vip_max).all()


def test_pls_da_passes_the_keyword_through():
    import pypyls_amd as pls
    rs = np.random.RandomState(12)
    S, B, G = 60, 150, 3
    y = np.arange(S) % G
    X = rs.randn(S, B)
    X[:, :5] += 0.8 * y[:, None]
    onehot = np.zeros((S, G))
    onehot[np.arange(S), y] = 1.0
    kw = dict(n_components=3, n_perm=20, n_boot=0, vip_components=2, vip_perm=True, seed=9, verbose=False)
    da = pls.pls_da(X, y, **kw)
    reg = pls.pls_regression(X, onehot, **kw)
    assert da.inputs.vip_perm is True
    for key in KEYS:
        assert np.array_equal(da.permres[key], reg.permres[key]), key
    assert da.permres.vip_pvals[:5].max() <= da.permres.vip_pvals[5:].mean()


def test_confounds_against_the_expectation_on_host_residualised_data():
    """S = 60, B = 150, T = 3, q = 2, k = 4, c = 2, 30 given permutations: the call with confounds=Z against the oracle's
    expectation on numpy's residuals (X_r, Y_r) -- the rows of Y_r permuted against X_r.  The seed is one for which the
    oracle-side gap, computed and asserted here, exceeds 1e-6 (4.6e-4 per feature, 2.6e-3 against the maxima): the two
    residualisations differ by rounding only, so the counts must be equal."""
    import pypyls_amd as pls
    from confound_expect import residualise
    S, B, T, q, k, c, n = 60, 150, 3, 2, 4, 2, 30
    rs = np.random.RandomState(33)
    Z = rs.randn(S, q)
    X = rs.randn(S, B) + Z @ rs.randn(q, B)
    Y = rs.randn(S, T) + 0.6 * X[:, :T] + Z @ rs.randn(q, T)
    perms = np.stack([rs.permutation(S) for _ in range(n)], axis=1).astype(np.int32)
    allr = np.ones(S, dtype=bool)
    want = vip_perm_expected(residualise(X, Z, allr), residualise(Y, Z, allr), perms, k, c)
    gaps = min_rel_gap(want['vip'], want['perms'])
    assert min(gaps) > 1e-6, gaps
    kw = dict(n_components=k, n_perm=n, permsamples=perms, n_boot=0, vip_components=c, seed=1, verbose=False)
    res = pls.pls_regression(X, Y, confounds=Z, vip_perm=True, **kw)
    pr = res.permres
    count = np.rint(pr.vip_pvals * (n + 1) - 1).astype(int)
    print('confounds: gaps {:.1e} / {:.1e}; vip err {:.3e}, vip_max err {:.3e}, differing counts {}, differing maxT {}'.format(
        gaps[0], gaps[1], max_rel(res.vip, want['vip']), max_rel(pr.vip_max, want['vip_max']),
        int((count != want['count']).sum()), int((pr.vip_pvals_fwe != want['vip_pvals_fwe']).sum())))
    assert_close(res.vip, want['vip'], rtol=RTOL, what='vip on the residuals')
    assert_close(pr.vip_max, want['vip_max'], rtol=RTOL, what='vip_max on the residuals')
    assert np.array_equal(count, want['count'])
    assert np.array_equal(pr.vip_pvals, want['vip_pvals'])
    assert np.array_equal(pr.vip_pvals_fwe, want['vip_pvals_fwe'])
    _others_keep_their_bits(pls.pls_regression(X, Y, confounds=Z, **kw), res)
