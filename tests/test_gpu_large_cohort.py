"""PLS-C on large cohorts with few features, against the oracle (oracle/cpu_ref.py):

* S = 8192 / 8193: the bound of the compact bootstrap and split-half blocks (their LDS row table holds S rows);
* S = 24 000: the symmetric k_nt_gemm grid of K = X X^T (dual routes) would need 66 066 blocks in y;
* S = 48 000: S^2 > 2^31 (element counts and indices of K past 32 bits), on the engine and through the public calls.

Few features keep the oracle cheap: one resample at S = 48 000, B = 256 is ~10^8 flop."""
import numpy as np
import pytest

from conftest import assert_close, assert_close_per_lv, live_lvs
from oracle import cpu_ref as ref

pytestmark = pytest.mark.gpu


def _data(S, B, T, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B) * (0.5 + rs.rand(1, B))
    Y = rs.randn(S, T) + 0.4 * X[:, :T] if T else None
    return X, Y, rs


def _bind(eng, X, Y, groups, n_cond, method='behavioral', covariance=False, mc=0):
    from pypyls_amd import resampling as rsmp
    eng.set_data(X, Y if method == 'behavioral' else None, rsmp.cell_of_row(groups, n_cond), len(groups), n_cond,
                 0 if method == 'behavioral' else 1, mean_centering=mc, covariance=covariance)
    spec = ref.Spec(method, groups, n_cond, covariance, mc)
    return spec, (Y if method == 'behavioral' else spec.dummy.astype(float))


def _original(eng, spec, X, Yo):
    """The device's decomposition against the oracle's, which is then bound as the original."""
    U, d, V = ref.decompose(spec, X, Yo)
    xw, sv, _ = eng.decompose()
    keep = live_lvs(np.diag(d))
    assert_close(sv[keep], np.diag(d)[keep], 1e-9, what='singvals')
    sg = np.sign(np.sum(xw * U, axis=0))
    assert_close_per_lv(xw * sg, U, 1, 1e-8, what='x_weights', keep=keep)
    eng.set_original(U, np.diag(d), V)
    return U, d, V


def _release():
    import gc
    import pypyls_amd as pls
    pls.release_default_engine()
    gc.collect()


def _check_boots(eng, spec, X, Yo, U, d, boots, what):
    usum, usq, dist = eng.boot(boots)
    usum, usq = usum.cpu().numpy(), usq.cpu().numpy()
    ws, wq, wd = np.zeros_like(U), np.zeros_like(U), []
    for i in range(boots.shape[1]):
        dd, ub = ref.single_boot(spec, X, Yo, boots[:, i], U, d)
        ws += ub
        wq += ub ** 2
        wd.append(dd)
    keep = live_lvs(np.diag(d))
    assert_close_per_lv(usum, ws, 1, 1e-8, what=what + ' sum of rotated bootstrap weights', keep=keep)
    assert_close_per_lv(usq, wq, 1, 1e-8, what=what + ' sum of squared bootstrap weights', keep=keep)
    assert_close_per_lv(usum[-64:], ws[-64:], 1, 1e-8, what=what + ' last feature columns', keep=keep)
    assert_close(dist, np.stack(wd, -1), 1e-9, what=what + ' distrib')


def _check_perm_null(got, want, keep, what):
    """Live LVs to 1e-9; the null LVs of a rank-deficient design (mean-centred: rank J - n_cond) come out of the
    T' x T' Gram matrices as sqrt(eps) d_max instead of ~eps d_max: all rows to 1e-7."""
    assert_close(got[keep], want[keep], 1e-9, what=what)
    assert_close(got, want, 1e-7, what=what + ' (null LVs)')


def _check_perms(eng, spec, X, Yo, V, d, perms, what):
    """Both permutation routes against the oracle and against each other."""
    want = np.stack([ref.single_perm(spec, X, Yo, perms[:, i], V)[0] for i in range(perms.shape[1])], -1)
    keep = live_lvs(np.diag(d))
    got = {}
    for dual in (True, False):
        eng.set_perm_path(dual)
        got[dual] = eng.perm(perms)
        assert bool(eng.last_timing()['dual_perm']) == dual, what + ': permutation route'
        _check_perm_null(got[dual], want, keep, '{} permutations, dual={}'.format(what, dual))
    eng.set_perm_path(True)
    _check_perm_null(got[True], got[False], keep, what + ' permutations: S x S route vs feature pass')


@pytest.mark.parametrize('S', [8192, 8193])
def test_compact_route_bound_on_s(S):
    """S = 8192 is the last cohort of the compact bootstrap and split-half blocks (S <= 8192 in compact_boot_ok and
    run_split_fused; their LDS row table is at its largest there), 8193 the first of the dense blocks.  T' = 20: the
    split-half pass takes the one-pass reader exactly on the compact route (split_route() == 1)."""
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    B, T = 2000, 20
    X, Y, rs = _data(S, B, T, 81 + S)
    # whether compact blocks pay is the cost model's call, a tuning matter; the bound on S is not, and
    # compact_boot_always still gives way above it
    eng = Engine(options={'compact_boot_always': 1})
    try:
        spec, Yo = _bind(eng, X, Y, [S], 1)
        U, d, V = _original(eng, spec, X, Yo)
        _check_perms(eng, spec, X, Yo, V, d, rsmp.gen_permsamp([S], 1, 8, seed=1, verbose=False), 'S = %d' % S)
        boots = rs.randint(0, S, size=(S, 8))
        boots[:2, 0] = (S - 1, 0)                       # a draw of the last row
        _check_boots(eng, spec, X, Yo, U, d, boots, 'S = %d' % S)
        frac = eng.last_timing()['compact_row_fraction']
        assert (frac > 0) == (S <= 8192), 'S = {}: compact_row_fraction {}'.format(S, frac)
        masks = rsmp.gen_splits([S], 1, 4, seed=3)
        uc, vc = eng.split_half(masks)
        assert eng.split_route() == (1 if S <= 8192 else 0), 'S = %d: split-half route' % S
        di = np.linalg.inv(d)
        wu, wv = ref.split_half(spec, X, Yo, U @ di, V @ di, masks)
        assert_close(uc[0].mean(-1), wu, 1e-9, what='S = %d split-half ucorr' % S)
        assert_close(vc[0].mean(-1), wv, 1e-9, what='S = %d split-half vcorr' % S)
    finally:
        eng.close()
    _release()


METHODS = [('behavioral', False), ('behavioral', True), ('meancentered', False)]


def _design(method, S):
    if method == 'meancentered':
        return [S // 6] * 3, 2                          # 3 groups x 2 conditions
    return [S], 1


@pytest.mark.parametrize('method,cov', METHODS)
@pytest.mark.parametrize('S', [24000, 48000])
def test_dual_routes_on_large_cohorts(S, method, cov):
    """K = X X^T of the dual permutation route and of the single-pass bootstrap (unscaled modes) past 65 535 blocks in
    y of the symmetric k_nt_gemm grid (S >= 23 169) and past 2^31 elements (S >= 46 341): permutations on the dual
    route and on the feature pass against the oracle and each other, bootstraps against the oracle."""
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    B, T = 256, 3
    groups, n_cond = _design(method, S)
    X, Y, rs = _data(S, B, T if method == 'behavioral' else 0, S + 7 * cov + (method == 'meancentered'))
    what = '{} cov={} S = {}'.format(method, cov, S)
    eng = Engine()
    try:
        spec, Yo = _bind(eng, X, Y, groups, n_cond, method, cov, 0 if method == 'behavioral' else 1)
        U, d, V = _original(eng, spec, X, Yo)
        _check_perms(eng, spec, X, Yo, V, d, rsmp.gen_permsamp(groups, n_cond, 4, seed=1, verbose=False), what)
        boots = rsmp.gen_bootsamp(groups, n_cond, 4, seed=2, verbose=False)
        boots[-1, 0] = S - 1                            # a draw of the last row (within its cell)
        eng.set_timing(True)                            # (counts the flop of the k_nt_gemm launches from here on)
        _check_boots(eng, spec, X, Yo, U, d, boots, what)
        # the unscaled modes take the single-pass bootstrap, which forms K itself (set_perm_path dropped the permutation
        # leg's): at least the S^2 B flop of its symmetric form; the correlation mode's two-pass route issues none
        nt = eng.last_timing()['nt_flops']
        if cov or method == 'meancentered':
            assert nt >= float(S) * S * B, what + ': bootstraps off the single-pass route (%g flop)' % nt
        else:
            assert nt == 0, what + ': bootstraps off the two-pass route (%g flop)' % nt
    finally:
        eng.close()
    _release()


@pytest.mark.parametrize('method,cov', METHODS)
def test_public_calls_s48000(method, cov):
    """One public call per method at S = 48 000 (S^2 > 2^31) with 32 permutations, 32 bootstraps and 8 split-halves,
    field by field against ref.run_plsc on the same resampling arrays."""
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    B, T, n_perm, n_boot, n_split = 128, 4, 32, 32, 8        # (T' = 2 would make every vcorr +-1: tied p-values)
    groups, n_cond = _design(method, 48000)
    X, Y, rs = _data(48000, B, T if method == 'behavioral' else 0, 480 + cov)
    perms = rsmp.gen_permsamp(groups, n_cond, n_perm, seed=1, verbose=False)
    boots = rsmp.gen_bootsamp(groups, n_cond, n_boot, seed=2, verbose=False)
    splits = rsmp.gen_splits(groups, n_cond, n_split, seed=3)
    psplits = np.stack([rsmp.gen_splits(groups, n_cond, n_split, seed=10 + i) for i in range(n_perm)])
    kw = dict(groups=groups, n_cond=n_cond, n_perm=n_perm, n_boot=n_boot, n_split=n_split, permsamples=perms,
              bootsamples=boots, _splitsamples=splits, _perm_splitsamples=psplits, seed=5, verbose=False)
    if method == 'behavioral':
        res = pls.behavioral_pls(X, Y, covariance=cov, test_split=0, **kw)
    else:
        res = pls.meancentered_pls(X, mean_centering=1, **kw)
    _release()
    want = ref.run_plsc(X, Y, method=method, groups=groups, n_cond=n_cond, covariance=cov,
                        mean_centering=0 if method == 'behavioral' else 1, permsamples=perms, bootsamples=boots,
                        splitsamples=splits, perm_splitsamples=psplits)
    keep = live_lvs(want['singvals'])
    assert_close(res.singvals[keep], want['singvals'][keep], 1e-9, what='singvals')
    assert_close_per_lv(res.x_weights, want['x_weights'], 1, 1e-8, what='x_weights', keep=keep)
    _check_perm_null(res.permres.perm_singval, want['permres']['perm_singval'], keep, 'perm_singval')
    np.testing.assert_array_equal(res.permres.pvals, want['permres']['pvals'])
    for key in ('x_weights_normed', 'x_weights_stderr'):
        assert_close_per_lv(res.bootres[key], want['bootres'][key], 1, 1e-8, what=key, keep=keep)
    # (the null LVs of the mean-centred design -- rank J - n_cond -- have arbitrary weights in both)
    dkey = 'y_loadings' if method == 'behavioral' else 'contrast'
    for key in (dkey + '_boot', dkey + '_ci'):
        assert_close(res.bootres[key][:, keep], want['bootres'][key][:, keep], 1e-9, what=key)
    for key in ('ucorr', 'vcorr', 'ucorr_pvals', 'vcorr_pvals', 'ucorr_lolim', 'ucorr_uplim', 'vcorr_lolim',
                'vcorr_uplim'):
        assert_close(res.splitres[key][keep], want['splitres'][key][keep], 1e-8, what=key)


def _pads(S, B, Tp):
    """Kpad, Bpad, T'pp of plsx_set_data (L = min(T', B) score columns ride behind the B features)."""
    return -(-S // 8) * 8, -(-(B + min(Tp, B)) // 128) * 128, -(-Tp // 4) * 4


@pytest.mark.parametrize('B', [524140, 524141])
def test_compact_route_bound_on_x_bytes(B):
    """S = 512, T' = 20: B = 524 140 is the widest X the compact bootstrap and split-half blocks address (Kpad Bpad 8 <
    2^31: their X offsets are 32-bit byte offsets through a buffer resource), 524 141 the first on the dense blocks.
    (T' = 20 rather than 16: from T'pp = 20 on the compact split-half pass takes the one-pass reader, which makes its
    route visible in split_route().)  R against the oracle on
    column windows (first, middle, last), the rest against numpy on the device's own R of the same resample (as
    test_more_than_two_million_features), split-halves against the oracle."""
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine
    S, T = 512, 20
    compact = B == 524140
    kpad, bpad, _ = _pads(S, B, T)
    assert (kpad * bpad * 8 < 2 ** 31) == compact and (kpad * (bpad + 128) * 8 < 2 ** 31) is False
    X, Y, rs = _data(S, B, T, 9)
    boots = rs.randint(0, S, size=(S, 3))
    boots[:2, 0] = (S - 1, 0)                           # a draw of row 511
    perms = rsmp.gen_permsamp([S], 1, 3, seed=1, verbose=False)
    eng = Engine(options={'compact_boot_always': 1})
    try:
        spec, _ = _bind(eng, X, Y, [S], 1)
        R0 = eng.crosscov(n=1)[0]
        Rp = eng.crosscov(ysrc=perms)
        Rb = eng.crosscov(xsrc=boots, ysrc=boots)
        for lo in (0, B // 2 - 500, B - 1000):
            w = slice(lo, lo + 1000)
            assert_close(R0[:, w], ref.xcorr(X[:, w], Y), 1e-10, what='R columns %d..' % lo)
            assert_close(Rp[2][:, w], ref.xcorr(X[:, w], Y[perms[:, 2]]), 1e-10, what='permuted R columns %d..' % lo)
            assert_close(Rb[0][:, w], ref.xcorr(X[boots[:, 0]][:, w], Y[boots[:, 0]]), 1e-10,
                         what='bootstrap R columns %d..' % lo)
        xw, sv, yw = eng.decompose()
        U0, d0, _ = np.linalg.svd(R0.T, full_matrices=False)
        assert_close(sv, d0, 1e-10, what='singvals')
        assert_close_per_lv(xw * np.sign(np.sum(xw * U0, axis=0)), U0, 1, 1e-8, what='x_weights')
        eng.set_original(xw, sv, yw)
        want_p = np.stack([np.sqrt(np.sum(ref.procrustes(yw, Vt.T, np.diag(dp)) ** 2, axis=0))
                           for _, dp, Vt in (np.linalg.svd(R.T, full_matrices=False) for R in Rp)], -1)
        for dual in (True, False):
            eng.set_perm_path(dual)
            assert_close(eng.perm(perms), want_p, 1e-9, what='permutations, dual=%s' % dual)
            assert bool(eng.last_timing()['dual_perm']) == dual
        eng.set_perm_path(True)
        usum, usq, _ = eng.boot(boots)
        assert (eng.last_timing()['compact_row_fraction'] > 0) == compact, 'bootstrap route'
        want = np.zeros((B, T))
        for R in Rb:
            Ub, db, _ = np.linalg.svd(R.T, full_matrices=False)
            want += ref.procrustes(xw, Ub, np.diag(db))
        assert_close_per_lv(usum.cpu().numpy(), want, 1, 1e-8, what='sum of rotated bootstrap weights')
        assert_close_per_lv(usum.cpu().numpy()[-1000:], want[-1000:], 1, 1e-8, what='last feature columns')
        masks = rsmp.gen_splits([S], 1, 2, seed=3)
        uc, vc = eng.split_half(masks)
        assert eng.split_route() == (1 if compact else 0), 'split-half route'
        wu, wv = ref.split_half(spec, X, Y, xw / sv, yw / sv, masks)
        assert_close(uc[0].mean(-1), wu, 1e-9, what='split-half ucorr')
        assert_close(vc[0].mean(-1), wv, 1e-9, what='split-half vcorr')
    finally:
        eng.close()
    _release()


def _gram_svd(R):
    """Singular values (descending) and left vectors V of a wide R (T' x B) through R R^T: the full SVD of a 2 GB R
    would cost the host more than the rest of the test."""
    lam, V = np.linalg.eigh(R @ R.T)
    order = np.argsort(lam)[::-1]
    return np.sqrt(np.maximum(lam[order], 0.0)), V[:, order]


def test_one_r_slot_bound_at_t50():
    """T' = 50 (T'pp = 52), S = 64: B = 5 162 062 is the widest X whose cross-covariance matrix R_r (T'pp x Bpad
    doubles, read through 31-bit buffer offsets) stays below 2 GB; B = 5 162 063 is refused.  On the admitted shape
    every kernel that reads R_r runs: R on column windows (first, middle, last) against the oracle; decomposition,
    permutations on both routes and bootstraps (one draws row 63) against numpy on the device's own R of the same
    resample; split-halves against the oracle.  X is 2.6 GB, so the checks fetch one R at a time and compare the
    weights on column windows."""
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine, PlsxError
    S, T = 64, 50
    for B, ok in ((5162062, True), (5162063, False)):
        kpad, bpad, tpp = _pads(S, B, T)
        assert (tpp * bpad * 8 < 2 ** 31) == ok
        assert kpad * bpad * 8 >= 2 ** 31                   # X past the compact blocks' offsets: dense blocks only
    rs = np.random.RandomState(50)
    B = 5162062
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.3 * X[:, :T]
    wins = [slice(lo, lo + 1000) for lo in (0, B // 2 - 500, B - 1000)]
    perms = rsmp.gen_permsamp([S], 1, 2, seed=1, verbose=False)
    boots = rs.randint(0, S, size=(S, 2))
    boots[:2, 0] = (S - 1, 0)                               # a draw of row 63
    eng = Engine()
    try:
        eng.set_data(X, Y, rsmp.cell_of_row([S], 1), 1, 1, 0)
        spec = ref.Spec('behavioral', [S], 1)
        R0 = eng.crosscov(n=1)[0]
        for w in wins:
            assert_close(R0[:, w], ref.xcorr(X[:, w], Y), 1e-10, what='R columns %d..' % w.start)
        d0, V0 = _gram_svd(R0)
        xw, sv, yw = eng.decompose()
        assert_close(sv, d0, 1e-9, what='singvals')
        sg = np.sign(np.sum(yw * V0, axis=0))
        assert_close_per_lv(yw * sg, V0, 1, 1e-8, what='y_weights')
        for w in wins:
            assert_close_per_lv(xw[w] * sg, R0[:, w].T @ V0 / d0, 1, 1e-8, what='x_weights columns %d..' % w.start)
        del R0
        eng.set_original(xw, sv, yw)
        # permutations: both routes against each other and against numpy on the device's permuted R
        got = {}
        for dual in (True, False):
            eng.set_perm_path(dual)
            got[dual] = eng.perm(perms)
            assert bool(eng.last_timing()['dual_perm']) == dual, 'permutation route'
        eng.set_perm_path(True)
        assert_close(got[True], got[False], 1e-9, what='permutations: S x S route vs feature pass')
        for i in range(perms.shape[1]):
            dp, Vp = _gram_svd(eng.crosscov(ysrc=perms[:, [i]])[0])
            want = np.sqrt(np.sum(ref.procrustes(yw, Vp, np.diag(dp)) ** 2, axis=0))
            assert_close(got[False][:, i], want, 1e-9, what='permutation %d' % i)
        # bootstraps (dense blocks: X is past the compact bound) against the rotation of the device's bootstrap R
        usum, usq, _ = eng.boot(boots)
        assert eng.last_timing()['compact_row_fraction'] == 0, 'bootstrap route'
        usum, usq = usum.cpu().numpy(), usq.cpu().numpy()
        ws = [np.zeros((1000, T)) for _ in wins]
        wq = [np.zeros((1000, T)) for _ in wins]
        for i in range(boots.shape[1]):
            Rb = eng.crosscov(xsrc=boots[:, [i]], ysrc=boots[:, [i]])[0]
            db, Vb = _gram_svd(Rb)
            # ref.procrustes_live: a bootstrap draws ~41 distinct rows of 64, so R_b has rank < T' = 50 and only its
            # live vectors are rotated onto x_weights (U_b = R_b^T V_b / d_b, live columns)
            live = db > ref.RANK_RTOL * db[0]
            db, Vb = db[live], Vb[:, live]
            N, _, P = np.linalg.svd((Rb @ xw).T @ Vb / db, full_matrices=False)    # xw^T U_b
            rot = np.diag(db) @ (P.T @ N.T)
            for k, w in enumerate(wins):
                ub = (Rb[:, w].T @ Vb / db) @ rot
                ws[k] += ub
                wq[k] += ub ** 2
            del Rb
        for k, w in enumerate(wins):
            assert_close_per_lv(usum[w], ws[k], 1, 1e-8, what='sum of rotated bootstrap weights %d..' % w.start)
            assert_close_per_lv(usq[w], wq[k], 1, 1e-8, what='sum of squared bootstrap weights %d..' % w.start)
        # split-halves (dense layout: the compact split-half blocks share the compact bound)
        masks = rsmp.gen_splits([S], 1, 2, seed=3)
        uc, vc = eng.split_half(masks)
        assert eng.split_route() == 0, 'split-half route'
        wu, wv = ref.split_half(spec, X, Y, xw / sv, yw / sv, masks)
        assert_close(uc[0].mean(-1), wu, 1e-9, what='split-half ucorr')
        assert_close(vc[0].mean(-1), wv, 1e-9, what='split-half vcorr')
        with pytest.raises(PlsxError, match='below 2 GB'):
            eng.set_data(np.zeros((S, B + 1)), Y, rsmp.cell_of_row([S], 1), 1, 1, 0)
    finally:
        eng.close()
    _release()


def test_refuses_plsc_k_beyond_device_memory():
    """S = 300 000: K = X X^T of the dual routes would be 720 GB.  A binding that would take those routes is refused
    with both sizes named; one that will not (the no_dual_perm option: permutations and bootstraps on the feature pass)
    is still bound."""
    from pypyls_amd import resampling as rsmp
    from pypyls_amd.engine import Engine, PlsxError
    rs = np.random.RandomState(0)
    S = 300000
    X, Y = rs.randn(S, 3), rs.randn(S, 2)
    for method in ('behavioral', 'meancentered'):
        groups, n_cond = ([S], 1) if method == 'behavioral' else ([S // 2] * 2, 1)
        eng = Engine()
        try:
            with pytest.raises(PlsxError, match='does not fit in the free device memory'):
                _bind(eng, X, Y, groups, n_cond, method, False, 0 if method == 'behavioral' else 1)
        finally:
            eng.close()
    eng = Engine(options={'no_dual_perm': 1})
    try:
        _bind(eng, X, Y, [S], 1)
        assert eng.S == S and eng.last_timing()['dual_perm'] == 0
    finally:
        eng.close()
    _release()
