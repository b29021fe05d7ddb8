"""behavioral_pls / meancentered_pls(weights_perm=m) on the device (plsx_perm_weights_build / plsx_perm_weights_test:
k_perm_W_behav, k_perm_VA + k_perm_W_mc, k_col_rsd, then k_coef_perm_prod / k_coef_perm_max over the binding's feature
matrix): the builders against numpy, the stateless test against the oracle's counts and maxima across tile edges,
pieces and chunks, the public call against the expectation, what must not move, a team, the refusals.

Gates.  The builders: W_p @ Xf, Xf formed in numpy, against the oracle's Z_p to NUMPY = 1e-10 of the largest entry --
both sides are fp64 sums of at most S <= 124 (then B) products of O(1) numbers, 1e-13 at worst; in correlation mode the
two sides also form 1 / std by the same two-pass formula.  Counts: exactly equal, after `closeness >= 1e-8` has been
asserted on the ORACLE's values (tests/weights_perm_expect.py: no comparison within eight digits of a tie, the device
within twelve of the oracle).  Maxima: RTOL = 1e-5 through conftest.assert_close, the bar of the coef_perm fixtures.
Bit equality across piece sizes, chunkings, repeated calls and a team.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

from conftest import assert_close
import weights_perm_expect as wp

pytestmark = pytest.mark.gpu
RTOL = 1e-5
NUMPY = 1e-10


def _engine(options=None, **kw):
    from pypyls_amd.engine import Engine
    return Engine(options=options or {}, **kw)


def max_rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = np.max(np.abs(b)) if b.size else 1.0
    return float(np.max(np.abs(a - b)) / scale) if b.size else 0.0


def _data(method, groups, n_cond, B, T, seed):
    """Features of unequal scale and offset (so that s_f matters), cell effects for mean-centred PLS, a behaviour that
    follows the first features."""
    S = sum(groups) * n_cond
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B) * (0.5 + 2.0 * rs.rand(B)) + 2.0 * rs.rand(1, B)
    if method == 'meancentered':
        X += np.repeat(rs.randn(len(groups) * n_cond, B), np.repeat(groups, n_cond), axis=0)
        return X, None, rs
    Y = rs.randn(S, T)
    k = min(T, B)
    Y[:, :k] += 0.5 * X[:, :k]
    return X, Y, rs


def _bind(eng, spec, X, Y):
    from pypyls_amd import resampling
    cells = resampling.cell_of_row(spec.groups, spec.n_cond)
    eng.set_data(X, Y, cells, len(spec.groups), spec.n_cond, 0 if spec.method == 'behavioral' else 1,
                 mean_centering=spec.mean_centering, covariance=spec.covariance)


def _standardise(spec):
    return not (spec.method == 'behavioral' and not spec.covariance)


# ---------------------------------------------------------------------------------------------------------------------
# the builders against numpy
# ---------------------------------------------------------------------------------------------------------------------

BUILD_CASES = [
    # method, groups, n_cond, T, m, covariance, mean_centering, B
    ('behavioral', [37], 1, 3, 3, False, 0, 40),                   # one cell, odd S
    ('behavioral', [64], 1, 3, 3, False, 0, 40),                   # one cell, S = one chunk of 64 rows exactly
    ('behavioral', [13, 11], 2, 3, 12, False, 0, 40),              # T' = 12, unequal cells, every column
    ('behavioral', [13, 11], 2, 3, 5, False, 0, 40),               # ... and the first five
    ('behavioral', [45], 1, 20, 20, False, 0, 40),                 # T = 20 in one cell: V0 spans more than one 16-row tile
    ('behavioral', [90], 1, 70, 70, False, 0, 80),                 # T' = 70 > 64: the block of V0 stays in global memory
    ('behavioral', [13, 11], 2, 3, 12, True, 0, 40),               # covariance
    ('behavioral', [37], 1, 3, 2, True, 0, 40),
    ('meancentered', [10, 12, 9], 2, 0, 6, False, 0, 40),
    ('meancentered', [10, 12, 9], 2, 0, 6, False, 1, 40),
    ('meancentered', [10, 12, 9], 2, 0, 4, False, 2, 40),
]


@pytest.mark.parametrize('method,groups,n_cond,T,m,covariance,mc,B', BUILD_CASES)
def test_builders_against_numpy(method, groups, n_cond, T, m, covariance, mc, B):
    S = sum(groups) * n_cond
    X, Y, rs = _data(method, groups, n_cond, B, T, seed=S + 7 * m + mc)
    spec = wp.spec_of(method, groups, n_cond, covariance=covariance, mean_centering=mc)
    _, V = wp.observed(spec, X, Y)
    V = np.ascontiguousarray(V[:, :m])
    n = 5
    perms = wp.random_perms(S, n, rs, identity_at=3)
    want = wp.null(spec, X, Y, perms, V)                                        # (B, m, n)
    Xf = wp.feature_matrix(spec, X)
    eng = _engine()
    try:
        _bind(eng, spec, X, Y)
        W = eng.perm_weights_build(eng.rows_tensor(perms.T), eng._dev(V, np.float64))
        eng.sync()
        W = W.cpu().numpy()
    finally:
        eng.close()
    assert W.shape == (n, m, S) and np.isfinite(W).all()
    got = np.stack([(W[p] @ Xf).T for p in range(n)], axis=-1)
    err = max_rel(got, want)
    print('{} {}x{} T={} m={} cov={} mc={}: W_p @ Xf vs oracle Z_p max err / scale {:.3e} (gate {:.0e})'.format(
        method, groups, n_cond, T, m, covariance, mc, err, NUMPY))
    assert err <= NUMPY


def test_builder_adds_repeated_rows_in_position_order_and_zeroes_skipped_ones():
    """Mean-centred PLS, index rows that are no permutation: W[l][s] = sum of (V0^T A)[l][p] over the positions p that
    hold row s; a row nobody holds gets 0.  (W_p @ Xf is then R^T V0 of X[rows].)"""
    groups, n_cond, B = [10, 12, 9], 2, 40
    S = sum(groups) * n_cond
    X, _, rs = _data('meancentered', groups, n_cond, B, 0, seed=3)
    spec = wp.spec_of('meancentered', groups, n_cond, mean_centering=0)
    _, V = wp.observed(spec, X, None)
    rows = rs.randint(S, size=(4, S))
    want = np.stack([wp.ref.gen_covcorr(spec, X[r], spec.dummy, spec.dummy).T @ V for r in rows], axis=-1)
    eng = _engine()
    try:
        _bind(eng, spec, X, None)
        W = eng.perm_weights_build(eng.rows_tensor(rows), eng._dev(V, np.float64))
        eng.sync()
        W = W.cpu().numpy()
    finally:
        eng.close()
    for r, Wr in zip(rows, W):
        assert not Wr[:, np.setdiff1d(np.arange(S), r)].any()
    got = np.stack([(Wr @ wp.feature_matrix(spec, X)).T for Wr in W], axis=-1)
    err = max_rel(got, want)
    print('repeated rows: max err / scale {:.3e}'.format(err))
    assert err <= NUMPY


# ---------------------------------------------------------------------------------------------------------------------
# the stateless test against the oracle
# ---------------------------------------------------------------------------------------------------------------------

MODES = {'correlation': ('behavioral', [50], 1, 3, False, 0), 'covariance': ('behavioral', [23, 27], 1, 2, True, 0),
         'meancentered': ('meancentered', [10, 12, 9], 2, 0, False, 0)}
M_OF = {'correlation': 3, 'covariance': 4, 'meancentered': 3}


@functools.lru_cache(maxsize=None)
def _stat_case(mode, B, n, identity_at=None):
    """Data, permutations and the oracle's answer, computed once per case and left unchanged."""
    method, groups, n_cond, T, covariance, mc = MODES[mode]
    X, Y, rs = _data(method, groups, n_cond, B, T, seed=B + n + len(mode))
    spec = wp.spec_of(method, groups, n_cond, covariance=covariance, mean_centering=mc)
    perms = wp.random_perms(X.shape[0], n, rs, identity_at=identity_at)
    want = wp.expected(spec, X, Y, perms, m=M_OF[mode])
    return spec, X, Y, perms, want


def _run_test(eng, spec, perms, want, torch, count=None):
    m = want['Z'].shape[1]
    B = want['Z'].shape[0]
    d_obs = eng._dev(want['Z'], np.float64)
    d_V = eng._dev(want['V'], np.float64)
    if count is None:
        count = torch.zeros((B, m), dtype=torch.int32, device=eng.device)
    dmax = eng._zeros((perms.shape[1], m))
    eng.perm_weights_test(eng.rows_tensor(perms.T), d_V, d_obs, count, dmax, standardise=_standardise(spec))
    eng.sync()
    return count, dmax.cpu().numpy().T


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('n', [70, 1])
@pytest.mark.parametrize('B', [150, 300])
def test_stateless_test_counts_and_maxima_against_the_oracle(B, n, mode):
    """B = 150: a partial second feature block; 300: three blocks.  n = 70: a partial second permutation tile; n = 1.
    A second call on the same counts doubles them and repeats the maxima's bits."""
    import torch
    spec, X, Y, perms, want = _stat_case(mode, B, n)
    print('{} B={} n={}: closeness of the oracle {:.3e}'.format(mode, B, n, want['closeness']))
    assert want['closeness'] >= wp.MIN_CLOSENESS
    eng = _engine()
    try:
        _bind(eng, spec, X, Y)
        count, gmax = _run_test(eng, spec, perms, want, torch)
        got_count = count.cpu().numpy()
        count2, again = _run_test(eng, spec, perms, want, torch, count=count)
        q = eng.perm_weights_scale().cpu().numpy()
    finally:
        eng.close()
    err = max_rel(gmax, want['max'])
    print('{} B={} n={}: maxima max err / scale {:.3e} (gate {:g}); counts {} .. {}'.format(
        mode, B, n, err, RTOL, got_count.min(), got_count.max()))
    assert np.array_equal(got_count, want['count'])
    assert_close(gmax, want['max'], rtol=RTOL, what='maxima')
    assert np.array_equal(count2.cpu().numpy(), 2 * want['count']) and np.array_equal(again, gmax)
    if _standardise(spec):
        assert max_rel(q, wp.feature_scale(spec, X)) <= 1e-12
    # ... and the p-values the front end forms from them
    from pypyls_amd.plsc import _weights_perm_pvals
    own = _weights_perm_pvals(wp.feature_scale(spec, X)[:, None] * np.abs(want['Z']), got_count, want['max'])
    assert np.array_equal(own['x_weights_pvals'], want['pvals'])
    assert np.array_equal(own['x_weights_pvals_fwe'], want['pvals_fwe'])


@pytest.mark.parametrize('mode', sorted(MODES))
def test_planted_identity_gives_the_observed_maximum(mode):
    """Permutation 65 of 70 (the second tile) is the identity: its maximum is max_f |Z| / s_f.  Its own comparison with
    the observed statistic is a tie up to rounding, so the counts are those of the other 69 permutations plus 0 or 1;
    closeness is asserted over those 69."""
    import torch
    B, n, at = 150, 70, 65
    spec, X, Y, perms, want = _stat_case(mode, B, n, identity_at=at)
    q = wp.feature_scale(spec, X)
    others = wp.statistics(want['Z'], np.delete(want['Zp'], at, axis=-1), q)
    print('{}: closeness of the oracle without the identity {:.3e}'.format(mode, others['closeness']))
    assert others['closeness'] >= wp.MIN_CLOSENESS
    eng = _engine()
    try:
        _bind(eng, spec, X, Y)
        count, gmax = _run_test(eng, spec, perms, want, torch)
        extra = count.cpu().numpy() - others['count']
    finally:
        eng.close()
    top = (q[:, None] * np.abs(want['Z'])).max(axis=0)
    err = max_rel(gmax[:, at], top)
    print('{}: identity maximum vs max_f |Z| / s_f: {:.3e}; ties counted {} of {}'.format(mode, err, int(extra.sum()), extra.size))
    assert err <= NUMPY
    assert np.isin(extra, (0, 1)).all()
    assert_close(np.delete(gmax, at, axis=1), others['max'], rtol=RTOL, what='maxima of the others')


@pytest.mark.parametrize('mode', ['correlation', 'meancentered'])
def test_pieces_and_feature_chunks_give_the_same_bits(mode):
    """S = 50 / 62, m = 3, B = 300, n = 12 000: a permutation's operand is 8 m S = 1200 / 1488 bytes and its maxima of one
    feature block 24.  A budget of 11 000 such permutations makes the piece 10 944 (whole 64-permutation tiles), leaves
    room for the maxima of ONE block per chunk (10 944 x 24 = 262 656 bytes; less than two are left), so the run is two
    pieces of three chunks each against one piece of one chunk."""
    import torch
    method, groups, n_cond, T, covariance, mc = MODES[mode]
    B, n, m = 300, 12000, 3
    X, Y, rs = _data(method, groups, n_cond, B, T, seed=19)
    S = X.shape[0]
    spec = wp.spec_of(method, groups, n_cond, covariance=covariance, mean_centering=mc)
    Z, V = wp.observed(spec, X, Y)
    want = dict(Z=np.ascontiguousarray(Z[:, :m]), V=np.ascontiguousarray(V[:, :m]))
    perms = wp.random_perms(S, n, rs)
    budget = 11000 * 8.0 * m * (S + 1)
    piece = int(budget // (8 * m * (S + 1))) // 64 * 64
    assert piece == 10944 and 1 <= (budget - 8 * m * S * piece) // (8 * m * piece) < 2
    runs = {}
    for name, kw in (('default', {}), ('two pieces, three chunks', dict(scratch_gb=budget / 2 ** 30))):
        eng = _engine(**kw)
        try:
            _bind(eng, spec, X, Y)
            eng.set_timing(True)
            count, gmax = _run_test(eng, spec, perms, want, torch)
            launches = eng.kernel_timing()['k_coef_prod'][1]
            eng.set_timing(False)
            runs[name] = (count.cpu().numpy(), gmax, launches)
        finally:
            eng.close()
        print('{} {}: {} timed brackets of the feature pass; counts {} .. {}'.format(
            mode, name, launches, runs[name][0].min(), runs[name][0].max()))
    one, cut = runs['default'], runs['two pieces, three chunks']
    assert cut[2] - one[2] == 5, 'the small budget did not cut the run into 2 x 3 launches'
    assert np.array_equal(one[0], cut[0]) and np.array_equal(one[1], cut[1])
    assert one[0].sum() > 0 and (one[1] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the public call
# ---------------------------------------------------------------------------------------------------------------------

def _check_public(res, want, m, n_perm, what):
    pr = res.permres
    assert pr.x_weights_pvals.shape == want['pvals'].shape and pr.x_weights_max.shape == (m, n_perm)
    print('{}: closeness of the oracle {:.3e}'.format(what, want['closeness']))
    assert want['closeness'] >= wp.MIN_CLOSENESS
    err = max_rel(pr.x_weights_max, want['max'])
    print('{}: x_weights_max max err / scale {:.3e} (gate {:g}); p in {} .. {}, fwe in {} .. {}'.format(
        what, err, RTOL, pr.x_weights_pvals.min(), pr.x_weights_pvals.max(), pr.x_weights_pvals_fwe.min(),
        pr.x_weights_pvals_fwe.max()))
    assert_close(pr.x_weights_max, want['max'], rtol=RTOL, what=what + ' x_weights_max')
    assert np.array_equal(pr.x_weights_pvals, want['pvals']), what + ' x_weights_pvals'
    assert np.array_equal(pr.x_weights_pvals_fwe, want['pvals_fwe']), what + ' x_weights_pvals_fwe'


@pytest.mark.parametrize('covariance', [False, True])
def test_public_call_behavioral_against_the_expectation(covariance):
    import pypyls_amd as pls
    groups, n_cond, B, T, n_perm = [23, 27], 1, 300, 2, 20
    X, Y, _ = _data('behavioral', groups, n_cond, B, T, seed=41 + covariance)
    kw = dict(groups=groups, n_cond=n_cond, n_perm=n_perm, n_boot=0, test_split=0, covariance=covariance, seed=7,
              verbose=False)
    res = pls.behavioral_pls(X, Y, weights_perm=True, **kw)
    assert res.inputs.weights_perm is True
    spec = wp.spec_of('behavioral', groups, n_cond, covariance=covariance)
    want = wp.expected(spec, X, Y, res.permres.permsamples)
    _check_public(res, want, 4, n_perm, 'behavioral cov={}'.format(covariance))
    assert_close(np.abs(res.x_weights * res.singvals), np.abs(want['Z']), rtol=RTOL, what='observed statistic')
    two = pls.behavioral_pls(X, Y, weights_perm=2, **kw)
    assert two.inputs.weights_perm == 2
    for key in ('x_weights_pvals', 'x_weights_pvals_fwe'):
        assert np.array_equal(two.permres[key], res.permres[key][:, :2]), key
    assert np.array_equal(two.permres.x_weights_max, res.permres.x_weights_max[:2])


def test_public_call_with_contrasts_against_the_expectation():
    import pypyls_amd as pls
    groups, n_cond, B, T, n_perm = [23, 27], 1, 300, 2, 20
    X, Y, rs = _data('behavioral', groups, n_cond, B, T, seed=43)
    C = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, 0.5], [-1.0, -0.5]])          # (T' = 4, Lc = 2), orthogonal columns
    res = pls.behavioral_pls(X, Y, groups=groups, n_perm=n_perm, n_boot=0, test_split=0, seed=8, verbose=False,
                             contrasts=C, weights_perm=True)
    spec = wp.spec_of('behavioral', groups, n_cond)
    want = wp.expected(spec, X, Y, res.permres.permsamples, contrasts=C)
    assert np.allclose(res.y_weights, want['V'], rtol=0, atol=1e-14)
    _check_public(res, want, 2, n_perm, 'contrasts')


@pytest.mark.parametrize('mean_centering', [0, 2])
def test_public_call_meancentered_against_the_expectation(mean_centering):
    """m = the live latent variables: the null-space columns of y_weights are arbitrary."""
    import pypyls_amd as pls
    groups, n_cond, B, n_perm = [10, 12, 9], 2, 300, 20
    X, _, _ = _data('meancentered', groups, n_cond, B, 0, seed=45 + mean_centering)
    spec = wp.spec_of('meancentered', groups, n_cond, mean_centering=mean_centering)
    Z, _ = wp.observed(spec, X, None)
    m = int(wp.ref.live_lvs(np.sqrt((Z ** 2).sum(axis=0))).sum())
    assert m == (3 if mean_centering == 0 else 5)
    res = pls.meancentered_pls(X, groups=groups, n_cond=n_cond, mean_centering=mean_centering, n_perm=n_perm, n_boot=0,
                               seed=9, verbose=False, weights_perm=m)
    want = wp.expected(spec, X, None, res.permres.permsamples, m=m)
    _check_public(res, want, m, n_perm, 'meancentered mc={}'.format(mean_centering))


def test_public_call_on_the_residuals_of_confounds():
    """confounds=: the keyword runs on the bound residuals -- the expectation on X, Y residualised on [1, Z - zbar]."""
    import pypyls_amd as pls
    groups, n_cond, B, T, n_perm = [50], 1, 150, 2, 20
    X, Y, rs = _data('behavioral', groups, n_cond, B, T, seed=47)
    Zc = rs.randn(50, 2)
    X, Y = X + Zc @ rs.randn(2, B), Y + Zc @ rs.randn(2, T)
    res = pls.behavioral_pls(X, Y, n_perm=n_perm, n_boot=0, test_split=0, covariance=True, seed=10, verbose=False,
                             confounds=Zc, weights_perm=True)
    Zt = np.c_[np.ones(50), Zc - Zc.mean(axis=0)]
    Xr, Yr = (A - Zt @ np.linalg.lstsq(Zt, A, rcond=None)[0] for A in (X, Y))
    want = wp.expected(wp.spec_of('behavioral', groups, covariance=True), Xr, Yr, res.permres.permsamples)
    _check_public(res, want, 2, n_perm, 'confounds')


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


NEW_KEYS = {'permres.x_weights_pvals', 'permres.x_weights_max', 'permres.x_weights_pvals_fwe'}


def test_nothing_else_moves_and_the_call_is_reproducible():
    import pypyls_amd as pls
    groups, n_cond, B, T = [13, 18], 2, 150, 3
    X, Y, _ = _data('behavioral', groups, n_cond, B, T, seed=71)
    kw = dict(groups=groups, n_cond=n_cond, n_perm=20, n_boot=30, n_split=4, test_split=5, seed=1234, verbose=False)
    off = _flatten(pls.behavioral_pls(X, Y, **kw))
    on = _flatten(pls.behavioral_pls(X, Y, weights_perm=True, **kw))
    again = _flatten(pls.behavioral_pls(X, Y, weights_perm=True, **kw))
    assert set(on) - set(off) == NEW_KEYS and set(off) <= set(on), sorted(set(on) ^ set(off))
    for key in sorted(off):
        same = np.array_equal(off[key], on[key], equal_nan=True)
        print('{}: {}'.format(key, 'same bits' if same else 'MOVED'))
        assert same, key
    for key in sorted(on):
        assert np.array_equal(on[key], again[key], equal_nan=True), key + ' differs between two runs'
    Xm, _, _ = _data('meancentered', groups, n_cond, B, 0, seed=72)
    for method_kw in (dict(mean_centering=0), dict(mean_centering=2)):
        mkw = dict(groups=groups, n_cond=n_cond, n_perm=10, n_boot=30, seed=5, verbose=False, **method_kw)
        off = _flatten(pls.meancentered_pls(Xm, **mkw))
        on = _flatten(pls.meancentered_pls(Xm, weights_perm=2, **mkw))
        assert set(on) - set(off) == NEW_KEYS
        for key in sorted(off):
            assert np.array_equal(off[key], on[key], equal_nan=True), key


def test_maxima_stay_below_the_rotated_singular_values():
    """rotate=True, L = T' = 3, correlation mode (s_f = 1): column l of Z_p has the rotated perm_singval[l, p] as its
    norm, which bounds its largest entry."""
    import pypyls_amd as pls
    X, Y, _ = _data('behavioral', [50], 1, 300, 3, seed=51)
    res = pls.behavioral_pls(X, Y, n_perm=20, n_boot=0, test_split=0, rotate=True, seed=11, verbose=False,
                             weights_perm=True)
    ratio = res.permres.x_weights_max / res.permres.perm_singval
    print('x_weights_max / perm_singval: {:.4f} .. {:.4f}'.format(ratio.min(), ratio.max()))
    assert (res.permres.x_weights_max <= res.permres.perm_singval * (1 + 1e-12)).all()
    assert (ratio > 0).all()


def test_a_team_of_two_gives_the_bits_of_one_device():
    import pypyls_amd as pls
    groups, n_cond, B, T = [23, 27], 1, 300, 2
    X, Y, _ = _data('behavioral', groups, n_cond, B, T, seed=81)
    for covariance in (False, True):
        kw = dict(groups=groups, n_cond=n_cond, n_perm=21, n_boot=0, test_split=0, covariance=covariance, seed=4,
                  verbose=False, weights_perm=True)
        one = pls.behavioral_pls(X, Y, **kw)
        team = pls.behavioral_pls(X, Y, device_ids=[0, 0], **kw)
        assert np.array_equal(one.permres.permsamples, team.permres.permsamples)
        for key in sorted(NEW_KEYS):
            key = key.split('.')[1]
            assert np.array_equal(one.permres[key], team.permres[key]), (covariance, key)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

def test_refusals_return_their_status_and_leave_the_context_usable():
    import torch
    from pypyls_amd.engine import PlsxError
    from pypyls_amd import resampling
    spec, X, Y, perms, want = _stat_case('correlation', 150, 70)
    B, m, S = 150, 3, 50
    eng = _engine()
    try:
        d_rows = eng.rows_tensor(perms.T)
        d_V, d_obs = eng._dev(want['V'], np.float64), eng._dev(want['Z'], np.float64)
        count, dmax = torch.zeros((B, m), dtype=torch.int32, device=eng.device), eng._zeros((70, m))
        W = eng._zeros((70, m, S))

        def test_rc(n=70, mm=m, rows=d_rows, V=d_V, obs=d_obs, cnt=count, mx=dmax):
            p = lambda t: None if t is None else t.data_ptr()
            return eng.lib.plsx_perm_weights_test(eng.ctx, p(rows), n, p(V), mm, p(obs), 0, p(cnt), p(mx), eng._stream())

        def build_rc(n=70, mm=m, rows=d_rows, V=d_V, out=W):
            p = lambda t: None if t is None else t.data_ptr()
            return eng.lib.plsx_perm_weights_build(eng.ctx, p(rows), n, p(V), mm, p(out), eng._stream())

        assert test_rc() == -4 and build_rc() == -4                         # nothing bound
        assert b'plsx_set_data' in eng.lib.plsx_last_error(eng.ctx)
        _bind(eng, spec, X, Y)
        for kw in (dict(n=0), dict(mm=0), dict(rows=None), dict(V=None), dict(mm=4)):
            assert test_rc(**kw) == -1 and build_rc(**kw) == -1, kw
        assert b"m = 4 outside 1 .. T' = 3" in eng.lib.plsx_last_error(eng.ctx)
        for kw in (dict(obs=None), dict(cnt=None), dict(mx=None)):
            assert test_rc(**kw) == -1, kw
        assert build_rc(out=None) == -1
        eng.sync()
        assert not bool(torch.any(count != 0).item()) and not bool(torch.any(W != 0).item())
        with pytest.raises(IndexError):
            eng.perm_weights_build(d_rows + 1, d_V)                          # an index S: refused before the device sees it
        # the context is usable
        got, gmax = _run_test(eng, spec, perms, want, torch)
        assert np.array_equal(got.cpu().numpy(), want['count'])
        # regression data: no PLS-C data bound
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), 2)
        assert test_rc() == -4 and build_rc() == -4
        assert b'not bound for PLS-C' in eng.lib.plsx_last_error(eng.ctx)
    finally:
        eng.close()
    # multiblock data: refused by both entries, the context stays usable
    eng = _engine()
    try:
        eng.set_data(X, Y, resampling.cell_of_row([25, 25], 1), 2, 1, 3)
        V8 = eng._dev(np.linalg.qr(np.random.RandomState(1).randn(eng.Tp, 2))[0], np.float64)
        with pytest.raises(PlsxError, match='status -2.*multiblock'):
            eng.perm_weights_build(eng.rows_tensor(perms.T), V8)
        count2 = torch.zeros((B, 2), dtype=torch.int32, device=eng.device)
        with pytest.raises(PlsxError, match='status -2.*multiblock'):
            eng.perm_weights_test(eng.rows_tensor(perms.T), V8, eng._zeros((B, 2)), count2, eng._zeros((70, 2)))
        _bind(eng, spec, X, Y)
        got, _ = _run_test(eng, spec, perms, want, torch)
        assert np.array_equal(got.cpu().numpy(), want['count'])
    finally:
        eng.close()
    # a budget below 64 permutations (64 x 8 m (S + 1) = 78 336 bytes): refused with the bytes named, then usable
    eng = _engine(scratch_gb=70000 / 2 ** 30)
    try:
        _bind(eng, spec, X, Y)
        count3 = torch.zeros((B, m), dtype=torch.int32, device=eng.device)
        with pytest.raises(PlsxError, match=r'status -2.*1200 bytes each.*need 78336 bytes.*70000 bytes'):
            _run_test(eng, spec, perms, want, torch, count=count3)
        assert not bool(torch.any(count3 != 0).item())
        W = eng.perm_weights_build(eng.rows_tensor(perms.T[:2]), eng._dev(want['V'], np.float64))
        eng.sync()
        assert np.isfinite(W.cpu().numpy()).all() and bool(torch.any(W != 0).item())
    finally:
        eng.close()
