"""pls_da(auc=True) on the device (plsx_simpls_cv_auc_begin / _end, k_sd_cv_auc): the C ABI against the oracle on the
reference fixtures and at the kernel's edges, ties, the permuted route across solver batches and calls, the rules of the
series, and the public call.

The comparison is EXACT integer equality of counts.  What makes that a fair demand is asserted next to every such
comparison: the oracle's pair margin -- the smallest gap between the predictions of any counted pair of opposite
membership -- is at least PAIR_MARGIN = 1e-7, three orders above the ~1e-10 at which the device's predictions agree with
the oracle's."""
import numpy as np
import pytest

from conftest import load_golden
from discriminant_auc_expect import (EDGE_IDS, EDGES, PAIR_MARGIN, auc_expected, auc_of, auc_perm_expected, design,
                                     edge_case)
from discriminant_expect import MARGIN, da_expected, da_perm_expected, one_hot

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, -1, -4
AUC_KEYS = ('auc_counts', 'auc', 'auc_macro', 'perm_auc_counts', 'perm_auc', 'perm_auc_macro', 'auc_pvals',
            'auc_macro_pvals')


def _bind(eng, X, codes, k, G=None):
    """The one-hot Y centred as the front-end centres it; rows of X that are NaN throughout go in as zeros behind the
    row masks."""
    Y = one_hot(codes, G)
    Yc = Y - Y.mean(axis=0)
    okx = ~np.isnan(X).all(axis=1)
    Xc = np.nan_to_num(X - np.nanmean(X, axis=0))
    eng.set_data_regression(Xc, Yc, k)
    if not okx.all():
        eng.simpls_set_row_masks(okx, np.ones(len(X), dtype=bool))
    return Y.shape[1]


def _observed(eng, masks, k, G, auc=True, conf=False):
    """plsx_simpls_crossval_batch on masks (S, n): (r, r2, sse, counts (G, 2, k, n) or None, confusion (G, G, k, n) or
    None)."""
    import torch
    n = masks.shape[1]
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    out = [eng._zeros((n, k, G)), eng._zeros((n, k, G)), eng._zeros((n, k + 1, G))]
    d_auc = d_conf = None
    if conf:
        d_conf = torch.full((n, k, G, G), -7, dtype=torch.int32, device=eng.device)               # (the library zeroes)
        eng.simpls_cv_class_begin(d_conf)
    if auc:
        d_auc = torch.full((n, k, G, 2), -7, dtype=torch.int64, device=eng.device)
        eng.simpls_cv_auc_begin(d_auc)
    eng.simpls_crossval_into(dm, *out)
    if auc:
        eng.simpls_cv_auc_end()
    if conf:
        eng.simpls_cv_class_end()
    eng.sync()
    return [t.cpu().numpy() for t in out] + [None if d_auc is None else d_auc.cpu().numpy().transpose(2, 3, 1, 0),
                                             None if d_conf is None else d_conf.cpu().numpy().transpose(2, 3, 1, 0)]


def _assert_counts(got, want, what):
    assert want['margin'] >= PAIR_MARGIN, (what, want['margin'])
    differ = int(np.sum(got != want['counts']))
    print('{}: oracle pair margin {:.3e}; {} of {} counts differ; {} pairs at c = 1'
          .format(what, want['margin'], differ, want['counts'].size, int(want['counts'][:, 1, 0].sum())))
    assert got.shape == want['counts'].shape and got.dtype == np.int64 and differ == 0, what


# ---- 1. C ABI, observed labels

@pytest.mark.parametrize('tag', ['a', 'b', 'nan'])
def test_abi_goldens(tag):
    from pypyls_amd.engine import Engine
    g = load_golden('simpls_da_' + tag)
    k, masks = int(g['n_components']), g['cvsamples']
    eng = Engine()
    try:
        G = _bind(eng, g['X'], g['y'], k)
        plain = _observed(eng, masks, k, G, auc=False)
        eng.simpls_set_classes(g['y'])
        conf_alone = _observed(eng, masks, k, G, auc=False, conf=True)[4]
        r, r2, sse, counts, _ = _observed(eng, masks, k, G)
        both = _observed(eng, masks, k, G, conf=True)
    finally:
        eng.close()
    want = auc_expected(g['X'], g['y'], masks, k)
    _assert_counts(counts, want, 'simpls_da_{} vs oracle'.format(tag))
    _assert_counts(both[3], want, 'simpls_da_{} vs oracle, both series open'.format(tag))
    for name, a, b in (('r', r, plain[0]), ('r2', r2, plain[1]), ('sse', sse, plain[2])):
        assert np.array_equal(a, b, equal_nan=True), 'd_{} changed its bits with the series open'.format(name)
    for name, a, b in (('r', both[0], plain[0]), ('r2', both[1], plain[1]), ('sse', both[2], plain[2])):
        assert np.array_equal(a, b, equal_nan=True), 'd_{} changed its bits with both series open'.format(name)
    assert np.array_equal(both[4], conf_alone) and np.array_equal(conf_alone, g['ref_confusion'])
    auc, macro = auc_of(want['counts'].sum(axis=-1))
    print('simpls_da_{}: pooled AUC per class at c = k {}; macro {:.3f}'.format(tag, np.round(auc[:, -1], 3).tolist(), macro[-1]))


# ---- 2. kernel edges

@pytest.mark.parametrize('gl', [0, 1], ids=['onchip', 'global'])
@pytest.mark.parametrize('S,sizes,k,nan_x', EDGES, ids=EDGE_IDS)
def test_kernel_edges(S, sizes, k, nan_x, gl):
    from pypyls_amd.engine import Engine
    X, y, masks = edge_case(S, sizes, k, nan_x)
    assert not (~masks[:, 0] & (y == 0)).any() and (~masks[:, 1] & (y == 0)).any()
    want = auc_expected(X, y, masks, k)
    assert np.all(want['counts'][0, :, :, 0] == 0) and np.all(want['counts'][0, 1, :, 1] > 0)   # the class split 0 does not test
    assert np.isnan(auc_of(want['counts'])[0][0, :, 0]).all()
    eng = Engine(options={'simpls_global': gl})
    try:
        G = _bind(eng, X, y, k)
        eng.simpls_set_classes(y)
        counts = _observed(eng, masks, k, G)[3]
    finally:
        eng.close()
    _assert_counts(counts, want, 'S={} G={} k={} simpls_global={}'.format(S, G, k, gl))


def _wide_case():
    """S = 300, G = 3 of sizes 200 / 60 / 40, 135 test rows per split: more than 64 listed positions, not a multiple of
    64, and about 90 positives of class 0 -- a second round of the lanes that own the positives, with a tail.  The seed
    was chosen on the CPU: the oracle's pair margin holds (asserted where the case is used)."""
    X, y, rs = design(300, 48, (200, 60, 40), 503)
    masks = np.ones((300, 3), dtype=bool)
    for s in range(3):
        masks[rs.choice(300, size=135, replace=False), s] = False
    return X, y, masks


def test_more_than_64_test_rows():
    from pypyls_amd.engine import Engine
    X, y, masks = _wide_case()
    n_pos0 = (~masks & (y == 0)[:, None]).sum(axis=0)
    assert n_pos0.min() > 64 and (n_pos0 % 64 != 0).all() and ((~masks).sum(axis=0) == 135).all()
    want = auc_expected(X, y, masks, 2)
    eng = Engine()
    try:
        G = _bind(eng, X, y, 2)
        eng.simpls_set_classes(y)
        counts = _observed(eng, masks, 2, G)[3]
    finally:
        eng.close()
    _assert_counts(counts, want, 'S=300 G=3 k=2, 135 test rows')


def test_one_usable_test_row():
    """Split 0 tests one row (a positive of its class and nobody's negative: no pair anywhere), split 1 tests two rows
    of different classes (one pair per class), split 2 tests two rows of one class and a row that is NaN throughout."""
    from pypyls_amd.engine import Engine
    X, y, rs = design(40, 30, (15, 13, 12), 4, nan_x=(7,))
    rows = [np.flatnonzero((y == g) & (np.arange(40) != 7)) for g in range(3)]
    masks = np.ones((40, 3), dtype=bool)
    masks[rows[1][0], 0] = False
    masks[[rows[0][0], rows[2][0]], 1] = False
    masks[[rows[1][1], rows[1][2], 7], 2] = False
    want = auc_expected(X, y, masks, 3)
    assert np.all(want['counts'][:, :, :, 0] == 0) and np.all(want['counts'][:, :, :, 2] == 0)
    assert np.all(want['counts'][:, 1, :, 1] == [[1], [0], [1]])
    eng = Engine()
    try:
        G = _bind(eng, X, y, 3)
        eng.simpls_set_classes(y)
        counts = _observed(eng, masks, 3, G)[3]
    finally:
        eng.close()
    _assert_counts(counts, want, 'one, two and two-of-one-class usable test rows')


# ---- 3. ties

def test_identical_rows_of_different_classes_tie():
    """Two test rows of X that are identical and of different classes: every one of their predictions ties, so the pair
    adds 1 to u2 of either class, not 0 or 2.  This rests on the supposition that identical rows get bit-identical
    predictions on the device (the same columns of K, the same sums in the same order); the oracle calls a gap of at
    most 1e-12 a tie, and the margin is asserted over the remaining pairs."""
    from pypyls_amd.engine import Engine
    X, y, masks = edge_case(*EDGES[1])
    k = EDGES[1][2]
    te = np.flatnonzero(~masks[:, 1] & ~np.isnan(X).all(axis=1))
    i, j = te[y[te] == 0][0], te[y[te] == 1][0]
    X = X.copy()
    X[j] = X[i]
    want = auc_expected(X, y, masks, k, tie_tol=1e-12)
    strict = auc_expected(X, y, masks, k)
    # the oracle itself sees the tie, or a gap far below what it can resolve: with the tolerance u2 is what exact
    # arithmetic gives
    assert strict['margin'] < 1e-12 or np.array_equal(strict['counts'], want['counts'])
    both = ~masks[i] & ~masks[j]
    assert both.sum() >= 1 and np.all(want['counts'][:2, 0][:, :, both] % 2 == 1)       # one tie: an odd u2 of classes 0 and 1
    eng = Engine()
    try:
        G = _bind(eng, X, y, k)
        eng.simpls_set_classes(y)
        counts = _observed(eng, masks, k, G)[3]
    finally:
        eng.close()
    _assert_counts(counts, want, 'S=65 G=3 k=4 with rows {} and {} identical'.format(i, j))


# ---- 4. C ABI, permuted labels

def _permuted(eng, masks, perms, k, G, calls=None, auc=True):
    """plsx_simpls_crossval_perm_batch on perms (S, P) under masks (S, n), in one call or in `calls` pieces:
    (r, r2, mse, counts (G, 2, k, P) or None)."""
    import torch
    P = perms.shape[1]
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    di = eng.rows_tensor(perms.T)
    out = [eng._zeros((P, k, G)), eng._zeros((P, k, G)), eng._zeros((P, k + 1))]
    d_auc = None
    if auc:
        d_auc = torch.full((P, k, G, 2), -7, dtype=torch.int64, device=eng.device)
        eng.simpls_cv_auc_begin(d_auc)
    a = 0
    for m in (calls or [P]):
        eng.simpls_crossval_perm_into(dm, di[a:a + m].contiguous(), *(t[a:a + m] for t in out))
        a += m
    if auc:
        eng.simpls_cv_auc_end()
    eng.sync()
    return [t.cpu().numpy() for t in out] + [None if d_auc is None else d_auc.cpu().numpy().transpose(2, 3, 1, 0)]


@pytest.fixture(scope='module')
def perm_case():
    g = load_golden('simpls_da_a')
    k, masks = int(g['n_components']), g['cvsamples'][:, :4]
    rs = np.random.RandomState(71)
    perms = np.stack([rs.permutation(len(g['y'])) for _ in range(6)], axis=1)
    return g['X'], g['y'], masks, perms, k, auc_perm_expected(g['X'], g['y'], masks, k, perms)


def test_abi_permuted(perm_case):
    """6 permutations x 4 splits of golden a.  Half of a 0.001 GB budget takes 13 fits (39.6 KB each): the batches are
    13 + 11 and permutation 3 (fits 12 .. 15) straddles them -- its block takes the counts of two launches."""
    from pypyls_amd.engine import Engine
    X, y, masks, perms, k, want = perm_case
    got, batches = {}, {}
    for name, kw, calls in (('one call', {}, None), ('0.001 GB', dict(scratch_gb=0.001), None), ('3 + 3', {}, [3, 3])):
        eng = Engine(**kw)
        try:
            G = _bind(eng, X, y, k)
            eng.simpls_set_classes(y)
            eng.set_timing(True)
            got[name] = _permuted(eng, masks, perms, k, G, calls)
            batches[name] = eng.kernel_timing()['k_sd_cv_auc'][1]
        finally:
            eng.close()
        print('{}: {} launches of k_sd_cv_auc'.format(name, batches[name]))
        _assert_counts(got[name][3], want, 'golden a, 6 permutations x 4 splits, {}'.format(name))
    assert batches == {'one call': 1, '0.001 GB': 2, '3 + 3': 2}
    # the regression scores keep their bits with the series open
    eng = Engine()
    try:
        G = _bind(eng, X, y, k)
        plain = _permuted(eng, masks, perms, k, G, auc=False)
    finally:
        eng.close()
    for name, a, b in zip(('r', 'r2', 'mse'), got['one call'][:3], plain[:3]):
        assert np.array_equal(a, b, equal_nan=True), 'd_{} changed its bits with the series open'.format(name)


# ---- 5. series rules

def test_series_rules():
    import torch
    from pypyls_amd.engine import Engine
    g = load_golden('simpls_da_b')
    k, masks = int(g['n_components']), g['cvsamples']
    eng = Engine()
    try:
        G = _bind(eng, g['X'], g['y'], k)
        cnt = torch.full((3, k, G, 2), -7, dtype=torch.int64, device=eng.device)
        assert eng.lib.plsx_simpls_cv_auc_begin(eng.ctx, cnt.data_ptr(), 3) == ERR_STATE         # before set_classes
        eng.simpls_set_classes(g['y'])
        assert eng.lib.plsx_simpls_cv_auc_begin(eng.ctx, None, 3) == ERR_ARG
        assert eng.lib.plsx_simpls_cv_auc_begin(eng.ctx, cnt.data_ptr(), 0) == ERR_ARG
        # capacity 3, a call of 8 splits: refused before anything is computed -- the outputs and both buffers keep what
        # they held, also those of a confusion series that WOULD have room
        conf = torch.full((8, k, G, G), -7, dtype=torch.int32, device=eng.device)
        eng.simpls_cv_class_begin(conf)
        eng.simpls_cv_auc_begin(cnt)
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        out = [torch.full(s, 3.5, dtype=torch.float64, device=eng.device) for s in ((8, k, G), (8, k, G), (8, k + 1, G))]
        rc = eng.lib.plsx_simpls_crossval_batch(eng.ctx, dm.data_ptr(), 8, *(t.data_ptr() for t in out), eng._stream())
        msg = eng.lib.plsx_last_error(eng.ctx).decode()
        print('status {}: {}'.format(rc, msg))
        eng.sync()
        assert rc == ERR_ARG and 'plsx_simpls_cv_auc_begin' in msg
        assert all(bool((t == 3.5).all().item()) for t in out)
        assert bool((cnt == -7).all().item()) and bool((conf == -7).all().item())
        di = eng.rows_tensor(np.stack([np.random.RandomState(s).permutation(len(g['y'])) for s in range(4)]))
        pout = [torch.full(s, 3.5, dtype=torch.float64, device=eng.device) for s in ((4, k, G), (4, k, G), (4, k + 1))]
        rc = eng.lib.plsx_simpls_crossval_perm_batch(eng.ctx, dm.data_ptr(), 8, di.data_ptr(), 4,
                                                     *(t.data_ptr() for t in pout), eng._stream())
        eng.sync()
        assert rc == ERR_ARG and all(bool((t == 3.5).all().item()) for t in pout)
        assert bool((cnt == -7).all().item()) and bool((conf == -7).all().item())
        eng.simpls_cv_class_end()                                  # (independent: the AUC series stays open)
        # two calls of 2 + 1 splits fill the three blocks in submission order; a fourth split does not fit
        want = auc_expected(g['X'], g['y'], masks[:, :3], k)
        o3 = [eng._zeros((3, k, G)), eng._zeros((3, k, G)), eng._zeros((3, k + 1, G))]
        eng.simpls_crossval_into(dm[:2].contiguous(), *(t[:2] for t in o3))
        eng.simpls_crossval_into(dm[2:3].contiguous(), *(t[2:3] for t in o3))
        rc = eng.lib.plsx_simpls_crossval_batch(eng.ctx, dm[3:4].contiguous().data_ptr(), 1,
                                                *(t.data_ptr() for t in o3), eng._stream())
        eng.sync()
        assert rc == ERR_ARG
        _assert_counts(cnt.cpu().numpy().transpose(2, 3, 1, 0), want, 'golden b, 2 + 1 splits in one series')
        assert bool((conf == -7).all().item())                     # (the closed confusion series counted nothing)
        # plsx_set_data ends the series and clears the classes: the next call counts nothing, _begin needs set_classes
        _bind(eng, g['X'], g['y'], k)
        cnt.fill_(-7)
        eng.simpls_crossval_into(dm[:3].contiguous(), *o3)
        eng.sync()
        assert bool((cnt == -7).all().item())
        assert eng.lib.plsx_simpls_cv_auc_begin(eng.ctx, cnt.data_ptr(), 3) == ERR_STATE
        # ... and so does plsx_simpls_set_classes
        eng.simpls_set_classes(g['y'])
        eng.simpls_cv_auc_begin(cnt)
        eng.simpls_set_classes(g['y'])
        eng.simpls_crossval_into(dm[:3].contiguous(), *o3)
        eng.sync()
        assert bool((cnt == -7).all().item())
        # ... and _end, and a second _begin (the first buffer stays as it was)
        eng.simpls_cv_auc_begin(cnt)
        eng.simpls_cv_auc_end()
        eng.simpls_crossval_into(dm[:3].contiguous(), *o3)
        other = torch.full((3, k, G, 2), -7, dtype=torch.int64, device=eng.device)
        eng.simpls_cv_auc_begin(cnt)
        eng.simpls_cv_auc_begin(other)
        eng.simpls_crossval_into(dm[:3].contiguous(), *o3)
        eng.simpls_cv_auc_end()
        eng.sync()
        assert bool((cnt == -7).all().item())
        _assert_counts(other.cpu().numpy().transpose(2, 3, 1, 0), want, 'golden b, the second series')
    finally:
        eng.close()


# ---- 6. the public call

def _flat(res, skip=('inputs',)):
    out = {}
    for key, val in res.items():
        if key in skip:
            continue
        if isinstance(val, dict):
            for k2, v2 in val.items():
                out[key + '.' + k2] = v2
        else:
            out[key] = val
    return out


@pytest.fixture(scope='module')
def public_case(perm_case):
    import pypyls_amd as pls
    X, y, masks, perms, k, want_perm = perm_case
    kw = dict(n_components=k, n_perm=8, n_boot=10, test_split=4, cvsamples=masks, cv_perm=6, cvpermsamples=perms,
              coef_components=3, vip_components=3, seed=4242, verbose=False)
    return X, y, masks, perms, k, kw, want_perm, auc_expected(X, y, masks, k), pls.pls_da(X, y, auc=True, **kw)


def test_public_call_equals_the_expectation(public_case):
    import pypyls_amd as pls
    X, y, masks, perms, k, kw, want_perm, want, res = public_case
    cv = res.cvres
    _assert_counts(cv.auc_counts, want, 'pls_da(auc=True) on golden a, observed')
    _assert_counts(cv.perm_auc_counts, want_perm, 'pls_da(auc=True) on golden a, permuted')
    auc, macro = auc_of(want['counts'])
    assert np.array_equal(cv.auc, auc, equal_nan=True) and cv.auc.shape == (3, k, 4)
    assert np.allclose(cv.auc_macro, macro, rtol=0, atol=1e-15) and cv.auc_macro.shape == (k, 4)
    pauc, pmacro = auc_of(want_perm['counts'])
    assert np.array_equal(cv.perm_auc, pauc, equal_nan=True) and cv.perm_auc.shape == (3, k, 6)
    assert np.allclose(cv.perm_auc_macro, pmacro, rtol=0, atol=1e-15) and cv.perm_auc_macro.shape == (k, 6)
    for got, fn in ((cv.auc, cv.auc_macro), (cv.perm_auc, cv.perm_auc_macro)):
        a, m = pls.auc_from_counts(cv.auc_counts if got is cv.auc else cv.perm_auc_counts)
        assert np.array_equal(got, a, equal_nan=True) and np.array_equal(fn, m, equal_nan=True)
    oauc, omacro = pls.auc_from_counts(want['counts'].sum(axis=-1))
    assert np.array_equal(cv.auc_pvals, (np.sum(cv.perm_auc >= oauc[..., None], axis=-1) + 1) / 7)
    assert np.array_equal(cv.auc_macro_pvals, (np.sum(cv.perm_auc_macro >= omacro[:, None], axis=-1) + 1) / 7)
    assert cv.auc_pvals.shape == (3, k) and cv.auc_macro_pvals.shape == (k,)
    print('pooled macro AUC per c {}; p-values {}'.format(np.round(omacro, 3).tolist(), cv.auc_macro_pvals.tolist()))
    # the confusion counts of the same call are the ones the expectation gives
    cw = da_expected(X, y, masks, k)
    assert cw['margin'] >= MARGIN and np.array_equal(cv.confusion, cw['confusion'])
    assert np.array_equal(cv.perm_confusion, da_perm_expected(X, y, masks, k, perms)['confusion'])


def test_public_call_keeps_the_bits_of_the_call_without_auc(public_case):
    import pypyls_amd as pls
    X, y, masks, perms, k, kw, want_perm, want, res = public_case
    base = pls.pls_da(X, y, **kw)
    fa, fb = _flat(base), _flat(res)
    assert set(fb) - set(fa) == {'cvres.' + key for key in AUC_KEYS} and not set(fa) - set(fb)
    for key, val in fa.items():
        if val is None:
            assert fb[key] is None, key
        else:
            assert np.array_equal(np.asarray(val), np.asarray(fb[key]), equal_nan=True), key
    print('{} arrays of pls_da(...) are bit-identical in the pls_da(..., auc=True) result'.format(len(fa)))
    assert base.inputs.get('_auc') is None and res.inputs.get('_auc') is True


def test_seeded_call_repeats():
    import pypyls_amd as pls
    g = load_golden('simpls_da_nan')
    X, y, k = g['X'], g['y'], int(g['n_components'])
    kw = dict(n_components=k, n_perm=4, n_boot=0, test_split=6, test_size=0.25, cv_perm=5, seed=77, verbose=False, auc=True)
    one, two = pls.pls_da(X, y, **kw), pls.pls_da(X, y, **kw)
    fa, fb = _flat(one), _flat(two)
    assert set(fa) == set(fb) and {'cvres.' + key for key in AUC_KEYS} <= set(fa)
    for key, val in fa.items():
        if val is not None:
            assert np.array_equal(np.asarray(val), np.asarray(fb[key]), equal_nan=True), key
    masks = one.cvres.cvsamples
    _assert_counts(one.cvres.auc_counts, auc_expected(X, y, masks, k), 'simpls_da_nan, drawn stratified splits')
    _assert_counts(one.cvres.perm_auc_counts, auc_perm_expected(X, y, masks, k, one.cvres.cvpermsamples),
                   'simpls_da_nan, drawn permutations')


def test_two_contexts_on_one_device_give_identical_counts(public_case, monkeypatch):
    import pypyls_amd as pls
    from pypyls_amd import team as _team
    X, y, masks, perms, k, kw, want_perm, want, res = public_case
    calls = []
    orig = _team.Team.allgather

    def counting(self, rank, flat):
        calls.append(rank)
        return orig(self, rank, flat)
    monkeypatch.setattr(_team.Team, 'allgather', counting)
    team = pls.pls_da(X, y, device_ids=[0, 0], auc=True, **kw)
    print('all-gather calls per rank: {}'.format(sorted(calls)))
    assert sorted(calls) == [0, 1]                           # ONE collective carries the counts too
    for key in AUC_KEYS:
        assert np.array_equal(team.cvres[key], res.cvres[key], equal_nan=True), key


def test_round_trip(public_case, tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    X, y, masks, perms, k, kw, want_perm, want, res = public_case
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    back = pls.load_results(pls.save_results(str(tmp_path / 'da_auc'), res))
    for key in AUC_KEYS:
        assert np.array_equal(back.cvres[key], res.cvres[key], equal_nan=True), key
        assert back.cvres[key].shape == res.cvres[key].shape, key
    assert np.issubdtype(back.cvres.auc_counts.dtype, np.integer)
