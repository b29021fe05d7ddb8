"""pls_da on the device (plsx_simpls_set_classes, plsx_simpls_cv_class_begin / _end, k_sd_cv_class): the C ABI against
the reference fixtures and the oracle at the kernel's edges, the permuted route across solver batches and calls, the rules
of the series, and the public call.

The comparison is EXACT integer equality of confusion counts.  What makes that a fair demand is asserted next to every
such comparison: the oracle's margin -- the smallest gap between the two largest predicted indicators of any counted
row -- is at least 1e-6, four orders above the ~1e-10 at which the device's predictions agree with the oracle's."""
import numpy as np
import pytest

from conftest import load_golden
from discriminant_expect import MARGIN, da_expected, da_perm_expected, one_hot

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 0, -1, -2, -4


def _design(S, B, sizes, seed, shift=0.6, nan_x=()):
    """Class means shifted on a tenth of the features; rows in random order."""
    rs = np.random.RandomState(seed)
    y = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    X = rs.randn(S, B)
    nf = max(2, B // 10)
    X[:, :nf] += (shift * rs.randn(len(sizes), nf))[y]
    for i in nan_x:
        X[i] = np.nan
    return X, y, rs


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


def _observed(eng, masks, k, G, series=True, capacity=None):
    """plsx_simpls_crossval_batch on masks (S, n): (r, r2, sse, conf (G, G, k, n) or None)."""
    import torch
    n = masks.shape[1]
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    out = [eng._zeros((n, k, G)), eng._zeros((n, k, G)), eng._zeros((n, k + 1, G))]
    conf = None
    if series:
        conf = torch.full((capacity or n, k, G, G), -7, dtype=torch.int32, device=eng.device)   # (the library zeroes)
        eng.simpls_cv_class_begin(conf)
    eng.simpls_crossval_into(dm, *out)
    if series:
        eng.simpls_cv_class_end()
    eng.sync()
    out = [t.cpu().numpy() for t in out]
    return out + [None if conf is None else conf.cpu().numpy()[:n].transpose(2, 3, 1, 0)]


def _assert_counts(got, want, what):
    assert want['margin'] >= MARGIN, (what, want['margin'])
    differ = int(np.sum(got != want['confusion']))
    print('{}: oracle margin {:.3e}; {} of {} cells differ; {} rows counted'
          .format(what, want['margin'], differ, want['confusion'].size, int(want['confusion'][:, :, 0].sum())))
    assert got.shape == want['confusion'].shape and differ == 0, what


# ---- 1. C ABI, observed labels

@pytest.mark.parametrize('tag', ['a', 'b', 'nan'])
def test_abi_goldens(tag):
    from pypyls_amd.engine import Engine
    g = load_golden('simpls_da_' + tag)
    k, masks = int(g['n_components']), g['cvsamples']
    eng = Engine()
    try:
        G = _bind(eng, g['X'], g['y'], k)
        plain = _observed(eng, masks, k, G, series=False)
        eng.simpls_set_classes(g['y'])
        r, r2, sse, conf = _observed(eng, masks, k, G)
    finally:
        eng.close()
    want = da_expected(g['X'], g['y'], masks, k)
    _assert_counts(conf, want, 'simpls_da_{} vs oracle'.format(tag))
    assert np.array_equal(conf, g['ref_confusion']) and float(g['ref_margin']) >= MARGIN
    for name, a, b in (('r', r, plain[0]), ('r2', r2, plain[1]), ('sse', sse, plain[2])):
        assert np.array_equal(a, b, equal_nan=True), 'd_{} changed its bits with the series open'.format(name)


# ---- 2. kernel edges

EDGES = [  # S, sizes, k, nan rows: lane-stride tails (63, 65, 130), the scorer's four-at-a-time boundary (k = 1, 4, 5),
           # the accumulator bounds (G = 2, 3 -> 4; 17 -> 32; 32 -> 32)
    (63, (33, 30), 1, (5,)),
    (65, (25, 22, 18), 4, (0, 64)),
    (130, tuple([8] * 14 + [6] * 3), 5, (17, 99)),
    (130, tuple([5] * 2 + [4] * 30), 5, (3,)),
]


def _edge_case(S, sizes, k, nan_x, seed=0):
    """5 splits: the second block of four waves has three idle ones.  Split 0's test side lacks class 0 altogether."""
    X, y, rs = _design(S, 48, sizes, 1000 + S + len(sizes) + seed, nan_x=nan_x)
    masks = np.ones((S, 5), dtype=bool)
    for s in range(5):
        for g in range(len(sizes)):
            rows = np.flatnonzero(y == g)
            if s == 0 and g == 0:
                continue
            masks[rs.choice(rows, size=max(1, int(round(len(rows) * 0.3))), replace=False), s] = False
    return X, y, masks


@pytest.mark.parametrize('gl', [0, 1], ids=['onchip', 'global'])
@pytest.mark.parametrize('S,sizes,k,nan_x', EDGES, ids=['S63-G2-k1', 'S65-G3-k4', 'S130-G17-k5', 'S130-G32-k5'])
def test_kernel_edges(S, sizes, k, nan_x, gl):
    from pypyls_amd.engine import Engine
    X, y, masks = _edge_case(S, sizes, k, nan_x)
    assert not (~masks[:, 0] & (y == 0)).any() and (~masks[:, 1] & (y == 0)).any()
    want = da_expected(X, y, masks, k)
    assert want['confusion'][0, :, :, 0].sum() == 0           # the class that split 0 does not test
    eng = Engine(options={'simpls_global': gl})
    try:
        G = _bind(eng, X, y, k)
        eng.simpls_set_classes(y)
        conf = _observed(eng, masks, k, G)[3]
    finally:
        eng.close()
    _assert_counts(conf, want, 'S={} G={} k={} simpls_global={}'.format(S, G, k, gl))


def test_more_than_32_classes_is_unsupported_and_the_context_lives():
    import torch
    from pypyls_amd.engine import Engine
    X, y, rs = _design(132, 40, tuple([4] * 33), 9)
    eng = Engine()
    try:
        G = _bind(eng, X, y, 3)
        dev = torch.from_numpy(y.astype(np.int32)).to(eng.device)
        rc = eng.lib.plsx_simpls_set_classes(eng.ctx, dev.data_ptr(), 33, eng._stream())
        msg = eng.lib.plsx_last_error(eng.ctx).decode()
        print('status {}: {}'.format(rc, msg))
        assert rc == ERR_UNSUPPORTED and '32' in msg
        conf = torch.zeros((2, 3, 33, 33), dtype=torch.int32, device=eng.device)
        assert eng.lib.plsx_simpls_cv_class_begin(eng.ctx, conf.data_ptr(), 2) == ERR_STATE       # nothing was bound
        masks = np.ones((132, 2), dtype=bool)
        masks[::4] = False
        r, r2, sse, _ = _observed(eng, masks, 3, G, series=False)                                # still usable
        assert np.isfinite(sse).all()
    finally:
        eng.close()


def test_set_classes_refusals():
    import torch
    from pypyls_amd.engine import Engine, PLSX_BEHAVIORAL
    X, y, rs = _design(40, 30, (15, 13, 12), 4)
    eng = Engine()
    try:
        dev = torch.from_numpy(y.astype(np.int32)).to(eng.device)

        def call(ptr, G):
            rc = eng.lib.plsx_simpls_set_classes(eng.ctx, ptr, G, eng._stream())
            print('status {}: {}'.format(rc, eng.lib.plsx_last_error(eng.ctx).decode()))
            return rc
        assert call(dev.data_ptr(), 3) == ERR_STATE                          # no data bound
        eng.set_data(X, one_hot(y), np.zeros(40, np.int32), 1, 1, PLSX_BEHAVIORAL)
        assert call(dev.data_ptr(), 3) == ERR_STATE                          # ... not for regression
        _bind(eng, X, y, 3)
        assert call(dev.data_ptr(), 4) == ERR_ARG                            # G != T
        bad = dev.clone()
        bad[11] = 3
        assert call(bad.data_ptr(), 3) == ERR_ARG                            # a code outside 0 .. G - 1
        bad[11] = -1
        assert call(bad.data_ptr(), 3) == ERR_ARG
        assert call(dev.data_ptr(), 3) == OK
        assert call(None, 0) == OK                                           # a null pointer clears the binding
        conf = torch.zeros((2, 3, 3, 3), dtype=torch.int32, device=eng.device)
        assert eng.lib.plsx_simpls_cv_class_begin(eng.ctx, conf.data_ptr(), 2) == ERR_STATE
    finally:
        eng.close()


# ---- 3. C ABI, permuted labels

def _permuted(eng, masks, perms, k, G, calls=None):
    """plsx_simpls_crossval_perm_batch on perms (S, P) under masks (S, n), in one call or in `calls` pieces:
    (r, r2, mse, conf (G, G, k, P))."""
    import torch
    P = perms.shape[1]
    dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
    di = eng.rows_tensor(perms.T)
    out = [eng._zeros((P, k, G)), eng._zeros((P, k, G)), eng._zeros((P, k + 1))]
    conf = torch.full((P, k, G, G), -7, dtype=torch.int32, device=eng.device)
    eng.simpls_cv_class_begin(conf)
    a = 0
    for m in (calls or [P]):
        eng.simpls_crossval_perm_into(dm, di[a:a + m].contiguous(), *(t[a:a + m] for t in out))
        a += m
    eng.simpls_cv_class_end()
    eng.sync()
    return [t.cpu().numpy() for t in out] + [conf.cpu().numpy().transpose(2, 3, 1, 0)]


@pytest.fixture(scope='module')
def perm_case():
    g = load_golden('simpls_da_a')
    k, masks = int(g['n_components']), g['cvsamples'][:, :4]
    rs = np.random.RandomState(71)
    perms = np.stack([rs.permutation(len(g['y'])) for _ in range(6)], axis=1)
    return g['X'], g['y'], masks, perms, k, da_perm_expected(g['X'], g['y'], masks, k, perms)


def test_abi_permuted(perm_case):
    """6 permutations x 4 splits of golden a: a fit holds 3751 doubles of solver state, 8640 bytes of dual weights and
    scores, 450 of sources and mask and 464 of scores -- 39.6 KB.  Half of a 0.001 GB budget takes 13 of them: the
    batches are 13 + 11 and permutation 3 (fits 12 .. 15) straddles them."""
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
            batches[name] = eng.kernel_timing()['k_sd_cv_class'][1]
        finally:
            eng.close()
        print('{}: {} launches of k_sd_cv_class'.format(name, batches[name]))
        _assert_counts(got[name][3], want, 'golden a, 6 permutations x 4 splits, {}'.format(name))
    assert batches == {'one call': 1, '0.001 GB': 2, '3 + 3': 2}
    # the regression scores keep their bits with the series open
    eng = Engine()
    try:
        import torch
        G = _bind(eng, X, y, k)
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        plain = [eng._zeros((6, k, G)), eng._zeros((6, k, G)), eng._zeros((6, k + 1))]
        eng.simpls_crossval_perm_into(dm, eng.rows_tensor(perms.T), *plain)
        eng.sync()
        plain = [t.cpu().numpy() for t in plain]
    finally:
        eng.close()
    for name, a, b in zip(('r', 'r2', 'mse'), got['one call'][:3], plain):
        assert np.array_equal(a, b, equal_nan=True), 'd_{} changed its bits with the series open'.format(name)


# ---- 4. series rules

def test_series_rules():
    import torch
    from pypyls_amd.engine import Engine
    g = load_golden('simpls_da_b')
    k, masks = int(g['n_components']), g['cvsamples']
    eng = Engine()
    try:
        G = _bind(eng, g['X'], g['y'], k)
        conf = torch.full((3, k, G, G), -7, dtype=torch.int32, device=eng.device)
        assert eng.lib.plsx_simpls_cv_class_begin(eng.ctx, conf.data_ptr(), 3) == ERR_STATE      # before set_classes
        eng.simpls_set_classes(g['y'])
        assert eng.lib.plsx_simpls_cv_class_begin(eng.ctx, None, 3) == ERR_ARG
        assert eng.lib.plsx_simpls_cv_class_begin(eng.ctx, conf.data_ptr(), 0) == ERR_ARG
        # capacity 3, a call of 8 splits: refused before anything is computed -- the outputs keep what they held
        eng.simpls_cv_class_begin(conf)
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        out = [torch.full(s, 3.5, dtype=torch.float64, device=eng.device) for s in ((8, k, G), (8, k, G), (8, k + 1, G))]
        rc = eng.lib.plsx_simpls_crossval_batch(eng.ctx, dm.data_ptr(), 8, *(t.data_ptr() for t in out), eng._stream())
        msg = eng.lib.plsx_last_error(eng.ctx).decode()
        print('status {}: {}'.format(rc, msg))
        eng.sync()
        assert rc == ERR_ARG and 'plsx_simpls_cv_class_begin' in msg
        assert all(bool((t == 3.5).all().item()) for t in out) and bool((conf == -7).all().item())
        di = eng.rows_tensor(np.stack([np.random.RandomState(s).permutation(len(g['y'])) for s in range(4)]))
        pout = [torch.full(s, 3.5, dtype=torch.float64, device=eng.device) for s in ((4, k, G), (4, k, G), (4, k + 1))]
        rc = eng.lib.plsx_simpls_crossval_perm_batch(eng.ctx, dm.data_ptr(), 8, di.data_ptr(), 4,
                                                     *(t.data_ptr() for t in pout), eng._stream())
        eng.sync()
        assert rc == ERR_ARG and all(bool((t == 3.5).all().item()) for t in pout) and bool((conf == -7).all().item())
        # two calls of 2 + 1 splits fill the three blocks in submission order; a fourth split does not fit
        want = da_expected(g['X'], g['y'], masks[:, :3], k)
        o3 = [eng._zeros((3, k, G)), eng._zeros((3, k, G)), eng._zeros((3, k + 1, G))]
        eng.simpls_crossval_into(dm[:2].contiguous(), *(t[:2] for t in o3))
        eng.simpls_crossval_into(dm[2:3].contiguous(), *(t[2:3] for t in o3))
        rc = eng.lib.plsx_simpls_crossval_batch(eng.ctx, dm[3:4].contiguous().data_ptr(), 1,
                                                *(t.data_ptr() for t in o3), eng._stream())
        eng.sync()
        assert rc == ERR_ARG
        _assert_counts(conf.cpu().numpy().transpose(2, 3, 1, 0), want, 'golden b, 2 + 1 splits in one series')
        # plsx_set_data ends the series and clears the classes: the next call counts nothing, _begin needs set_classes
        _bind(eng, g['X'], g['y'], k)
        conf.fill_(-7)
        eng.simpls_crossval_into(dm[:3].contiguous(), *o3)
        eng.sync()
        assert bool((conf == -7).all().item())
        assert eng.lib.plsx_simpls_cv_class_begin(eng.ctx, conf.data_ptr(), 3) == ERR_STATE
        # ... and so does plsx_simpls_set_classes
        eng.simpls_set_classes(g['y'])
        eng.simpls_cv_class_begin(conf)
        eng.simpls_set_classes(g['y'])
        eng.simpls_crossval_into(dm[:3].contiguous(), *o3)
        eng.sync()
        assert bool((conf == -7).all().item())
    finally:
        eng.close()


# ---- 5. the public call

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


DA_KEYS = ('confusion', 'accuracy', 'balanced_accuracy', 'perm_confusion', 'perm_accuracy', 'perm_balanced_accuracy',
           'accuracy_pvals', 'balanced_accuracy_pvals')


@pytest.fixture(scope='module')
def public_case(perm_case):
    import pypyls_amd as pls
    X, y, masks, perms, k, want_perm = perm_case
    kw = dict(n_components=k, n_perm=8, n_boot=10, test_split=4, cvsamples=masks, cv_perm=6, cvpermsamples=perms,
              coef_components=3, vip_components=3, seed=4242, verbose=False)
    return X, y, masks, perms, k, kw, want_perm, da_expected(X, y, masks, k), pls.pls_da(X, y, **kw)


def test_public_call_equals_the_expectation(public_case):
    import pypyls_amd as pls
    X, y, masks, perms, k, kw, want_perm, want, res = public_case
    cv = res.cvres
    assert np.array_equal(res.classes, [0, 1, 2])
    _assert_counts(cv.confusion, want, 'pls_da on golden a, observed')
    _assert_counts(cv.perm_confusion, want_perm, 'pls_da on golden a, permuted')
    assert np.array_equal(cv.confusion, load_golden('simpls_da_a')['ref_confusion'][..., :4])
    assert np.issubdtype(cv.confusion.dtype, np.integer) and np.issubdtype(cv.perm_confusion.dtype, np.integer)
    acc, bal = pls.scores_from_confusion(want['confusion'])
    assert np.array_equal(cv.accuracy, acc) and np.array_equal(cv.balanced_accuracy, bal) and acc.shape == (k, 4)
    pacc, pbal = pls.scores_from_confusion(want_perm['confusion'])
    assert np.array_equal(cv.perm_accuracy, pacc) and np.array_equal(cv.perm_balanced_accuracy, pbal)
    oacc, obal = pls.scores_from_confusion(want['confusion'].sum(axis=-1))
    assert np.array_equal(cv.accuracy_pvals, (np.sum(pacc >= oacc[:, None], axis=1) + 1) / 7)
    assert np.array_equal(cv.balanced_accuracy_pvals, (np.sum(pbal >= obal[:, None], axis=1) + 1) / 7)
    print('accuracy per c (pooled) {}; p-values {}'.format(np.round(oacc, 3).tolist(), cv.accuracy_pvals.tolist()))


def test_public_call_keeps_the_bits_of_pls_regression(public_case):
    import pypyls_amd as pls
    X, y, masks, perms, k, kw, want_perm, want, res = public_case
    reg = pls.pls_regression(X, one_hot(y), **kw)
    fa, fb = _flat(reg), _flat(res)
    assert set(fb) - set(fa) == {'classes'} | {'cvres.' + key for key in DA_KEYS}
    for key, val in fa.items():
        if val is None:
            assert fb[key] is None, key
        else:
            assert np.array_equal(np.asarray(val), np.asarray(fb[key]), equal_nan=True), key
    print('{} arrays of pls_regression(X, onehot) are bit-identical in the pls_da result'.format(len(fa)))
    for key in ('n_perm', 'n_boot', 'n_components', 'seed', 'test_split', 'test_size', 'coef_components', 'cv_perm'):
        assert res.inputs.get(key) == reg.inputs.get(key), key
    assert np.array_equal(res.inputs.Y, one_hot(y))


def test_seeded_call_repeats_and_draws_stratified_splits():
    import pypyls_amd as pls
    from pypyls_amd import resampling as rsmp
    g = load_golden('simpls_da_nan')
    X, y, k = g['X'], g['y'], int(g['n_components'])
    kw = dict(n_components=k, n_perm=4, n_boot=0, test_split=6, test_size=0.25, cv_perm=5, seed=77, verbose=False)
    one, two = pls.pls_da(X, y, **kw), pls.pls_da(X, y, **kw)
    fa, fb = _flat(one), _flat(two)
    assert set(fa) == set(fb)
    for key, val in fa.items():
        if val is not None:
            assert np.array_equal(np.asarray(val), np.asarray(fb[key]), equal_nan=True), key
    masks = one.cvres.cvsamples
    for cls, n_g in enumerate(np.bincount(y)):
        kept = masks[y == cls].sum(axis=0)
        assert set(kept.tolist()) <= {int(np.floor(n_g * 0.75)), int(np.ceil(n_g * 0.75))}, (cls, kept)
    # the draw sits where pls_regression draws its own: behind the SVD seeds and the permutations of the call
    rstate = np.random.RandomState(77)
    for _ in range(k):
        rstate.normal(size=(min(X.shape[1], 4), 11))
    assert np.array_equal(one.permres.permsamples, rsmp.gen_permsamp([len(y)], 1, 4, seed=rstate, verbose=False))
    assert np.array_equal(masks, rsmp.gen_stratified_splits(y, 6, seed=rstate, test_size=0.25))
    assert np.array_equal(one.cvres.cvpermsamples, rsmp.gen_permsamp([len(y)], 1, 5, seed=rstate, verbose=False))
    want = da_expected(X, y, masks, k)
    _assert_counts(one.cvres.confusion, want, 'simpls_da_nan, drawn stratified splits')
    want_perm = da_perm_expected(X, y, masks, k, one.cvres.cvpermsamples)
    _assert_counts(one.cvres.perm_confusion, want_perm, 'simpls_da_nan, drawn permutations')


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
    team = pls.pls_da(X, y, device_ids=[0, 0], **kw)
    print('all-gather calls per rank: {}'.format(sorted(calls)))
    assert sorted(calls) == [0, 1]                           # ONE collective carries the counts too
    for key in DA_KEYS:
        assert np.array_equal(team.cvres[key], res.cvres[key]), key


def test_round_trip_predict_class_and_string_labels(public_case, tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    X, y, masks, perms, k, kw, want_perm, want, res = public_case
    want_cls = res.classes[np.argmax(pls.predict(res, X), axis=1)]
    got_cls = pls.predict_class(res, X)
    assert np.array_equal(got_cls, want_cls) and got_cls.shape == (len(y),)
    print('training accuracy of the 3-component model: {:.3f}'.format(float(np.mean(got_cls == y))))
    assert np.mean(got_cls == y) > 0.5
    names = np.array(['ctl', 'pat', 'sib'])
    named = pls.pls_da(X, names[y], **dict(kw, n_perm=0, n_boot=0))
    assert np.array_equal(named.classes, names)
    for key in DA_KEYS:
        assert np.array_equal(named.cvres[key], res.cvres[key]), key
    assert np.array_equal(pls.predict_class(named, X), names[want_cls])
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    back = pls.load_results(pls.save_results(str(tmp_path / 'da'), res))
    assert np.array_equal(back.classes, res.classes)
    for key in DA_KEYS:
        assert np.array_equal(back.cvres[key], res.cvres[key]) and back.cvres[key].shape == res.cvres[key].shape, key
    assert np.array_equal(pls.predict_class(back, X), got_cls)
