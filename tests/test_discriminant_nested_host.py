"""pls_da(inner_split=ni, inner_select=), the nested cross-validation of n_components on counts: what can be checked
without a GPU -- the criterion and the selection on hand-made count blocks (the package's functions against
tests/discriminant_nested_expect.py and against values worked out by hand), the stratified draw of the inner folds and
its place in the seeded stream, validation before any engine exists, ``nested_results``, the C ABI declaration, the
ctypes signature and the records."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import discriminant_nested_expect as dn


# ---- criterion and selection ---------------------------------------------------------------------------------------

def test_criteria_on_hand_made_blocks():
    from pypyls_amd.discriminant import nested_criterion
    conf = np.array([[3, 1, 0], [2, 2, 0], [0, 0, 0]])               # class 2 has no counted row
    for f in (nested_criterion, dn.criterion):
        assert f(conf, 'accuracy') == 5 / 8
        assert f(conf, 'balanced_accuracy') == (0.0 + 3 / 4 + 2 / 4) / 2    # the absent class is left out of the mean
        assert np.isnan(f(np.zeros((3, 3), dtype=int), 'accuracy'))
        assert np.isnan(f(np.zeros((3, 3), dtype=int), 'balanced_accuracy'))
    with pytest.raises(ValueError, match=r"`rule` must be"):
        nested_criterion(conf, 'auc')
    with pytest.raises(ValueError, match=r'shape \(G, G\)'):
        nested_criterion(np.zeros((2, 3)), 'accuracy')


def test_balanced_accuracy_at_12_classes_is_the_explicit_loop():
    """Twelve recalls whose pairwise sum (np.sum at 8 or more terms) need not be the left-to-right one: the package's
    value and the expectation's are the loop's, bit for bit."""
    from pypyls_amd.discriminant import nested_criterion
    rs = np.random.RandomState(4)
    differ = 0
    for _ in range(200):
        conf = rs.randint(0, 30, size=(12, 12))
        conf[rs.randint(12)] = 0                                     # ... one class absent
        rows = conf.sum(axis=1)
        acc, present = 0.0, 0
        for g in range(12):
            if rows[g] > 0:
                acc = acc + conf[g, g] / rows[g]
                present += 1
        want = acc / present
        assert nested_criterion(conf, 'balanced_accuracy') == want == dn.balanced(conf)
        recalls = np.array([conf[g, g] / rows[g] for g in range(12) if rows[g] > 0])
        differ += int(np.sum(recalls) / present != want)
    print('blocks of 200 on which np.sum gives other bits than the loop: {}'.format(differ))


def test_selection_rule():
    from pypyls_amd.discriminant import nested_select
    nan = float('nan')
    for f in (nested_select, dn.select):
        assert f([0.5, 0.75, 0.75, 0.6]) == 2                        # a tie goes to the smaller model
        assert f([0.75, 0.75, 0.75]) == 1
        assert f([nan, 0.2, 0.9]) == 0                               # (best starts at c = 1 and a NaN is never beaten ...
        assert f([0.2, nan, 0.9]) == 3                               # ... nor does it ever win)
        assert f([nan, nan]) == 0                                    # an empty pooled block: undefined
        assert f([3.0, 2.0, 2.0, 5.0], smaller=True) == 2            # mse: the first minimum
        assert f([np.inf, np.inf], smaller=True) == 0
        assert f([0.3]) == 1
    # a NaN at c = 1 is what an empty pooled block gives at EVERY c: the total does not depend on c
    crit = [dn.criterion(np.zeros((2, 2), dtype=int), 'accuracy')] * 3
    assert nested_select(crit) == 0


def test_nested_results_against_scores_from_confusion():
    from pypyls_amd.discriminant import (nested_results, scores_from_confusion, auc_from_counts, pvals_from_null)
    rs = np.random.RandomState(2)
    n, k, G, P = 3, 4, 3, 5
    blocks = rs.randint(0, 9, size=(n, G, G)).astype(np.float64)
    blocks[1] = 0                                                    # an undefined split
    inner = rs.randint(0, 9, size=(n, k, G, G)).astype(np.float64)
    aucb = np.stack([rs.randint(0, 20, size=(n, G)), np.full((n, G), 10)], axis=-1).astype(np.float64)
    pblocks = rs.randint(0, 20, size=(P, G, G)).astype(np.float64)
    paucb = np.stack([rs.randint(0, 60, size=(P, G)), np.full((P, G), 30)], axis=-1).astype(np.float64)
    out = nested_results(blocks, inner, auc_blocks=aucb, perm_blocks=pblocks, perm_auc_blocks=paucb)
    conf = blocks.astype(np.int64).transpose(1, 2, 0)
    assert out['nested_confusion'].dtype == np.int64 and np.array_equal(out['nested_confusion'], conf)
    assert np.array_equal(out['inner_confusion'], inner.astype(np.int64).transpose(2, 3, 1, 0))
    acc, bal = scores_from_confusion(conf)
    assert np.array_equal(out['nested_accuracy'], acc, equal_nan=True) and np.isnan(out['nested_accuracy'][1])
    assert np.array_equal(out['nested_balanced_accuracy'], bal, equal_nan=True)
    eacc, ebal = dn.scores(conf)
    assert np.allclose(acc, eacc, rtol=0, atol=1e-15, equal_nan=True) and np.allclose(bal, ebal, rtol=0, atol=1e-15, equal_nan=True)
    iacc, ibal = scores_from_confusion(out['inner_confusion'])
    assert np.array_equal(out['inner_accuracy'], iacc) and np.array_equal(out['inner_balanced_accuracy'], ibal)
    assert out['inner_accuracy'].shape == (k, n)
    auc, macro = auc_from_counts(aucb.astype(np.int64).transpose(1, 2, 0))
    assert np.array_equal(out['nested_auc'], auc, equal_nan=True) and np.array_equal(out['nested_auc_macro'], macro, equal_nan=True)
    pconf = pblocks.astype(np.int64).transpose(1, 2, 0)
    pacc, pbal = scores_from_confusion(pconf)
    oacc, obal = scores_from_confusion(conf.sum(axis=-1))
    assert np.array_equal(out['perm_nested_confusion'], pconf) and np.array_equal(out['perm_nested_accuracy'], pacc)
    assert out['nested_accuracy_pvals'] == float(pvals_from_null(oacc, pacc)) == float(dn.pvals_ge(oacc, pacc))
    assert out['nested_balanced_accuracy_pvals'] == float(dn.pvals_ge(obal, pbal))
    assert out['perm_nested_auc_counts'].shape == (G, 2, P) and out['nested_auc_pvals'].shape == (G,)
    oauc, omacro = auc_from_counts(out['nested_auc_counts'].sum(axis=-1))
    assert np.array_equal(out['nested_auc_pvals'], dn.pvals_ge(oauc, out['perm_nested_auc']), equal_nan=True)
    assert out['nested_auc_macro_pvals'] == float(dn.pvals_ge(omacro, out['perm_nested_auc_macro']))
    # without AUC counts and without permutations nothing of theirs is added
    plain = nested_results(blocks, inner)
    assert sorted(plain) == sorted(['nested_confusion', 'nested_accuracy', 'nested_balanced_accuracy', 'inner_confusion',
                                    'inner_accuracy', 'inner_balanced_accuracy'])
    # a NaN observed value gives a NaN p-value
    nanres = nested_results(np.zeros((2, G, G)), inner[:2], perm_blocks=pblocks)
    assert np.isnan(nanres['nested_accuracy_pvals']) and np.isnan(nanres['nested_balanced_accuracy_pvals'])


# ---- the stratified draw of the inner folds -------------------------------------------------------------------------

@pytest.mark.parametrize('sizes, n, ni, test_size', [((20, 14, 9), 3, 4, 0.25), ((30, 6), 2, 3, 0.4)])
def test_stratified_inner_draw(sizes, n, ni, test_size):
    from pypyls_amd import resampling
    from pypyls_amd.regression import _draw_inner_codes
    rs0 = np.random.RandomState(3)
    cls = rs0.permutation(np.repeat(np.arange(len(sizes)), sizes))
    S = len(cls)
    masks = resampling.gen_stratified_splits(cls, n, seed=5, test_size=test_size)
    codes = _draw_inner_codes(masks, ni, np.random.RandomState(99), test_size, classes=cls)
    assert codes.shape == (S, n, ni) and codes.dtype == np.uint8 and set(np.unique(codes)) <= {0, 1, 2}
    # 2 exactly on the outer test rows
    assert np.array_equal(codes == 2, np.broadcast_to(~masks[:, :, None], codes.shape))
    # every class keeps ceil or floor of ITS outer training rows on every inner training side: at least one
    for s in range(n):
        for g in range(len(sizes)):
            m = int((masks[:, s] & (cls == g)).sum())
            kept = (codes[cls == g, s, :] == 1).sum(axis=0)
            print('split {} class {}: {} outer training rows, inner training rows {}'.format(s, g, m, kept))
            assert all(v in (int(np.floor(m * (1 - test_size))), int(np.ceil(m * (1 - test_size)))) for v in kept)
            assert kept.min() >= 1
    # the sequence of generator calls from a fresh RandomState: split by split, gen_stratified_splits on the class codes
    # of the training rows in ascending row order
    rs = np.random.RandomState(99)
    for s in range(n):
        rows = np.flatnonzero(masks[:, s])
        want = resampling.gen_stratified_splits(cls[rows], ni, seed=rs, test_size=test_size)
        assert np.array_equal(codes[rows, s, :] == 1, want), s
    # pls_regression's own draw is the unstratified one it was
    plain = _draw_inner_codes(masks, ni, np.random.RandomState(99), test_size)
    rs = np.random.RandomState(99)
    for s in range(n):
        rows = np.flatnonzero(masks[:, s])
        assert np.array_equal(plain[rows, s, :] == 1, resampling.gen_splits([len(rows)], 1, ni, seed=rs, test_size=test_size))


class _Captured(Exception):
    pass


def _jobs_of(monkeypatch, **kw):
    """The draw jobs of a pls_da call, captured where the draw thread would start (no device is touched)."""
    import pypyls_amd as pls
    from pypyls_amd import resampling
    got = {}

    class Capture:
        def __init__(self, rs, jobs):
            got['jobs'] = list(jobs)
            raise _Captured()
    monkeypatch.setattr(resampling, 'DrawThread', Capture)
    X, y = _data()
    with pytest.raises(_Captured):
        pls.pls_da(X, y, n_components=3, n_perm=4, n_boot=3, seed=77, verbose=False, test_split=3, cv_perm=2,
                   _engine=object(), **kw)
    return got['jobs']


def test_inner_draw_comes_last_in_the_seeded_stream(monkeypatch):
    """The call with inner_split runs the jobs of the call without it, in their order, and ONE more behind them: what a
    seeded call drew before, it draws still, and the generator stands where it stood when the inner draw begins."""
    without = _jobs_of(monkeypatch)
    with_ = _jobs_of(monkeypatch, inner_split=2, inner_select='accuracy')
    assert len(with_) == len(without) + 1
    a, b = np.random.RandomState(77), np.random.RandomState(77)
    for job in without:
        job(a)
    for job in with_[:-1]:
        job(b)
    sa, sb = a.get_state(), b.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    with_[-1](b)                                                     # the inner draw itself moves the generator on
    assert not np.array_equal(b.get_state()[1], sa[1]) or b.get_state()[2] != sa[2]


# ---- validation before any engine ---------------------------------------------------------------------------------

def _data(S=40, B=30, seed=0):
    rs = np.random.RandomState(seed)
    return rs.randn(S, B), np.arange(S) % 2


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


KW = dict(n_components=3, n_perm=0, n_boot=0, verbose=False)


def test_inner_select_refusals(no_engine):
    import pypyls_amd as pls
    X, y = _data()
    with pytest.raises(ValueError, match=r"`inner_select` must be one of \['balanced_accuracy', 'accuracy', 'mse'\]; got 'auc'"):
        pls.pls_da(X, y, test_split=4, inner_split=2, inner_select='auc', **KW)
    with pytest.raises(ValueError, match=r'`inner_select` needs `inner_split` > 0'):
        pls.pls_da(X, y, test_split=4, inner_select='accuracy', **KW)
    with pytest.raises(ValueError, match=r'`inner_select` needs `inner_split` > 0'):
        pls.pls_da(X, y, test_split=4, inner_split=0, inner_select='mse', **KW)
    # the criterion has no default: the call that was refused before the nested selection existed is refused still
    with pytest.raises(ValueError, match=r"`inner_split` is not available for pls_da without `inner_select`.*'balanced_accuracy'"):
        pls.pls_da(X, y, test_split=4, inner_split=2, **KW)
    with pytest.raises(ValueError, match=r'`inner_split` is not available for pls_da without `inner_select`'):
        pls.pls_regression(X, np.eye(2)[y], test_split=4, inner_split=2, _classes=y, **KW)


def test_what_pls_regression_refuses_is_refused(no_engine):
    import pypyls_amd as pls
    X, y = _data()
    KWS = dict(KW, inner_select='balanced_accuracy')
    with pytest.raises(ValueError, match=r'`inner_split` needs cross-validation'):
        pls.pls_da(X, y, inner_split=2, **KWS)
    for bad in (-1, 2.5, True, '3'):
        with pytest.raises(ValueError, match=r'`inner_split` must be a non-negative integer'):
            pls.pls_da(X, y, test_split=4, inner_split=bad, **KW)
    masks, inner = dn.given_folds(y, 2, 2, 1)
    with pytest.raises(ValueError, match=r'`innersamples` needs `cvsamples`'):
        pls.pls_da(X, y, test_split=2, inner_split=2, innersamples=inner, **KWS)
    with pytest.raises(ValueError, match=r'`innersamples` needs `inner_split`'):
        pls.pls_da(X, y, test_split=2, cvsamples=masks, innersamples=inner, **KW)
    with pytest.raises(ValueError, match=r'`innersamples` must have shape'):
        pls.pls_da(X, y, test_split=2, cvsamples=masks, inner_split=2, innersamples=inner[:, :, :1], **KWS)
    leak = inner.copy()
    leak[np.flatnonzero(~masks[:, 0])[0], 0, 1] = 0
    with pytest.raises(ValueError, match=r'2 exactly on the outer test rows'):
        pls.pls_da(X, y, test_split=2, cvsamples=masks, inner_split=2, innersamples=leak, **KWS)
    with pytest.raises(ValueError, match=r'`inner_split` cannot be combined with `confounds`'):
        pls.pls_da(X, y, test_split=2, inner_split=2, confounds=np.random.RandomState(1).randn(40, 2), **KWS)
    with pytest.raises(ValueError, match=r"`cv_predict='nested'` is not available for pls_da without `inner_split` > 0"):
        pls.pls_da(X, y, test_split=2, cv_predict='nested', **KW)


def test_inner_fold_without_a_class_on_its_training_side(no_engine):
    import pypyls_amd as pls
    KWS = dict(KW, inner_select='accuracy')
    X, y = _data()
    masks, inner = dn.given_folds(y, 2, 2, 1)
    bad = inner.copy()
    rows = np.flatnonzero(masks[:, 1] & (y == 1))
    bad[rows, 1, 0] = 0                                              # class 1 wholly on the test side of fold 0 of split 1
    with pytest.raises(ValueError, match=r'Every inner fold needs a usable training row of every class; inner fold 0 of '
                                         r'split 1 of `innersamples` has none of class 1'):
        pls.pls_da(X, y, test_split=2, cvsamples=masks, inner_split=2, innersamples=bad, **KWS)
    # ... a training row that is NaN throughout is no usable one
    one = inner.copy()
    one[rows[1:], 1, 0] = 0
    Xn = X.copy()
    Xn[rows[0]] = np.nan
    with pytest.raises(ValueError, match=r'inner fold 0 of split 1 of `innersamples` has none of class 1'):
        pls.pls_da(Xn, y, test_split=2, cvsamples=masks, inner_split=2, innersamples=one, **KWS)
    # drawn folds, the worst case: 4 rows of class 1 -> 3 outer training rows -> 2 inner ones; two masked rows of the
    # class can both lie there
    y2 = np.r_[np.zeros(36, dtype=int), np.ones(4, dtype=int)]
    Xm = X.copy()
    Xm[[36, 37]] = np.nan
    with pytest.raises(ValueError, match=r'Every inner fold needs a usable training row of every class; test_size = 0.25 '
                                         r'can leave class 1 \(4 rows, 2 of them NaN throughout\)'):
        pls.pls_da(Xm, y2, test_split=2, inner_split=2, **dict(KWS, n_components=2))


# ---- the C ABI, the ctypes signature, the records -------------------------------------------------------------------

def test_abi_is_declared_bound_and_recorded():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    assert re.search(r'int plsx_simpls_cvn_class_begin\(plsx_ctx\* ctx, int rule, int32_t\* d_conf, int64_t\* d_auc, '
                     r'int32_t\* d_inner_conf,\s+long long capacity\);', header)
    assert 'int plsx_simpls_cvn_class_end(plsx_ctx* ctx);' in header
    for name, val in (('MSE', 0), ('ACCURACY', 1), ('BALANCED', 2)):
        assert re.search(r'#define PLSX_CVN_SELECT_{} {}\b'.format(name, val), header)
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        eng = f.read()
    assert "'plsx_simpls_cvn_class_begin': ([vp, i32, vp, vp, vp, ctypes.c_longlong], i32)" in eng
    assert "'plsx_simpls_cvn_class_end': ([vp], i32)" in eng
    from pypyls_amd.engine import Engine
    assert Engine.CVN_RULES == {'mse': 0, 'accuracy': 1, 'balanced_accuracy': 2}
    from pypyls_amd.structures import PLSCrossValidationResults, PLSInputs
    for key in ('inner_confusion', 'inner_accuracy', 'inner_balanced_accuracy', 'nested_confusion', 'nested_accuracy',
                'nested_balanced_accuracy', 'nested_auc_counts', 'nested_auc', 'nested_auc_macro', 'perm_nested_confusion',
                'perm_nested_accuracy', 'perm_nested_balanced_accuracy', 'nested_accuracy_pvals',
                'nested_balanced_accuracy_pvals', 'perm_nested_auc_counts', 'perm_nested_auc', 'perm_nested_auc_macro',
                'nested_auc_pvals', 'nested_auc_macro_pvals'):
        assert key in PLSCrossValidationResults.allowed, key
    assert 'inner_select' in PLSInputs.allowed


def test_expectation_on_a_case_counted_by_hand():
    """Two classes, one outer split, two inner folds, k = 2, the expectation's pooling and selection against
    da_expected called fold by fold."""
    import discriminant_expect as de
    X, y, _ = __import__('discriminant_auc_expect').design(40, 12, (22, 18), 5)
    masks, inner = dn.given_folds(y, 1, 2, 9)
    codes = np.concatenate([masks[:, :, None].astype(np.uint8), inner], axis=2)
    out = dn.nested_da_expected(X, y, codes, 2, 'accuracy')
    pooled = np.zeros((2, 2, 2), dtype=np.int64)
    for j in (1, 2):
        Xm = X.copy()
        Xm[codes[:, 0, j] == 2] = np.nan
        pooled += de.da_expected(Xm, y, (codes[:, 0, j] == 1)[:, None], 2)['confusion'][:, :, :, 0]
    assert np.array_equal(out['inner_confusion'][:, :, :, 0], pooled)
    assert pooled[:, :, 0].sum() == (inner[:, 0, :] == 0).sum()       # every inner test row is counted once per c
    crit = [np.trace(pooled[:, :, c]) / pooled[:, :, c].sum() for c in range(2)]
    assert out['crit'][:, 0].tolist() == crit
    c = 2 if crit[1] > crit[0] else 1
    assert out['ncomp'][0] == c
    full = de.da_expected(X, y, masks, 2)['confusion']
    assert np.array_equal(out['confusion'][:, :, 0], full[:, :, c - 1, 0])
