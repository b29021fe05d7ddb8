"""pls_da(inner_split=ni, inner_select=) on the device (plsx_simpls_cvn_class_begin riding the nested entries:
k_sd_cv_class / k_sd_cv_auc per fit into the batch's scratch, k_sd_cvn_class_select, k_sd_cvn_class_reduce) against the
oracle (tests/discriminant_nested_expect.py), the plain pls_da call, solver batches, a team, persistence and the
refusals of the series.

Counts, selected component counts and p-values are compared EXACTLY.  What keeps that honest is asserted on the
oracle's own numbers before any device number is looked at: the argmax margin of every fit, inner ones included
(discriminant_expect.MARGIN), the pair margin of the AUC counts (discriminant_auc_expect.PAIR_MARGIN) and, for the
'mse' rule, the selection gap of tests/test_gpu_regression_nested.py (GAP, ten times its bar).  The two count criteria
are functions of integers and need no gap.  r, R^2, mse and inner_mse at that file's tolerance, RTOL = 1e-5 absolute
on r, relative to max(1, |value|) elsewhere.

Shapes: B = 40, k = 4, 3 outer splits x 2 or 3 inner folds, 3 permutations of which the first is the identity; G = 2
and 3 (the <4> instantiations of the counting kernels, S = 60), G = 5 (<16>, S = 90, class sizes 40 .. 8) and G = 17
(<32>, S = 170).  The seeds were chosen on the CPU so that the conditions of _oracle() hold; they are asserted."""
import functools

import numpy as np
import pytest

import discriminant_auc_expect as ae
import discriminant_expect as de
import discriminant_nested_expect as dn
import regression_nested_expect as ne

pytestmark = pytest.mark.gpu
RTOL = 1e-5
GAP = 1e-4
# scores_from_confusion / auc_from_counts against the expectation's left-to-right loops on the SAME integers: at most 17
# terms of at most 1 each, whose partial sums stay below 32 (an ulp of 3.6e-15) and are divided by their number
SUMS = 1e-14
B, K, N, P = 40, 4, 3, 3
# S, class sizes, inner folds, rows of X that are NaN throughout, seed
CASES = {'G2': (60, (34, 26), 2, (), 4), 'G3': (60, (25, 20, 15), 3, (7, 41), 0),
         'G5': (90, (40, 20, 12, 10, 8), 2, (), 3), 'G17': (170, tuple([10] * 17), 2, (5,), 2)}
COUNTS = ('nested_confusion', 'inner_confusion', 'nested_auc_counts', 'perm_nested_confusion', 'perm_nested_auc_counts',
          'nested_ncomp', 'perm_nested_ncomp')
SCORES = ('nested_accuracy', 'nested_balanced_accuracy', 'inner_accuracy', 'inner_balanced_accuracy', 'nested_auc',
          'nested_auc_macro', 'perm_nested_accuracy', 'perm_nested_balanced_accuracy', 'perm_nested_auc',
          'perm_nested_auc_macro', 'nested_accuracy_pvals', 'nested_balanced_accuracy_pvals', 'nested_auc_pvals',
          'nested_auc_macro_pvals')
REGRESSION = ('nested_pearson_r', 'nested_r_squared', 'nested_mse', 'inner_mse', 'perm_nested_pearson_r',
              'perm_nested_r_squared', 'perm_nested_mse', 'nested_pearson_r_pvals', 'nested_r_squared_pvals',
              'nested_mse_pvals')
PLAIN = ('confusion', 'accuracy', 'balanced_accuracy', 'auc_counts', 'auc', 'auc_macro', 'perm_confusion',
         'perm_auc_counts', 'accuracy_pvals', 'auc_pvals', 'pearson_r_ncomp', 'r_squared_ncomp', 'mse', 'perm_pearson_r',
         'perm_mse', 'mse_pvals')


@functools.lru_cache(maxsize=None)
def _case(name):
    S, sizes, ni, nan_x, seed = CASES[name]
    X, y, rs = ae.design(S, B, sizes, seed, nan_x=nan_x)
    masks, inner = dn.given_folds(y, N, ni, seed + 100)
    perms = np.stack([np.arange(S)] + [rs.permutation(S) for _ in range(P - 1)], axis=1)
    codes = np.concatenate([masks[:, :, None].astype(np.uint8), inner], axis=2)
    return X, y, masks, inner, perms, codes


@functools.lru_cache(maxsize=None)
def _oracle(name, rule):
    """The oracle on the case's folds and permutations; margins, gap and the conditions on the input asserted HERE."""
    X, y, masks, inner, perms, codes = _case(name)
    obs = dn.nested_da_expected(X, y, codes, K, rule, auc=True)
    nul = dn.nested_da_perm_expected(X, y, codes, K, perms, rule, auc=True)
    margin, pair = min(obs['margin'], nul['margin']), min(obs['pair_margin'], nul['pair_margin'])
    print('{} {}: oracle argmax margin {:.3e}, pair margin {:.3e}; ncomp {}; per permutation {}'
          .format(name, rule, margin, pair, obs['ncomp'], nul['choice'].T.tolist()))
    assert margin >= de.MARGIN and pair >= ae.PAIR_MARGIN, (name, rule, margin, pair)
    if rule == 'mse':
        gap = ne.selection_gap(obs['inner_mse'], nul['inner_mse'])
        print('{} mse: oracle selection gap {:.3e}'.format(name, gap))
        assert gap >= GAP, (name, gap)
    assert (obs['ncomp'] >= 1).all() and (nul['choice'] >= 1).all()           # (no undefined group in these designs)
    if rule != 'mse':
        # a kernel that always answers c = 1 must not pass: the choice varies over the splits and under a permutation
        assert len(set(obs['ncomp'].tolist())) >= 2, (name, rule, obs['ncomp'])
        assert any(not np.array_equal(nul['choice'][:, p], obs['ncomp']) for p in range(1, P)), (name, rule)
    return obs, nul


def _kw(name, rule, **more):
    X, y, masks, inner, perms, codes = _case(name)
    kw = dict(n_components=K, n_perm=0, n_boot=0, verbose=False, test_split=N, cvsamples=masks, inner_split=inner.shape[2],
              innersamples=inner, inner_select=rule, cv_perm=P, cvpermsamples=perms, auc=True)
    kw.update(more)
    return kw


@functools.lru_cache(maxsize=None)
def _run(name, rule):
    import pypyls_amd as pls
    X, y = _case(name)[:2]
    return pls.pls_da(X, y, **_kw(name, rule, cv_predict='nested'))


def _close(got, want, rel, where=None):
    """NaN in the same places; elsewhere |got - want| (rel: / max(1, |want|)) -> the largest.  where: the entries that
    are compared at all."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    if where is not None:
        got, want = got[where], want[where]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    d = np.abs(got[ok] - want[ok])
    return float(np.max(d / np.maximum(1.0, np.abs(want[ok])) if rel else d))


def _scored(name):
    """(G, P) bool: the indicator column of class g varies on the usable test side of EVERY outer split under permutation
    p.  Where it does not -- a permutation can leave a class of 10 rows off a test side of 51 -- Pearson r and R^2 of that
    column are 0 / 0 on that split, on the oracle and on the device alike, and their split means say nothing: such
    entries of the null's r and R^2 are not compared (the observed folds are stratified: every class is on every test
    side; mse and every count are defined throughout and compared throughout)."""
    X, y, masks, inner, perms, codes = _case(name)
    G = len(CASES[name][1])
    usable = ~np.isnan(X).all(axis=1)
    out = np.ones((G, P), dtype=bool)
    for p in range(P):
        true = y[perms[:, p]]
        for s in range(N):
            te = true[~masks[:, s] & usable]
            for g in range(G):
                out[g, p] &= 0 < int((te == g).sum()) < len(te)
    return out


def _same_bits(a, b, what, keys):
    for key in keys:
        same = np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True)
        print('{}: {} bit-identical: {}'.format(what, key, same))
        assert same, (what, key)


@pytest.mark.parametrize('rule', dn.RULES)
@pytest.mark.parametrize('name', list(CASES))
def test_against_the_oracle(name, rule):
    from pypyls_amd.discriminant import roc_curve
    X, y, masks, inner, perms, codes = _case(name)
    obs, nul = _oracle(name, rule)
    cv = _run(name, rule).cvres
    G = len(CASES[name][1])
    print('{} {}: nested_ncomp {} expected {}; perm_nested_ncomp\n{}'.format(name, rule, cv['nested_ncomp'], obs['ncomp'],
                                                                            cv['perm_nested_ncomp']))
    # ---- the observed call: integers exactly
    assert np.array_equal(cv['nested_ncomp'], obs['ncomp'])
    assert cv['inner_confusion'].shape == (G, G, K, N) and np.array_equal(cv['inner_confusion'], obs['inner_confusion'])
    assert cv['nested_confusion'].shape == (G, G, N) and np.array_equal(cv['nested_confusion'], obs['confusion'])
    assert cv['nested_auc_counts'].shape == (G, 2, N) and np.array_equal(cv['nested_auc_counts'], obs['auc_counts'])
    assert np.array_equal(cv['innersamples'], inner)
    # ... consistent with the plain cross-validation of the same call: the selected column of its counts
    for s in range(N):
        c = int(cv['nested_ncomp'][s])
        assert np.array_equal(cv['nested_confusion'][:, :, s], cv['confusion'][:, :, c - 1, s]), s
        assert np.array_equal(cv['nested_auc_counts'][:, :, s], cv['auc_counts'][:, :, c - 1, s]), s
    acc, bal = dn.scores(obs['confusion'])
    iacc, ibal = dn.scores(obs['inner_confusion'])
    auc, macro = ae.auc_of(obs['auc_counts'])
    for key, want in (('nested_accuracy', acc), ('nested_balanced_accuracy', bal), ('inner_accuracy', iacc),
                      ('inner_balanced_accuracy', ibal), ('nested_auc', auc), ('nested_auc_macro', macro)):
        err = _close(cv[key], want, False)
        print('{} {}: {} max err {:.3e}'.format(name, rule, key, err))
        assert err <= SUMS, key
    # ... the criterion the device selected by is the one of the pooled counts it returned
    if rule != 'mse':
        for s in range(N):
            crit = [dn.criterion(cv['inner_confusion'][:, :, c, s], rule) for c in range(K)]
            assert dn.select(crit) == cv['nested_ncomp'][s] and crit == obs['crit'][:, s].tolist()
    errs = dict(r=_close(cv['nested_pearson_r'], obs['r'], False), r2=_close(cv['nested_r_squared'], obs['r2'], True),
                mse=_close(cv['nested_mse'], obs['mse'], True), inner=_close(cv['inner_mse'], obs['inner_mse'], True))
    print('{} {}: max err of nested r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}  inner_mse {inner:.3e}'.format(name, rule, **errs))
    assert max(errs.values()) <= RTOL, errs
    # ---- cv_predict='nested': the predictions of the selected model recount its confusion, their ROC area is its AUC
    assert np.array_equal(cv['y_pred_ncomp'], obs['ncomp'])
    pred = cv['predicted']
    for s in range(N):
        conf = np.zeros((G, G), dtype=np.int64)
        rows = np.flatnonzero(pred[:, s] >= 0)
        np.add.at(conf, (y[rows], pred[rows, s]), 1)
        assert np.array_equal(conf, cv['nested_confusion'][:, :, s]), s
        assert np.array_equal(pred[:, s] >= 0, ~masks[:, s] & ~np.isnan(X).all(axis=1))
    res = _run(name, rule)
    worst = 0.0
    for g in range(G):
        for s in range(N):
            fpr, tpr, _ = roc_curve(res, res.classes[g], s)
            area = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2))
            if np.isnan(cv['nested_auc'][g, s]):
                continue
            worst = max(worst, abs(area - cv['nested_auc'][g, s]))
    print('{} {}: largest |ROC area - nested_auc| {:.3e}'.format(name, rule, worst))
    assert worst <= 1e-12
    # ---- the null: the whole procedure per permutation
    assert cv['perm_nested_confusion'].shape == (G, G, P) and np.array_equal(cv['perm_nested_confusion'], nul['confusion'])
    assert cv['perm_nested_auc_counts'].shape == (G, 2, P) and np.array_equal(cv['perm_nested_auc_counts'], nul['auc_counts'])
    assert np.array_equal(cv['perm_nested_ncomp'], nul['ncomp']) and (cv['perm_nested_ncomp'].sum(axis=0) == N).all()
    # the identity permutation is column 0: its sums are the observed ones
    assert np.array_equal(cv['perm_nested_confusion'][:, :, 0], cv['nested_confusion'].sum(axis=-1))
    assert np.array_equal(cv['perm_nested_auc_counts'][:, :, 0], cv['nested_auc_counts'].sum(axis=-1))
    for c in range(1, K + 1):
        assert cv['perm_nested_ncomp'][c - 1, 0] == int((cv['nested_ncomp'] == c).sum())
    pacc, pbal = dn.scores(nul['confusion'])
    pauc, pmacro = ae.auc_of(nul['auc_counts'])
    oacc, obal = dn.scores(obs['confusion'].sum(axis=-1))
    oauc, omacro = ae.auc_of(obs['auc_counts'].sum(axis=-1))
    for key, want in (('perm_nested_accuracy', pacc), ('perm_nested_balanced_accuracy', pbal), ('perm_nested_auc', pauc),
                      ('perm_nested_auc_macro', pmacro)):
        assert _close(cv[key], want, False) <= SUMS, key
    # the p-values: both sides by the package's own functionals of the ORACLE's integers, as the issue defines them (the
    # identity permutation ties with the observed value exactly, so the two sides must round alike)
    from pypyls_amd.discriminant import auc_from_counts, scores_from_confusion
    sacc, sbal = scores_from_confusion(obs['confusion'].sum(axis=-1))
    nacc, nbal = scores_from_confusion(nul['confusion'])
    sauc, smacro = auc_from_counts(obs['auc_counts'].sum(axis=-1))
    nauc, nmacro = auc_from_counts(nul['auc_counts'])
    assert _close(sacc, oacc, False) <= SUMS and _close(sbal, obal, False) <= SUMS and _close(sauc, oauc, False) <= SUMS
    for key, want in (('nested_accuracy_pvals', dn.pvals_ge(sacc, nacc)),
                      ('nested_balanced_accuracy_pvals', dn.pvals_ge(sbal, nbal)),
                      ('nested_auc_pvals', dn.pvals_ge(sauc, nauc)),
                      ('nested_auc_macro_pvals', dn.pvals_ge(smacro, nmacro))):
        print('{} {}: {} {} expected {}'.format(name, rule, key, cv[key], want))
        assert np.array_equal(np.asarray(cv[key], dtype=float), np.asarray(want, dtype=float), equal_nan=True), key
    assert np.ndim(cv['nested_accuracy_pvals']) == 0 and np.shape(cv['nested_auc_pvals']) == (G,)
    scored = _scored(name)
    assert scored[:, 0].all() and scored.mean() > 0.8, scored
    errs = dict(r=_close(cv['perm_nested_pearson_r'], nul['r'], False, scored),
                r2=_close(cv['perm_nested_r_squared'], nul['r2'], True, scored),
                mse=_close(cv['perm_nested_mse'], nul['mse'], True))
    print('{} {}: max err of the nested null r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}'.format(name, rule, **errs))
    assert max(errs.values()) <= RTOL, errs


def test_accuracy_and_balanced_accuracy_choose_differently_under_imbalance():
    """Class sizes 40, 20, 12, 10, 8: on at least one split the two count criteria select another model, on the oracle
    and on the device alike."""
    a, b = _oracle('G5', 'accuracy')[0]['ncomp'], _oracle('G5', 'balanced_accuracy')[0]['ncomp']
    print('oracle: accuracy chooses {}, balanced accuracy {}'.format(a, b))
    assert not np.array_equal(a, b)
    da, db = _run('G5', 'accuracy').cvres, _run('G5', 'balanced_accuracy').cvres
    assert np.array_equal(da['nested_ncomp'], a) and np.array_equal(db['nested_ncomp'], b)
    # the pooled counts do not depend on the rule, the selected blocks do
    assert np.array_equal(da['inner_confusion'], db['inner_confusion'])
    assert not np.array_equal(da['nested_confusion'], db['nested_confusion'])
    # ... and the 'mse' rule selects exactly what pls_regression's nested call selects on the same indicators
    import pypyls_amd as pls
    X, y, masks, inner, perms, codes = _case('G5')
    kw = _kw('G5', 'mse')
    for key in ('inner_select', 'auc'):
        kw.pop(key)
    reg = pls.pls_regression(X, de.one_hot(y), **kw).cvres
    _same_bits(_run('G5', 'mse').cvres, reg, "inner_select='mse' vs pls_regression", ('nested_ncomp', 'perm_nested_ncomp') + REGRESSION)


def test_inner_split_0_and_the_keys_of_the_plain_call_keep_their_bits():
    import pypyls_amd as pls
    X, y, masks, inner, perms, codes = _case('G3')
    kw = _kw('G3', 'balanced_accuracy')
    for key in ('inner_split', 'innersamples', 'inner_select'):
        kw.pop(key)
    plain = pls.pls_da(X, y, **kw)
    zero = pls.pls_da(X, y, inner_split=0, **kw)
    assert sorted(plain.cvres.keys()) == sorted(zero.cvres.keys())
    assert not any(key.startswith(('nested_', 'inner', 'perm_nested')) for key in zero.cvres.keys())
    assert zero.inputs.get('inner_split') is None and zero.inputs.get('inner_select') is None
    _same_bits(plain.cvres, zero.cvres, 'inner_split=0 vs no keyword', tuple(plain.cvres.keys()))
    for key in ('x_weights', 'y_loadings', 'varexp'):
        assert np.array_equal(plain[key], zero[key]), key
    # ... and what the plain call returns, the nested call returns beside its own keys, bit for bit
    _same_bits(plain.cvres, _run('G3', 'balanced_accuracy').cvres, 'plain keys of the nested call', PLAIN)


def test_drawn_folds_are_stratified_and_equal_the_given_ones():
    import pypyls_amd as pls
    X, y = _case('G3')[:2]
    kw = dict(n_components=K, n_perm=0, n_boot=0, verbose=False, test_split=N, inner_split=2, cv_perm=P, auc=True, seed=31,
              inner_select='balanced_accuracy')
    drawn = pls.pls_da(X, y, **kw)
    cv = drawn.cvres
    inner, masks = cv['innersamples'], cv['cvsamples']
    assert inner.shape == (len(y), N, 2) and inner.dtype == np.uint8
    assert np.array_equal(inner == 2, np.broadcast_to(~masks[:, :, None], inner.shape))
    usable = ~np.isnan(X).all(axis=1)
    for g in range(3):
        assert ((inner[(y == g) & usable] == 1).sum(axis=0) >= 1).all() and ((inner[y == g] == 0).sum(axis=0) >= 1).all()
    assert drawn.inputs.inner_select == 'balanced_accuracy'
    # the seeded call without the keyword draws what it drew: the same outer splits and permutations
    plain = pls.pls_da(X, y, **{key: v for key, v in kw.items() if key not in ('inner_split', 'inner_select')})
    assert np.array_equal(plain.cvres.cvsamples, masks) and np.array_equal(plain.cvres.cvpermsamples, cv['cvpermsamples'])
    given = pls.pls_da(X, y, cvsamples=masks, innersamples=inner, cvpermsamples=cv['cvpermsamples'],
                       **{key: v for key, v in kw.items() if key != 'seed'})
    _same_bits(cv, given.cvres, 'drawn vs given folds', COUNTS + SCORES + REGRESSION)
    # ... and against the oracle on the drawn folds, where its margins allow the exact comparison
    codes = np.concatenate([masks[:, :, None].astype(np.uint8), inner], axis=2)
    obs = dn.nested_da_expected(X, y, codes, K, 'balanced_accuracy', auc=True)
    print('drawn folds: oracle margin {:.3e}, pair margin {:.3e}, ncomp {}'.format(obs['margin'], obs['pair_margin'], obs['ncomp']))
    assert obs['margin'] >= de.MARGIN and obs['pair_margin'] >= ae.PAIR_MARGIN
    assert np.array_equal(cv['nested_ncomp'], obs['ncomp']) and np.array_equal(cv['nested_confusion'], obs['confusion'])
    assert np.array_equal(cv['inner_confusion'], obs['inner_confusion']) and np.array_equal(cv['nested_auc_counts'], obs['auc_counts'])


def test_solver_batches_do_not_change_the_bits():
    """3 outer x 2 inner x 5 permutations at S = 1000, G = 6 (the <16> instantiations), k = 5: 15 groups of 3 fits of
    about half a megabyte each, their count blocks included.  Half of a 0.02 GB budget takes at most 7 whole groups, so
    the groups go in three batches and permutations straddle them; the default budget takes all in one.  A series too
    small for the call is refused before anything is computed and the context works afterwards."""
    import torch
    import pypyls_amd as pls
    from pypyls_amd.engine import Engine, PlsxError
    S, k = 1000, 5
    X, y, rs = ae.design(S, 200, (250, 200, 180, 150, 120, 100), 29)
    kw = dict(n_components=k, n_perm=0, n_boot=0, test_split=3, inner_split=2, seed=12, cv_perm=5, auc=True, verbose=False,
              cv_predict='nested', inner_select='balanced_accuracy')
    one = pls.pls_da(X, y, **kw)
    eng = Engine(scratch_gb=0.02)
    try:
        got = pls.pls_da(X, y, _engine=eng, **kw)
        _same_bits(one.cvres, got.cvres, 'scratch 0.02 GB vs the default engine', COUNTS + SCORES + REGRESSION + ('y_pred', 'predicted'))
        # the series of nested counts: capacity 2 for a call of 3 outer splits
        from pypyls_amd.regression import nested_codes
        codes = nested_codes(one.cvres.cvsamples, one.cvres.innersamples)
        dc = torch.from_numpy(np.ascontiguousarray(codes.transpose(1, 2, 0))).to(eng.device)
        T = 6
        obs = [eng._zeros((3, T)), eng._zeros((3, T)), eng._zeros((3,)),
               torch.zeros((3,), dtype=torch.int32, device=eng.device), eng._zeros((3, k + 1))]
        conf = torch.full((2, T, T), -7, dtype=torch.int32, device=eng.device)
        eng.simpls_cvn_class_begin('accuracy', conf)
        with pytest.raises(PlsxError, match=r'status -1.*series of nested counts holds 0 of 2 blocks, 3 more do not fit') as info:
            eng.simpls_crossval_nested_into(dc, *obs)
        print(info.value)
        assert (conf == -7).all().item()
        eng.simpls_cvn_class_end()
        conf3 = torch.zeros((3, T, T), dtype=torch.int32, device=eng.device)
        eng.simpls_cvn_class_begin('balanced_accuracy', conf3)           # (no AUC counts, no pooled counts asked for)
        eng.simpls_crossval_nested_into(dc, *obs)
        eng.simpls_cvn_class_end()
        eng.sync()
        assert np.array_equal(conf3.cpu().numpy().transpose(1, 2, 0), one.cvres.nested_confusion)
        assert np.array_equal(obs[3].cpu().numpy(), one.cvres.nested_ncomp)
    finally:
        eng.close()


def test_sharded_over_a_team():
    import pypyls_amd as pls
    X, y = _case('G5')[:2]
    team = pls.pls_da(X, y, **_kw('G5', 'balanced_accuracy', cv_predict='nested', device_ids=[0, 0]))
    _same_bits(_run('G5', 'balanced_accuracy').cvres, team.cvres, 'team [0, 0] vs one device',
               COUNTS + SCORES + REGRESSION + PLAIN + ('y_pred', 'predicted', 'y_pred_ncomp'))


def test_save_load_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    res = _run('G2', 'balanced_accuracy')
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    back = pls.load_results(pls.save_results(str(tmp_path / 'da_nested'), res))
    for key in COUNTS + SCORES + REGRESSION + ('innersamples',):
        assert np.array_equal(np.asarray(back.cvres[key]), np.asarray(res.cvres[key]), equal_nan=True), key
        assert np.shape(back.cvres[key]) == np.shape(res.cvres[key]), key
    for key in COUNTS:
        assert np.asarray(back.cvres[key]).dtype == np.int64, key
    assert str(back.inputs.inner_select) == 'balanced_accuracy' and int(back.inputs.inner_split) == 2
