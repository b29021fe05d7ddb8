"""``cv_predict=`` of pls_regression and pls_da on the device (plsx_simpls_cv_pred_begin / _end, k_sd_cv_pred): the
out-of-fold predictions against the oracle (tests/cv_predict_expect.py), against the scores the same call returns, the
nested selection, bit-identity across runs, solver batches, calls and teams, the classification and the ROC curve of
pls_da, and the refusals of the C ABI.

Tolerance: the project's parity bar for regression (tests/test_gpu_regression_cv.py), RTOL = 1e-5 relative to
max(1, |value|), absolute on r.  Every figure is printed before it is asserted; the NaN pattern of every ``y_pred`` must
equal exactly "not a usable test row of that split" (cv_predict_expect.rel_err asserts it on every comparison)."""
import numpy as np
import pytest

import cv_predict_expect as pe
import regression_nested_expect as ne

pytestmark = pytest.mark.gpu
RTOL = 1e-5
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4
CV_KEYS = ('y_pred', 'y_pred_ncomp', 'y_true', 'predicted')


def _global_engine(**kw):
    from pypyls_amd.engine import Engine
    return Engine(options={'simpls_global': 1}, **kw)


def _design(S, B, T, seed, nan=True):
    """randn X, Y = randn + 0.5 X[:, :T]; two rows of X and one of Y NaN throughout; 5 given splits of about a quarter
    of the rows, the masked rows on both sides of them."""
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :T]
    if nan:
        X[[3, S - 2]] = np.nan
        Y[11] = np.nan
    masks = np.ones((S, 5), dtype=bool)
    for s in range(5):
        masks[rs.choice(S, size=S // 4, replace=False), s] = False
    masks[[3, 11], 0] = [False, True]
    masks[S - 2, 1] = False
    return X, Y, masks


def _call(X, Y, masks, k, **kw):
    import pypyls_amd as pls
    args = dict(n_components=k, n_perm=0, n_boot=0, test_split=masks.shape[1], cvsamples=masks, seed=1, verbose=False)
    args.update(kw)
    return pls.pls_regression(X, Y, **args)


def _self_consistency(cv, y_true, c, what):
    """r, R^2 and the summed squared error of every split recomputed on the host from y_pred: the scores of the call."""
    sc = pe.scores_from_pred(cv['y_pred'], y_true)
    errs = dict(r=float(np.max(np.abs(sc['r'] - cv['pearson_r_ncomp'][:, c - 1]))),
                r2=float(np.max(np.abs(sc['r2'] - cv['r_squared_ncomp'][:, c - 1])
                                / np.maximum(1.0, np.abs(cv['r_squared_ncomp'][:, c - 1])))),
                mse=float(np.max(np.abs(sc['mse'] - cv['mse'][c]) / np.maximum(1.0, np.abs(cv['mse'][c])))))
    print('{}: scores recomputed from y_pred differ by r {r:.3e}  r2 {r2:.3e}  mse {mse:.3e}'.format(what, **errs))
    assert max(errs.values()) <= RTOL, (what, errs)
    return errs


# ---- 1. against the oracle

@pytest.mark.parametrize('S', [37, 64, 130])
@pytest.mark.parametrize('T', [1, 3])
def test_regression_against_the_oracle_on_both_routes(S, T):
    """S = 37 / 64 / 130: a ragged last position tile, exactly one tile, more than two positions per lane.  k = 1, 4, 5, 7
    with c = 1, 3, 4, 5, k: c = 4 and 5 on either side of a group of four components, k = 5 and 7 with a partial last
    group and its clamped rows.  Rows that are NaN throughout in X and in Y.  Both solver routes."""
    X, Y, masks = _design(S, 60, T, 100 + S + T)
    eng = _global_engine()
    worst = 0.0
    try:
        for k in (1, 4, 5, 7):
            for c in sorted({c for c in (1, 3, 4, 5, k) if c <= k}):
                want = pe.pred_expected(X, Y, masks, c)
                assert np.array_equal(~np.isnan(want[:, 0, :]), pe.usable_test_rows(X, Y, masks))
                for route, kw in (('on-chip', {}), ('global', dict(_engine=eng))):
                    res = _call(X, Y, masks, k, cv_predict=True if c == k else c, **kw)
                    err = pe.rel_err(res.cvres.y_pred, want)
                    worst = max(worst, err)
                    print('S={} T={} k={} c={} {}: max err of y_pred {:.3e}'.format(S, T, k, c, route, err))
                    assert err <= RTOL
                    assert res.cvres.y_pred.shape == (S, T, 5)
                    assert res.cvres.y_pred_ncomp.dtype == np.int32 and (res.cvres.y_pred_ncomp == c).all()
                    assert 'y_true' not in res.cvres and 'predicted' not in res.cvres
                    _self_consistency(res.cvres, Y, c, 'S={} T={} k={} c={} {}'.format(S, T, k, c, route))
    finally:
        eng.close()
    print('S={} T={}: worst error of y_pred {:.3e}'.format(S, T, worst))


def test_3d_y_in_the_units_of_the_aggregated_y():
    import pypyls_amd as pls
    S, B, T, C, k = 70, 60, 3, 4, 5
    rs = np.random.RandomState(21)
    X = rs.randn(S, B)
    Y = rs.randn(S, T, C) + 0.5 * X[:, :T, None] + 7.0
    X[[3, 40]] = np.nan
    Y[11] = np.nan
    _, _, masks = _design(S, B, T, 5)
    res = pls.pls_regression(X, Y, n_components=k, n_perm=0, n_boot=0, aggfunc='median', test_split=5, cvsamples=masks,
                             cv_predict=3, seed=2, verbose=False)
    Ym = np.median(Y, axis=-1)
    err = pe.rel_err(res.cvres.y_pred, pe.pred_expected(X, Ym, masks, 3))
    print('3-D Y, median: max err of y_pred {:.3e}; mean of y_pred {:.3f}'.format(err, np.nanmean(res.cvres.y_pred)))
    assert err <= RTOL
    _self_consistency(res.cvres, Ym, 3, '3-D Y median')


# ---- 2. self-consistency under confounds (plain: inside test 1)

def test_confounds_return_the_fold_residualised_y():
    """The scores of the confound route compare against a Y the user does not hold: y_true.  An off-by-one in c moves r
    in the second digit."""
    from confound_expect import residualise
    S, B, T, k = 130, 60, 3, 5
    X, Y, masks = _design(S, B, T, 9, nan=False)
    rs = np.random.RandomState(4)
    Z = rs.randn(S, 2)
    X = X + Z @ rs.randn(2, B)
    Y = Y + Z @ rs.randn(2, T)
    for c in (2, 4, 5):
        res = _call(X, Y, masks, k, confounds=Z, cv_predict=c)
        cv = res.cvres
        assert cv.y_true.shape == cv.y_pred.shape == (S, T, 5)
        assert np.array_equal(np.isnan(cv.y_true), np.isnan(cv.y_pred))
        assert np.array_equal(np.isnan(cv.y_pred[:, 0, :]), masks)
        _self_consistency(cv, cv.y_true, c, 'confounds, c={}'.format(c))
        # ... and both against numpy: the fold residuals of X and Y, the c-component model of the training rows
        want_p, want_t = np.full((S, T, 5), np.nan), np.full((S, T, 5), np.nan)
        for s in range(5):
            tr = masks[:, s]
            Xs, Ys = residualise(X, Z, tr), residualise(Y, Z, tr)
            want_p[:, :, s] = pe.pred_expected(Xs, Ys, masks[:, s:s + 1], c)[:, :, 0]
            want_t[~tr, :, s] = Ys[~tr]
        ep, et = pe.rel_err(cv.y_pred, want_p), pe.rel_err(cv.y_true, want_t)
        print('confounds, c={}: max err of y_pred {:.3e}, of y_true {:.3e}'.format(c, ep, et))
        assert max(ep, et) <= RTOL
        near = [float(np.max(np.abs(pe.scores_from_pred(cv.y_pred, cv.y_true)['r'] - cv.pearson_r_ncomp[:, j])))
                for j in range(k) if j != c - 1]
        print('confounds, c={}: r of the neighbouring counts is off by at least {:.3e}'.format(c, min(near)))
        assert min(near) > 100 * RTOL


# ---- 3. nested

def _nested_case():
    """S = 90, k = 5, 6 outer x 3 inner folds: the oracle's selection is [3, 1, 2, 1, 3, 1] (gap 9.8e-3)."""
    from pypyls_amd import resampling
    from pypyls_amd.regression import _draw_inner_codes
    X, Y = ne.design(90, 150, 3, 5, 0.5)
    rs = np.random.RandomState(105)
    masks = resampling.gen_splits([90], 1, 6, seed=rs, test_size=0.25)
    inner = _draw_inner_codes(masks, 3, rs, 0.25)
    return X, Y, masks, inner


def test_nested_predictions_are_those_of_the_chosen_count_to_the_bit():
    from pypyls_amd.regression import nested_codes
    X, Y, masks, inner = _nested_case()
    k = 5
    want = ne.nested_expected(X, Y, nested_codes(masks, inner), k)
    gap = ne.selection_gap(want['inner_mse'])
    print('oracle selection {} (gap {:.3e})'.format(want['ncomp'], gap))
    assert len(set(want['ncomp'].tolist())) >= 2 and want['ncomp'].min() >= 1 and gap >= 1e-4
    res = _call(X, Y, masks, k, inner_split=3, innersamples=inner, cv_predict='nested')
    cv = res.cvres
    print('nested_ncomp {}  y_pred_ncomp {}'.format(cv.nested_ncomp, cv.y_pred_ncomp))
    assert np.array_equal(cv.nested_ncomp, want['ncomp'])
    assert np.array_equal(cv.y_pred_ncomp, cv.nested_ncomp) and cv.y_pred_ncomp.dtype == np.int32
    err = pe.rel_err(cv.y_pred, pe.pred_expected(X, Y, masks, want['ncomp']))
    print('nested: max err of y_pred {:.3e}'.format(err))
    assert err <= RTOL
    for c in sorted(set(cv.nested_ncomp.tolist())):
        plain = _call(X, Y, masks, k, cv_predict=int(c))
        for s in np.flatnonzero(cv.nested_ncomp == c):
            same = np.array_equal(cv.y_pred[:, :, s], plain.cvres.y_pred[:, :, s], equal_nan=True)
            print('split {} (c = {}): nested y_pred bit-identical to the plain call: {}'.format(s, c, same))
            assert same
    # every other array of the nested call keeps its bits
    off = _call(X, Y, masks, k, inner_split=3, innersamples=inner)
    assert set(cv.keys()) - set(off.cvres.keys()) == {'y_pred', 'y_pred_ncomp'}
    for key in off.cvres.keys():
        assert np.array_equal(np.asarray(off.cvres[key]), np.asarray(cv[key]), equal_nan=True), key
    assert res.inputs.cv_predict == 'nested' and 'cv_predict' not in off.inputs


# ---- 4. bits

def _flat(res):
    out = {}
    for key, val in res.items():
        if key == 'inputs':
            continue
        if isinstance(val, dict):
            for k2, v2 in val.items():
                if v2 is not None:
                    out[key + '.' + k2] = v2
        elif val is not None:
            out[key] = val
    return out


def _same_but_new(with_kw, without, what):
    a, b = _flat(with_kw), _flat(without)
    new = set(a) - set(b)
    print('{}: the keyword adds {}'.format(what, sorted(new)))
    assert new <= {'cvres.' + k for k in CV_KEYS} and 'cvres.y_pred' in new and set(b) <= set(a)
    for key in b:
        if isinstance(b[key], np.ndarray) and b[key].dtype == object:
            assert all(np.array_equal(x, y) for x, y in zip(a[key].ravel(), b[key].ravel())), key
        else:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), (what, key)


def test_every_other_array_keeps_its_bits_and_a_repeat_is_identical():
    S, B, T, k = 130, 80, 3, 5
    X, Y, masks = _design(S, B, T, 31)
    kw = dict(n_perm=12, n_boot=12, cv_perm=4, coef_components=3, vip_components=2, n_split=2)
    off = _call(X, Y, masks, k, **kw)
    on = _call(X, Y, masks, k, cv_predict=4, **kw)
    again = _call(X, Y, masks, k, cv_predict=4, **kw)
    _same_but_new(on, off, 'next to cv_perm, coef_components, vip_components and n_split')
    assert np.array_equal(on.cvres.y_pred, again.cvres.y_pred, equal_nan=True)
    assert on.inputs.cv_predict == 4 and 'cv_predict' not in off.inputs
    assert 'cv_predict' not in _call(X, Y, masks, k, cv_predict=False).inputs
    err = pe.rel_err(on.cvres.y_pred, pe.pred_expected(X, Y, masks, 4))
    print('with cv_perm in the same call: max err of y_pred {:.3e} (the observed fits only)'.format(err))
    assert err <= RTOL


def test_same_bits_over_solver_batches_calls_and_a_team(monkeypatch):
    """One fit at S = 130, T = 3, k = 5 holds some 45 KB of solver state, dual weights and scores: a budget of 0.0002 GB
    (half of it for a batch) cuts the 5 splits into several solver batches."""
    import torch
    from pypyls_amd.engine import Engine
    S, B, T, k, c = 130, 80, 3, 5, 3
    X, Y, masks = _design(S, B, T, 41)
    one = _call(X, Y, masks, k, cv_predict=c)
    eng = Engine(scratch_gb=0.0002)
    try:
        eng.set_timing(True)
        small = _call(X, Y, masks, k, cv_predict=c, _engine=eng)
        launches = eng.kernel_timing()['k_sd_cv_score'][1]
    finally:
        eng.close()
    print('0.0002 GB: {} launches in the scoring class (two per solver batch: k_sd_cv_score, k_sd_cv_pred)'.format(launches))
    assert launches >= 4 and launches % 2 == 0
    assert np.array_equal(one.cvres.y_pred, small.cvres.y_pred, equal_nan=True)
    from pypyls_amd import team as _team
    calls, orig = [], _team.Team.allgather

    def counting(self, rank, flat):
        calls.append(rank)
        return orig(self, rank, flat)
    monkeypatch.setattr(_team.Team, 'allgather', counting)
    team = _call(X, Y, masks, k, cv_predict=c, device_ids=[0, 0])
    print('all-gather calls per rank with cv_predict: {}'.format(sorted(calls)))
    assert sorted(calls) == [0, 1]                           # the prediction rows ride in the ONE collective
    assert np.array_equal(one.cvres.y_pred, team.cvres.y_pred, equal_nan=True)
    assert np.array_equal(one.cvres.y_pred_ncomp, team.cvres.y_pred_ncomp)
    # the C entry in two calls of 2 + 3 splits under one series
    eng = Engine()
    try:
        ok = ~np.isnan(X).all(axis=1)
        oky = ~np.isnan(Y).all(axis=1)
        eng.set_data_regression(np.nan_to_num(X - np.nanmean(X, axis=0)), np.nan_to_num(Y - np.nanmean(Y, axis=0)), k)
        eng.simpls_set_row_masks(ok & oky, ok & oky)
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        pred = torch.full((5, T, S), -7.0, dtype=torch.float64, device=eng.device)
        nc = torch.full((5,), -7, dtype=torch.int32, device=eng.device)
        out = [eng._zeros((5, k, T)), eng._zeros((5, k, T)), eng._zeros((5, k + 1, T))]
        eng.simpls_cv_pred_begin(c, pred, nc)
        for a, b in ((0, 2), (2, 5)):
            eng.simpls_crossval_into(dm[a:b], *(t[a:b] for t in out))
        eng.simpls_cv_pred_end()
        eng.sync()
        got = pred.cpu().numpy().transpose(2, 1, 0) + np.nanmean(Y, axis=0)[None, :, None]
        assert (nc.cpu().numpy() == c).all()
    finally:
        eng.close()
    same = np.array_equal(got, one.cvres.y_pred, equal_nan=True)
    print('the C entry in 2 + 3 splits: bit-identical to the front end: {}'.format(same))
    assert same


# ---- 5. pls_da

def _da_design(S, sizes, seed, shift=0.6):
    """Overlapping classes (the AUC is not 1), and in every split two test rows of different classes with identical
    feature rows: a tie the ROC curve and the AUC counts must rank alike."""
    rs = np.random.RandomState(seed)
    G = len(sizes)
    y = rs.permutation(np.repeat(np.arange(G), sizes))
    X = rs.randn(S, 40)
    X[:, :5] += (shift * rs.randn(G, 5))[y]
    i, j = int(np.flatnonzero(y == 0)[0]), int(np.flatnonzero(y == 1)[0])
    X[j] = X[i]
    masks = np.ones((S, 5), dtype=bool)
    for s in range(5):
        for g in range(G):
            rows = np.setdiff1d(np.flatnonzero(y == g), [i, j])
            masks[rs.choice(rows, size=max(2, len(rows) // 4), replace=False), s] = False
        masks[[i, j], s] = False
    return X, y, masks, (i, j)


@pytest.mark.parametrize('sizes', [(60, 55), (30, 28, 26, 24), (26, 24, 22, 20, 18)], ids=['G2', 'G4', 'G5'])
def test_pls_da_predictions_classes_and_roc(sizes):
    """G = 4 and G = 5 sit on either side of the compile-time bounds 4 / 16 of k_sd_cv_pred<GB>.

    The trapezoid area under roc_curve against cvres.auc: both count the same ranks, so only the rounding of the
    trapezoid sum is allowed.  The same check on the ORACLE's predictions on the CPU (roc_points against
    cv_predict_expect.auc_mann_whitney, these three designs, every class and split) differs by at most 1.11e-16; with a
    100 x margin the floor is AUC_TOL = 1.2e-14."""
    import pypyls_amd as pls
    AUC_TOL = 1.2e-14
    S, G, k, c = sum(sizes), len(sizes), 4, 3
    X, y, masks, (i, j) = _da_design(S, sizes, 7 + G)
    res = pls.pls_da(X, y, n_components=k, n_perm=0, n_boot=0, test_split=5, cvsamples=masks, cv_predict=c, auc=True,
                     seed=1, verbose=False)
    cv = res.cvres
    want_p, want_cls = pe.da_pred_expected(X, y, masks, c)
    err = pe.rel_err(cv.y_pred, want_p)
    print('G={}: max err of the predicted indicators {:.3e}'.format(G, err))
    assert err <= RTOL and cv.y_pred.shape == (S, G, 5)
    assert cv.predicted.shape == (S, 5) and cv.predicted.dtype == np.int32
    test = ~masks
    assert np.array_equal(cv.predicted >= 0, test) and (cv.predicted[~test] == -1).all()
    for s in range(5):
        assert np.array_equal(np.argmax(cv.y_pred[test[:, s], :, s], axis=1), cv.predicted[test[:, s], s]), s
    conf = pe.confusion_from_predicted(cv.predicted, y, G)
    differ = int(np.sum(conf != cv.confusion[:, :, c - 1, :]))
    print('G={}: {} of {} confusion cells recounted from `predicted` differ'.format(G, differ, conf.size))
    assert differ == 0
    # the planted tie: identical feature rows give identical predictions, bit for bit
    assert np.array_equal(cv.y_pred[i], cv.y_pred[j])
    worst = 0.0
    for g in range(G):
        for s in range(5):
            fpr, tpr, thr = pls.roc_curve(res, res.classes[g], s)
            area = pe.trapezoid(fpr, tpr)
            worst = max(worst, abs(area - cv.auc[g, c - 1, s]))
            assert (np.diff(thr) < 0).all() and fpr[0] == tpr[0] == 0.0 and fpr[-1] == tpr[-1] == 1.0
            if g <= 1:
                assert len(thr) - 1 < int(test[:, s].sum())      # (the tied pair is one point)
    print('G={}: trapezoid area of roc_curve vs cvres.auc: max diff {:.3e}; auc in [{:.3f}, {:.3f}]'
          .format(G, worst, np.nanmin(cv.auc[:, c - 1]), np.nanmax(cv.auc[:, c - 1])))
    assert worst <= AUC_TOL
    assert np.nanmin(cv.auc[:, c - 1]) < 1.0                  # (overlapping classes: the curves are not the corner)
    off = pls.pls_da(X, y, n_components=k, n_perm=0, n_boot=0, test_split=5, cvsamples=masks, auc=True, seed=1,
                     verbose=False)
    _same_but_new(res, off, 'pls_da G={}'.format(G))


# ---- 7. capacity and refusals

def test_abi_capacity_permutation_entries_and_refusals():
    import torch
    from pypyls_amd.engine import Engine, PlsxError
    S, B, T, k = 64, 40, 2, 3
    X, Y, masks = _design(S, B, T, 51, nan=False)
    eng = Engine()
    try:
        lib = eng.lib
        pred = torch.full((3, T, S), -7.0, dtype=torch.float64, device=eng.device)
        assert lib.plsx_simpls_cv_pred_begin(eng.ctx, 1, None, pred.data_ptr(), None, 3) == ERR_STATE   # nothing bound
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)
        assert lib.plsx_simpls_cv_pred_begin(eng.ctx, 1, None, None, None, 3) == ERR_ARG
        assert lib.plsx_simpls_cv_pred_begin(eng.ctx, 1, None, pred.data_ptr(), None, 0) == ERR_ARG
        assert lib.plsx_simpls_cv_pred_begin(eng.ctx, k + 1, None, pred.data_ptr(), None, 3) == ERR_ARG
        print(lib.plsx_last_error(eng.ctx).decode())
        dm = torch.from_numpy(np.ascontiguousarray(masks.T, dtype=np.uint8)).to(eng.device)
        out = [eng._zeros((5, k, T)), eng._zeros((5, k, T)), eng._zeros((5, k + 1, T))]
        # 5 splits into a series of 3: refused before anything is written
        eng.simpls_cv_pred_begin(2, pred)
        rc = lib.plsx_simpls_crossval_batch(eng.ctx, dm.data_ptr(), 5, *(t.data_ptr() for t in out), eng._stream())
        msg = lib.plsx_last_error(eng.ctx).decode()
        print('status {}: {}'.format(rc, msg))
        eng.sync()
        assert rc == ERR_ARG and 'plsx_simpls_cv_pred_begin' in msg and '3' in msg
        assert (pred == -7.0).all().item() and all((t == 0).all().item() for t in out)
        # a permutation entry under the open series leaves the stack alone
        perms = eng.rows_tensor(np.stack([np.random.RandomState(s).permutation(S) for s in range(2)]))
        pout = [eng._zeros((2, k, T)), eng._zeros((2, k, T)), eng._zeros((2, k + 1))]
        eng.simpls_crossval_perm_into(dm, perms, *pout)
        eng.sync()
        assert (pred == -7.0).all().item() and np.isfinite(pout[0].cpu().numpy()).all()
        # c = 0 waits for a nested selection: the plain entry refuses
        eng.simpls_cv_pred_begin(0, pred)
        rc = lib.plsx_simpls_crossval_batch(eng.ctx, dm.data_ptr(), 3, *(t.data_ptr() for t in out), eng._stream())
        print('status {}: {}'.format(rc, lib.plsx_last_error(eng.ctx).decode()))
        assert rc == ERR_ARG and (pred == -7.0).all().item()
        # the context works afterwards: 3 splits fill the 3 slots
        eng.simpls_cv_pred_begin(2, pred)
        eng.simpls_crossval_into(dm[:3], *(t[:3] for t in out))
        eng.simpls_cv_pred_end()
        eng.sync()
        got = pred.cpu().numpy().transpose(2, 1, 0) + Y.mean(axis=0)[None, :, None]
        err = pe.rel_err(got, pe.pred_expected(X, Y, masks[:, :3], 2))
        print('after the refusals: max err of y_pred {:.3e}'.format(err))
        assert err <= RTOL
        # ... and after the series has ended nothing is appended
        pred.fill_(-7.0)
        eng.simpls_crossval_into(dm[:3], *(t[:3] for t in out))
        eng.sync()
        assert (pred == -7.0).all().item()
    finally:
        eng.close()
    # a stack beyond the scratch budget: PLSX_ERR_UNSUPPORTED with the sizes, and the context lives
    eng = Engine(scratch_gb=0.001)
    try:
        eng.set_data_regression(X - X.mean(axis=0), Y - Y.mean(axis=0), k)
        big = torch.empty((2000, T, S), dtype=torch.float64, device=eng.device)
        with pytest.raises(PlsxError) as exc:
            eng.simpls_cv_pred_begin(2, big)
        print(exc.value)
        assert 'status {}'.format(ERR_UNSUPPORTED) in str(exc.value) and 'GB' in str(exc.value)
        assert '2000' in str(exc.value)
        small = torch.empty((3, T, S), dtype=torch.float64, device=eng.device)
        eng.simpls_cv_pred_begin(2, small)
        eng.simpls_cv_pred_end()
    finally:
        eng.close()
