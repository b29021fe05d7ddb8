"""``behavioral_pls(cv_predict=True)`` on the device (plsx_crossval_pred_begin / _end, k_cv_pred_export): the ``pred`` of
k_cv_final / k_cvp_final against the numpy definition (tests/cv_predict_expect.py on tests/crossval_expect.py and
tests/behavioral_confound_expect.py), against the scores the same call returns, with and without ``covariance``, with and
without ``confounds``, next to ``cv_lv=True``; the NaN pattern; every other array keeps its bits; the refusals of the C ABI.

Tolerance: the bar of the behavioural cross-validation GPU tests, crossval_expect.TOL = 1e-7 per entry (relative to
max(1, |value|)); the designs are those of tests/behavioral_confound_expect.py, whose conditioning that bar rests on
(kappa <= KAPPA_MAX) is asserted there on the expectation.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from oracle import cpu_ref as ref
import behavioral_confound_expect as bx
import crossval_expect as cx
import cv_predict_expect as pe

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -2, -4
# one group, one condition; two groups x two conditions -- each with and without covariance
DESIGNS = {'1g1c': ('C1', False), '1g1c_cov': ('C1', True), '2g2c': ('C2', False), '2g2c_cov': ('C2', True)}


def _problem(name):
    case, cov = DESIGNS[name]
    _, X, Y, Z, masks = bx.problem(case)
    c = bx.CASES[case]
    return ref.Spec('behavioral', c['groups'], c['n_cond'], cov), X, Y, Z, np.array(masks), c, cov


def _call(name, confounds, **extra):
    import pypyls_amd as pls
    spec, X, Y, Z, masks, c, cov = _problem(name)
    kw = dict(groups=c['groups'], n_cond=c['n_cond'], covariance=cov, n_perm=0, n_boot=0, n_split=0,
              test_split=masks.shape[1], test_size=0.25, _cvsplits=masks, cv_lv=True, seed=3, verbose=False)
    kw.update(extra)
    if confounds:
        kw['confounds'] = Z
    return pls.behavioral_pls(X, Y, **kw)


def _self_consistency(cv, y_true, what):
    sc = pe.scores_from_pred(cv['y_pred'], y_true)
    e_r, e_r2 = cx.errors(sc['r'], sc['r2'], cv['pearson_r'], cv['r_squared'])
    print('{}: scores recomputed from y_pred differ by r {:.3e}  r2 {:.3e}'.format(what, e_r, e_r2))
    assert max(e_r, e_r2) <= cx.TOL, what


@pytest.mark.parametrize('confounds', [False, True], ids=['plain', 'confounds'])
@pytest.mark.parametrize('name', sorted(DESIGNS))
def test_against_the_oracle_and_the_scores_of_the_call(name, confounds):
    from confound_expect import residualise
    spec, X, Y, Z, masks, c, cov = _problem(name)
    # what the bar rests on, asserted on the expectation first (measured: kappa <= 24 on all four designs)
    kappa = max(cx.single(spec, *((residualise(X, Z, masks[:, s]), residualise(Y, Z, masks[:, s])) if confounds
                                  else (X, Y)), masks[:, s])[2]['kappa'] for s in range(masks.shape[1]))
    print('{}{}: kappa of the training decompositions <= {:.1f}'.format(name, ' confounds' if confounds else '', kappa))
    assert kappa <= cx.KAPPA_MAX
    res = _call(name, confounds, cv_predict=True)
    off = _call(name, confounds)
    cv = res.cvres
    S, T, n = len(X), Y.shape[1], masks.shape[1]
    assert cv.y_pred.shape == (S, T, n)
    # the NaN pattern: exactly the training rows
    assert np.array_equal(np.isnan(cv.y_pred), np.broadcast_to(masks[:, None, :], (S, T, n)))
    if confounds:
        want, want_true = pe.behav_fold_expected(spec, X, Y, Z, masks)
        e_t = pe.rel_err(cv.y_true, want_true)
        print('{} confounds: max err of y_true {:.3e}'.format(name, e_t))
        assert e_t <= cx.TOL
        _self_consistency(cv, cv.y_true, name + ' confounds')
    else:
        want = pe.behav_pred_expected(spec, X, Y, masks)
        assert 'y_true' not in cv
        _self_consistency(cv, Y, name)
    err = pe.rel_err(cv.y_pred, want)
    print('{}{}: max err of y_pred {:.3e}'.format(name, ' confounds' if confounds else '', err))
    assert err <= cx.TOL
    # every other array keeps its bits (cv_lv rides in the same call)
    new = {'y_pred', 'y_true'} if confounds else {'y_pred'}
    assert set(cv.keys()) - set(off.cvres.keys()) == new and 'lv_corr' in off.cvres
    for key in off.cvres.keys():
        assert np.array_equal(np.asarray(off.cvres[key]), np.asarray(cv[key]), equal_nan=True), key
    for key in ('x_weights', 'y_weights', 'x_scores', 'y_scores', 'y_loadings', 'singvals', 'varexp'):
        assert np.array_equal(off[key], res[key], equal_nan=True), key
    assert res.inputs.cv_predict is True and 'cv_predict' not in off.inputs


def test_team_permutations_and_persistence(tmp_path):
    import pypyls_amd as pls
    one = _call('2g2c', True, cv_predict=True, n_perm=8, n_boot=8, cv_perm=3)
    two = _call('2g2c', True, cv_predict=True, n_perm=8, n_boot=8, cv_perm=3, device_ids=[0, 0])
    for key in ('y_pred', 'y_true', 'pearson_r', 'lv_corr', 'perm_pearson_r'):
        same = np.array_equal(one.cvres[key], two.cvres[key], equal_nan=True)
        print('team of two contexts: cvres.{} bit-identical: {}'.format(key, same))
        assert same
    plain = _call('2g2c', True, cv_predict=True)
    assert np.array_equal(one.cvres.y_pred, plain.cvres.y_pred, equal_nan=True)      # (the observed fits only)
    back = pls.load_results(pls.save_results(str(tmp_path / 'bp'), one))
    for key in ('y_pred', 'y_true'):
        assert np.array_equal(back.cvres[key], one.cvres[key], equal_nan=True), key
    assert bool(back.inputs.cv_predict) is True


def test_abi_capacity_and_refusals():
    import torch
    from pypyls_amd.engine import Engine
    from pypyls_amd import resampling as rsmp
    spec, X, Y, Z, masks, c, cov = _problem('2g2c')
    S, T = len(X), Y.shape[1]
    eng = Engine()
    try:
        lib = eng.lib
        pred = torch.full((3, T, S), -7.0, dtype=torch.float64, device=eng.device)
        assert lib.plsx_crossval_pred_begin(eng.ctx, pred.data_ptr(), None, 3) == ERR_STATE       # nothing bound
        eng.set_data(X, Y, rsmp.cell_of_row(c['groups'], c['n_cond']), len(c['groups']), c['n_cond'], 0)
        assert lib.plsx_crossval_pred_begin(eng.ctx, None, None, 3) == ERR_ARG
        assert lib.plsx_crossval_pred_begin(eng.ctx, pred.data_ptr(), None, 0) == ERR_ARG
        plain = eng.crossval(masks)
        eng.crossval_pred_begin(pred)
        with pytest.raises(Exception) as exc:                 # 5 splits into a series of 3: before anything is written
            eng.crossval(masks)
        print(exc.value)
        assert 'status {}'.format(ERR_ARG) in str(exc.value) and 'plsx_crossval_pred_begin' in str(exc.value)
        eng.sync()
        assert (pred == -7.0).all().item()
        # a permutation entry under the open series leaves the stack alone
        perms = np.stack([np.random.RandomState(s).permutation(S) for s in range(2)], axis=1)
        eng.crossval_perm(masks, perms)
        eng.sync()
        assert (pred == -7.0).all().item()
        # the context works afterwards: 2 + 1 splits fill the 3 slots, the scores keep their bits
        a = eng.crossval(masks[:, :2])
        b = eng.crossval(masks[:, 2:3])
        eng.crossval_pred_end()
        eng.sync()
        assert np.array_equal(np.hstack([a[0], b[0]]), plain[0][:, :3])
        assert np.array_equal(np.hstack([a[1], b[1]]), plain[1][:, :3])
        got = pred.cpu().numpy().transpose(2, 1, 0)
        err = pe.rel_err(got, pe.behav_pred_expected(spec, X, Y, masks[:, :3]))
        print('after the refusals, in two calls: max err of y_pred {:.3e}'.format(err))
        assert err <= cx.TOL
    finally:
        eng.close()
    eng = Engine(scratch_gb=0.001)
    try:
        eng.set_data(X, Y, rsmp.cell_of_row(c['groups'], c['n_cond']), len(c['groups']), c['n_cond'], 0)
        big = torch.empty((1000, T, S), dtype=torch.float64, device=eng.device)
        rc = eng.lib.plsx_crossval_pred_begin(eng.ctx, big.data_ptr(), None, 1000)
        msg = eng.lib.plsx_last_error(eng.ctx).decode()
        print('status {}: {}'.format(rc, msg))
        assert rc == ERR_UNSUPPORTED and 'GB' in msg and '1000' in msg
        assert eng.lib.plsx_crossval_pred_begin(eng.ctx, big.data_ptr(), None, 2) == 0    # (the context lives)
        eng.crossval_pred_end()
    finally:
        eng.close()
