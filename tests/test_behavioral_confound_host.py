"""behavioral_pls(confounds=Z): what can be checked without a GPU -- the conditions the comparison with the device rests
on (tests/behavioral_confound_expect.py), the host-side refusals (raised before any engine exists) and the C ABI
declarations."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import crossval_expect as cx
import behavioral_confound_expect as bx

ENTRIES = ['plsx_residualize', 'plsx_set_confounds', 'plsx_crossval_confound_batch', 'plsx_crossval_confound_perm_batch']


@pytest.mark.parametrize('name', list(bx.CASES))
def test_conditions_on_the_expectation(name):
    """Fold-wise and whole-cohort scores part by >= 0.05 in some entry; kappa, the gaps and M_s M = M_s hold; the mean
    test-row r of the three routes are the measured ones: the raw data predict through Z, the residuals do not."""
    exp = bx.expected(name)
    fig = bx.check_conditions(name, exp)
    print(name, fig)
    case = bx.CASES[name]
    assert exp['r'].shape == exp['r2'].shape == (case['T'], case['m'])
    assert fig['gap'] >= bx.MIN_FOLD_GAP and fig['kappa'] <= cx.KAPPA_MAX and fig['msm'] <= 1e-12
    for got, want in zip(fig['mean_r'], bx.MEAN_R[name]):
        assert abs(got - want) <= 0.006, (name, fig['mean_r'], bx.MEAN_R[name])
    assert fig['mean_r'][0] > 0.3 > 0.15 > abs(fig['mean_r'][1])


def test_fold_operator_is_the_lstsq_of_the_training_rows():
    """M_s = I - Z~ P_s with P_s = (Z~' D Z~)^-1 Z~' D, Z~ = [1, Z - zbar]: the residuals of the expectation."""
    spec, X, Y, Z, masks = bx.problem('C2')
    Xr, Yr = bx.residuals('C2')
    Zt = np.c_[np.ones(len(Z)), Z - Z.mean(axis=0)]
    for s in range(2):
        D = np.diag(masks[:, s].astype(float))
        Ms = np.eye(len(Z)) - Zt @ np.linalg.solve(Zt.T @ D @ Zt, Zt.T @ D)
        Xs, Ys = bx.fold('C2', s)
        assert np.abs(Ms @ Xr - Xs).max() <= 1e-11 and np.abs(Ms @ Yr - Ys).max() <= 1e-11
        assert np.abs(Ms @ Zt).max() <= 1e-11
    # the identity arrangement of the null is the observed statistic
    ident = np.arange(len(Z))[:, None]
    r, r2 = bx.null('C2', ident, masks[:, :2])[:2]
    assert np.array_equal(r[:, 0], bx.expected('C2')['r'][:, :2]) and np.array_equal(r2[:, 0], bx.expected('C2')['r2'][:, :2])
    assert np.array_equal(bx.perms('C2')[:, 0], ident[:, 0])


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create or look up an engine fails the test: validation comes first."""
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was requested before the input was validated')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def _call(X, Y, **kw):
    import pypyls_amd as pls
    kw.setdefault('n_perm', 0)
    kw.setdefault('n_boot', 0)
    kw.setdefault('test_split', 0)
    return pls.behavioral_pls(X, Y, verbose=False, **kw)


def _design():
    spec, X, Y, Z, masks = bx.problem('C3')
    return X, Y, np.c_[Z, np.random.RandomState(9).randn(len(Z))], masks


def test_wrong_shape_raises(no_engine):
    X, Y, Z, masks = _design()
    for bad in (Z[:-1], Z[:, :, None], np.zeros((len(X), 0)), np.array([['a']] * len(X))):
        with pytest.raises(ValueError, match=r'`confounds` must be numeric with shape \(S, q\) or \(S,\)'):
            _call(X, Y, confounds=bad)


def test_too_many_columns_raises(no_engine):
    X, Y, Z, masks = _design()
    with pytest.raises(ValueError, match=r'at most 15 columns; got 16'):
        _call(X, Y, confounds=np.random.RandomState(1).randn(len(X), 16))


def test_non_finite_raises(no_engine):
    X, Y, Z, masks = _design()
    for bad in (np.inf, np.nan):
        Zb = Z.copy()
        Zb[7, 1] = bad
        with pytest.raises(ValueError, match=r'`confounds` must be finite; row 7 is not'):
            _call(X, Y, confounds=Zb)


def test_rank_deficiency_raises(no_engine):
    X, Y, Z, masks = _design()
    with pytest.raises(ValueError, match=r'rank deficient together with the intercept on the 65 rows'):
        _call(X, Y, confounds=np.c_[Z, Z[:, 0] - 2.0 * Z[:, 1]])
    with pytest.raises(ValueError, match=r'rank deficient together with the intercept'):
        _call(X, Y, confounds=np.full(len(X), 3.0))        # a constant: collinear with the intercept


def test_rank_deficiency_on_a_split_raises_and_names_it(no_engine):
    X, Y, Z, masks = _design()
    ind = np.zeros(len(X))
    ind[np.flatnonzero(~masks[:, 2])[:3]] = 1.0            # varies over the cohort, constant on the training rows of split 2
    assert np.ptp(ind[masks[:, 2]]) == 0 and np.ptp(ind) > 0
    with pytest.raises(ValueError, match=r'training rows of split 2'):
        _call(X, Y, confounds=np.c_[Z, ind], test_split=masks.shape[1], _cvsplits=np.array(masks))


def test_pre_permuted_y_raises(no_engine):
    X, Y, Z, masks = _design()
    stack = np.stack([Y[np.random.RandomState(i).permutation(len(Y))] for i in range(2)])
    with pytest.raises(ValueError, match=r'`permindices=False`: pre-permuted Y matrices are not residualised'):
        _call(X, Y, confounds=Z, n_perm=2, permsamples=stack, permindices=False)


def test_the_other_front_ends_refuse_the_keyword(no_engine):
    import pypyls_amd as pls
    X, Y, Z, masks = _design()
    X, Y, Z = X[:64], Y[:64], Z[:64]
    with pytest.raises(ValueError, match=r'`confounds` .* is not available for mean-centred PLS'):
        pls.meancentered_pls(X, groups=[32], n_cond=2, n_perm=0, n_boot=0, verbose=False, confounds=Z)
    with pytest.raises(ValueError, match=r'`confounds` .* is not available for multiblock PLS'):
        pls.multiblock_pls(X, Y, groups=[32], n_cond=2, n_perm=0, n_boot=0, verbose=False, confounds=Z)


def test_result_containers_round_trip_the_new_keys(tmp_path):
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    rs = np.random.RandomState(3)
    res = PLSResults(x_weights=rs.randn(6, 2), singvals=np.array([2.0, 1.0]), confound_mean=rs.randn(2),
                     confound_x=rs.randn(2, 6), confound_y=rs.randn(2, 3),
                     cvres=dict(pearson_r=rs.rand(3, 5), r_squared=rs.rand(3, 5)),
                     inputs=dict(X=rs.randn(8, 6), Y=rs.randn(8, 3), test_split=5, confounds=rs.randn(8, 2)))
    back = io.load_results(io.save_results(str(tmp_path / 'cf'), res))
    for key in ('confound_mean', 'confound_x', 'confound_y'):
        assert np.array_equal(back[key], res[key]), key
    assert np.array_equal(back.inputs.confounds, res.inputs.confounds)


def test_header_declares_and_a_unit_defines_the_entries():
    with open(os.path.join(ROOT, 'include', 'plsx.h')) as f:
        header = f.read()
    with open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')) as f:
        eng = f.read()
    sources = []
    for path in glob.glob(os.path.join(ROOT, 'pypyls_amd', 'csrc', '*.hip')):
        with open(path) as f:
            sources.append(f.read())
    for entry in ENTRIES:
        assert re.search(r'\bint\s+' + entry + r'\s*\(\s*plsx_ctx\s*\*', header), entry
        assert any(re.search(r'\bint\s+' + entry + r'\s*\([^;{]*\)\s*try\s*\{', src, re.S) for src in sources), entry
        assert eng.count("'" + entry + "'") >= 2, entry        # the ctypes signature and the required-symbol list
    from pypyls_amd import _build
    assert 'plsx_confound_behav' in _build.UNITS
    with open(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_k_confound_behav.h')) as f:
        assert re.search(r'void\s+k_cfb_fold_X\s*\(', f.read())
