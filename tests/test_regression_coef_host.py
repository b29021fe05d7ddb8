"""pls_regression(coef_components=c) and predict on the host (no GPU): the oracle helper against the fixtures the
reference's ``simpls(...)['beta']`` wrote (tests/golden/make_coef_golden.py), ``predict`` against ``[1, x] @ beta`` and
against the cross-validation helper, validation before any engine exists, the header, persistence."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden, assert_close
from oracle import cpu_ref as ref
from regression_coef_expect import coef_expected, max_rel, packed_bootsamples
from regression_cv_expect import cv_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ['a', 'nan', 'y3d']
PIN = 1e-10            # helper vs reference fixtures (the generator measured 1.6e-15 at worst)


def _case(tag):
    g = load_golden('simpls_coef_' + tag)
    return g, int(g['n_components']), int(g['coef_components']), str(g['aggfunc']), g.get('third')


def _oracle_result(X, Y, k, aggfunc='mean', **inputs):
    """A PLSResults as pls_regression lays it out, from the oracle's fit."""
    from pypyls_amd.structures import PLSResults
    fit = ref.run_regression(X, Y, k, aggfunc=aggfunc)
    return PLSResults(x_weights=fit['x_weights'], y_loadings=fit['y_loadings'], x_scores=fit['x_scores'],
                      varexp=fit['varexp'], inputs=dict(X=X, Y=Y, n_components=k, aggfunc=aggfunc, **inputs))


@pytest.mark.parametrize('tag', TAGS)
def test_helper_reproduces_the_reference_fixtures(tag):
    g, k, c, aggfunc, third = _case(tag)
    want = coef_expected(g['X'], g['Y'], g['bootsamples'], k, c, aggfunc=aggfunc, third=third)
    for key in ('coefs', 'intercept', 'bsum', 'bsq'):
        err = max_rel(want[key], g['ref_' + key])
        print('simpls_coef_{} {}: oracle vs reference {:.3e}'.format(tag, key, err))
        assert err <= PIN, (tag, key, err)
    assert want['n'] == g['bootsamples'].shape[1]
    assert np.max(np.abs(want['normed'])) < 1e3 and want['stderr'].min() >= 1e-8 * want['stderr'].max()


@pytest.mark.parametrize('tag', TAGS)
def test_predict_is_one_x_times_beta_of_the_reference(tag):
    import pypyls_amd as pls
    g, k, c, aggfunc, third = _case(tag)
    X, Y = g['X'], g['Y']
    res = _oracle_result(X, Y, k, aggfunc=aggfunc)
    rs = np.random.RandomState(5)
    X_new = rs.randn(9, X.shape[1])
    want = np.column_stack([np.ones(9), X_new]) @ np.vstack([g['ref_intercept'][None], g['ref_coefs']])
    got = pls.predict(res, X_new, n_components=c)
    assert got.shape == (9, Y.shape[1])
    assert_close(got, want, rtol=1e-10, what='predict ' + tag)
    # n_components=None: the coef_components of the result when it has one, otherwise every component
    assert np.array_equal(pls.predict(_oracle_result(X, Y, k, aggfunc=aggfunc, coef_components=c), X_new), got)
    assert np.array_equal(pls.predict(res, X_new), pls.predict(res, X_new, n_components=k))


def test_predict_gives_back_the_cross_validation_errors():
    """Fitted on the training rows of a split, predict on its test rows reproduces the sse rows of cv_expected, for
    every component count."""
    import pypyls_amd as pls
    g = load_golden('simpls_cv_a')
    X, Y, masks, k = g['X'], g['Y'], g['cvsamples'], int(g['n_components'])
    want = cv_expected(X, Y, masks, k)
    for s in range(masks.shape[1]):
        tr, te = masks[:, s], ~masks[:, s]
        res = _oracle_result(X[tr], Y[tr], k)
        for c in range(1, k + 1):
            sse = np.sum((Y[te] - pls.predict(res, X[te], n_components=c)) ** 2, axis=0)
            assert_close(sse, want['sse'][:, c, s], rtol=1e-9, what='split {} c {}'.format(s, c))


def test_validation_errors_come_before_any_engine():
    import pypyls_amd as pls
    rs = np.random.RandomState(0)
    X, Y = rs.randn(20, 30), rs.randn(20, 3)
    for bad in (0, 5, -1, 2.5, True, 'two'):
        with pytest.raises((ValueError, TypeError)) as exc:
            pls.pls_regression(X, Y, n_components=4, coef_components=bad, n_perm=0, n_boot=0, verbose=False)
        assert exc.type is not TypeError or bad == 'two'
    with pytest.raises(ValueError, match='coef_components'):
        pls.pls_regression(X, Y, n_components=4, coef_components=5, n_perm=0, n_boot=0, verbose=False)
    res = _oracle_result(X, Y, 4)
    with pytest.raises(ValueError):
        pls.predict(res, rs.randn(3, 29))                      # wrong feature count
    for bad in (0, 5, 1.5):
        with pytest.raises(ValueError):
            pls.predict(res, rs.randn(3, 30), n_components=bad)
    from pypyls_amd.structures import PLSResults
    other = PLSResults(x_weights=res.x_weights, y_loadings=res.y_loadings, singvals=np.ones(4),
                       inputs=dict(X=X, Y=Y))
    with pytest.raises(ValueError, match='pls_regression'):
        pls.predict(other, rs.randn(3, 30))                    # a PLS-C result


def test_header_and_structures_declare_the_new_surface():
    hdr = open(os.path.join(ROOT, 'include', 'plsx.h')).read()
    for name in ('plsx_simpls_coef_begin', 'plsx_simpls_coef_finish'):
        assert re.search(r'\bint ' + name + r'\s*\(plsx_ctx\* ctx', hdr), name
    src = open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')).read()
    assert src.count("'plsx_simpls_coef_begin'") >= 2 and src.count("'plsx_simpls_coef_finish'") >= 2
    from pypyls_amd import structures as st
    assert {'coefs', 'intercept'} <= set(st.PLSResults.allowed)
    assert {'coefs_stderr', 'coefs_normed'} <= set(st.PLSBootResults.allowed)
    assert 'coef_components' in st.PLSInputs.allowed
    # a record that was not given the keyword holds no trace of it
    assert 'coef_components' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1)


def test_save_load_predict_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g, k, c, aggfunc, third = _case('y3d')
    X, Y = g['X'], g['Y']
    want = coef_expected(X, Y, g['bootsamples'], k, c, aggfunc=aggfunc, third=third)
    res = _oracle_result(X, Y, k, aggfunc=aggfunc, coef_components=c)
    res['coefs'], res['intercept'] = want['coefs'], want['intercept']
    res['bootres'].update(dict(coefs_stderr=want['stderr'], coefs_normed=want['normed']))
    back = pls.load_results(pls.save_results(str(tmp_path / 'coef'), res))
    assert int(back.inputs.coef_components) == c
    for key in ('coefs', 'intercept'):
        assert np.array_equal(back[key], res[key]), key
    for key in ('coefs_stderr', 'coefs_normed'):
        assert np.array_equal(back.bootres[key], res.bootres[key]), key
    X_new = np.random.RandomState(2).randn(4, X.shape[1])
    got = pls.predict(back, X_new)
    assert np.array_equal(got, pls.predict(res, X_new))
    assert_close(got, want['intercept'] + X_new @ want['coefs'], rtol=1e-12, what='predict after load')
