"""pls_regression(vip_components=c) and pyls.vip on the host (no GPU): the oracle helpers against the fixtures the
reference's ``simpls`` wrote (tests/golden/make_vip_golden.py), ``pyls.vip`` on results assembled the way the front-end
assembles them, the invariant sum VIP^2 = B, independence of the signs and the order of the components, validation
before any engine exists, the records, persistence, the header and the built library."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from oracle import cpu_ref as ref
from regression_coef_expect import _AGG, max_rel
from regression_vip_expect import stack_boot, stack_vip, summary, vip_boot, vip_expected, vip_formula, vip_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ['a', 'nan', 'y3d']
PIN = 1e-10            # oracle vs reference fixtures (the generator measured 4.2e-15 at worst)
ENTRIES = ('plsx_simpls_vip_keep', 'plsx_simpls_vip_ci')


def _result(g, **inputs):
    """A PLSResults the way pls_regression fills it (regression.py of this package: x_scores NaN on masked rows,
    y_loadings = Yc^T x_scores over the rows of the fit), from the oracle's fit."""
    from pypyls_amd.structures import PLSResults
    k, aggfunc = int(g['n_components']), str(g['aggfunc'])
    X, Y = g['X'], g['Y']
    Y_agg = _AGG[aggfunc](Y, axis=-1) if Y.ndim == 3 else Y
    Xc = X - np.nanmean(X, axis=0, keepdims=True)
    Yc = Y_agg - np.nanmean(Y_agg, axis=0, keepdims=True)
    mask = ref.get_mask(Xc, Yc)
    fit = ref.simpls(Xc[mask], Yc[mask], k)
    x_scores = np.full((len(X), k), np.nan)
    x_scores[mask] = Xc[mask] @ fit['x_weights']
    return PLSResults(x_weights=fit['x_weights'], x_scores=x_scores, y_loadings=Yc[mask].T @ x_scores[mask],
                      inputs=dict(X=X, Y=Y, n_components=k, aggfunc=aggfunc, **inputs))


@pytest.mark.parametrize('tag', TAGS)
def test_helpers_reproduce_the_reference_fixtures(tag):
    g, f = load_golden('simpls_coef_' + tag), load_golden('simpls_vip_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    B = g['X'].shape[1]
    assert f['ref_vip'].shape == (B,) and f['ref_stderr'].shape == (B,)
    assert f['ref_ci'].shape == (len(f['ci']), B, 2) and list(f['ci']) == [95, 80]
    boot = vip_boot(g['X'], g['Y'], g['bootsamples'], k, c, aggfunc=aggfunc, third=g.get('third'))
    assert boot.shape == (g['bootsamples'].shape[1], B)
    inv = float(np.max(np.abs((boot ** 2).sum(axis=1) - B)) / B)
    print('simpls_vip_{}: sum VIP^2 off B by {:.3e} relative over the bootstraps'.format(tag, inv))
    assert inv <= 1e-12
    for i, level in enumerate(f['ci']):
        want = vip_expected(g['X'], g['Y'], g['bootsamples'], k, c, ci=level, aggfunc=aggfunc, third=g.get('third'))
        errs = dict(vip=max_rel(want['vip'], f['ref_vip']), stderr=max_rel(want['stderr'], f['ref_stderr']),
                    ci=max_rel(want['ci'], f['ref_ci'][i]))
        print('simpls_vip_{} ci={:g}: oracle vs reference {}'.format(tag, level, errs))
        assert max(errs.values()) <= PIN, (tag, level, errs)
        assert np.all(want['ci'][:, 0] <= want['ci'][:, 1])
    assert np.all(f['ref_ci'][0][:, 0] <= f['ref_ci'][1][:, 0]) and np.all(f['ref_ci'][1][:, 1] <= f['ref_ci'][0][:, 1])


@pytest.mark.parametrize('tag', TAGS)
def test_public_vip_against_the_reference_fixtures(tag):
    """pyls.vip on a result holds the reference's VIP of the original fit -- with rows that are NaN throughout (tag nan)
    through simpls' own y_loadings, with 3-D Y through the aggregated Y -- and the invariant."""
    import pypyls_amd as pls
    g, f = load_golden('simpls_coef_' + tag), load_golden('simpls_vip_' + tag)
    k, c = int(g['n_components']), int(g['coef_components'])
    B = g['X'].shape[1]
    res = _result(g)
    got = pls.vip(res, n_components=c)
    err = max_rel(got, f['ref_vip'])
    print('simpls_vip_{}: pyls.vip vs reference {:.3e}'.format(tag, err))
    assert got.shape == (B,) and err <= PIN
    assert np.array_equal(pls.vip(_result(g, vip_components=c)), got)          # the recorded count is the default
    for cc in range(1, k + 1):                                                  # nested models, the invariant for each
        v = pls.vip(res, n_components=cc)
        assert abs((v ** 2).sum() - B) <= 1e-12 * B, (cc, (v ** 2).sum())
    assert np.array_equal(pls.vip(res), pls.vip(res, n_components=k))          # otherwise all components


def test_vip_is_independent_of_component_signs_and_order():
    import pypyls_amd as pls
    g = load_golden('simpls_coef_a')
    res = _result(g)
    k = int(g['n_components'])
    want = pls.vip(res)
    rs = np.random.RandomState(3)
    signs, order = rs.choice([-1.0, 1.0], size=k), rs.permutation(k)
    for key in ('x_weights', 'y_loadings', 'x_scores'):
        res[key] = (np.asarray(res[key]) * signs)[:, order]
    assert max_rel(pls.vip(res), want) <= 1e-14
    # a scaled weight column changes nothing either: the formula normalises it
    res['x_weights'] = np.asarray(res['x_weights']) * np.linspace(0.5, 2.0, k)
    assert max_rel(pls.vip(res), want) <= 1e-14


def test_vip_degenerate_fits_give_nan_and_bad_arguments_raise():
    import pypyls_amd as pls
    g = load_golden('simpls_coef_a')
    res = _result(g)
    k = int(g['n_components'])
    W = np.array(res['x_weights'])
    W[:, 1] = 0.0
    res['x_weights'] = W
    with np.errstate(all='ignore'):
        assert np.isnan(pls.vip(res, n_components=2)).all()                     # a component of zero weight norm
        assert np.isfinite(pls.vip(res, n_components=1)).all()
    res['y_loadings'] = np.zeros_like(res['y_loadings'])
    with np.errstate(all='ignore'):
        assert np.isnan(pls.vip(res, n_components=1)).all()                     # nothing explained
    for bad in (0, k + 1, 1.5, True):
        with pytest.raises(ValueError, match='n_components'):
            pls.vip(res, n_components=bad)
    with pytest.raises(ValueError, match='not a pls_regression result'):
        pls.vip(dict(x_weights=W))


def test_helper_weights_and_stack_form():
    """Replication counts repeat the rows; the subject-space form gives the same series; one bootstrap has no spread."""
    rs = np.random.RandomState(1)
    boot = np.abs(rs.randn(5, 7))
    w = np.array([3, 1, 2, 1, 4])
    for got, want in zip(summary(boot, 90, weights=w), summary(np.repeat(boot, w, axis=0), 90)):
        assert np.array_equal(got, want)
    Xc, stack = rs.randn(11, 7), rs.randn(5, 3, 11)
    want = np.stack([np.sqrt(7 * ((Xc.T @ stack[b].T) ** 2).sum(axis=1)) for b in range(5)])
    assert max_rel(stack_boot(Xc, stack), want) <= 1e-14
    sd, iv = stack_vip(Xc, stack, 80)
    assert max_rel(sd, np.std(want, ddof=1, axis=0)) <= 1e-14 and iv.shape == (7, 2)
    assert np.isnan(summary(boot[:1])[0]).all()
    # the stack form of a fit: rows sqrt(ssq_a / (|w_a|^2 sum ssq)) a_a with w_a = Xc^T a_a reproduce the formula
    W, Q = rs.randn(7, 3), rs.randn(4, 3)
    A = np.linalg.lstsq(Xc.T, W, rcond=None)[0].T                       # (3, 11): Xc^T a_a = w_a (11 > 7: solvable)
    ssq = (Q ** 2).sum(axis=0)
    G = A * np.sqrt(ssq / ((W ** 2).sum(axis=0) * ssq.sum()))[:, None]
    assert max_rel(stack_boot(Xc, G[None])[0], vip_formula(W, Q, 3)) <= 1e-12


def test_validation_errors_come_before_any_engine(monkeypatch):
    import pypyls_amd as pls
    from pypyls_amd import engine
    made = []
    monkeypatch.setattr(engine, 'default_engine', lambda *a, **k: made.append(1))
    monkeypatch.setattr(engine.Engine, '__init__', lambda self, *a, **k: made.append(1))
    rs = np.random.RandomState(0)
    X, Y = rs.randn(20, 30), rs.randn(20, 3)
    kw = dict(n_components=4, n_perm=0, verbose=False)
    for bad in (0, 5, 2.5, True, 'two'):
        with pytest.raises((ValueError, TypeError), match='vip_components|invalid literal'):
            pls.pls_regression(X, Y, vip_components=bad, n_boot=10, **kw)
    with pytest.raises(ValueError, match=r'vip_components.*1 \.\. n_components = 4'):
        pls.pls_regression(X, Y, vip_components=5, n_boot=10, **kw)
    with pytest.raises(ValueError, match='vip_components.*16384.*no host fallback'):
        pls.pls_regression(X, Y, vip_components=2, n_boot=16385, **kw)
    assert not made


def test_records_declare_the_new_surface():
    from pypyls_amd import structures as st
    assert {'vip_stderr', 'vip_ci'} <= set(st.PLSBootResults.allowed)
    assert 'vip' in st.PLSResults.allowed and 'vip_components' in st.PLSInputs.allowed
    # a record that was not given the keyword holds no trace of it
    assert 'vip_components' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1)
    assert st.PLSInputs(X=np.zeros((2, 2)), n_components=1, vip_components=1).vip_components == 1
    import inspect
    import pypyls_amd as pls
    assert inspect.signature(pls.pls_regression).parameters['vip_components'].default is None
    assert callable(pls.vip) and list(inspect.signature(pls.vip).parameters) == ['results', 'n_components']


def test_header_engine_and_library_carry_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'plsx.h')).read()
    for name in ENTRIES:
        assert re.search(r'\bint ' + name + r'\s*\(plsx_ctx\* ctx', hdr), name
    src = open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')).read()
    for name in ENTRIES:
        assert src.count("'" + name + "'") >= 2, name
    from pypyls_amd import _build, engine
    _build.build()
    assert set(ENTRIES) <= set(engine.exported_symbols())
    for meth in ('simpls_vip_keep', 'simpls_vip_ci'):
        assert callable(getattr(engine.Engine, meth))
    kernels = open(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_kernels.h')).read()
    assert '#include "plsx_k_vip.h"' in kernels


def test_save_load_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g = load_golden('simpls_coef_nan')
    k, c = int(g['n_components']), int(g['coef_components'])
    want = vip_expected(g['X'], g['Y'], g['bootsamples'], k, c, ci=90)
    res = _result(g, ci=90, vip_components=c)
    res['vip'] = want['vip']
    res['bootres']['vip_stderr'], res['bootres']['vip_ci'] = want['stderr'], want['ci']
    back = pls.load_results(pls.save_results(str(tmp_path / 'vip'), res))
    assert int(back.inputs.vip_components) == c
    assert np.array_equal(back.vip, want['vip']) and np.array_equal(back.bootres.vip_stderr, want['stderr'])
    assert np.array_equal(back.bootres.vip_ci, want['ci']) and back.bootres.vip_ci.shape == want['ci'].shape
    # pyls.vip on what was read back: the same function, the recorded component count
    got = pls.vip(back)
    assert max_rel(got, want['vip']) <= PIN and max_rel(got, load_golden('simpls_vip_nan')['ref_vip']) <= PIN
