"""pls_regression(coef_components=c, coef_perm=True) on the host (no GPU): the oracle helper against the fixtures the
reference's ``simpls(...)['beta']`` wrote (tests/golden/make_coef_perm_golden.py), validation before any engine exists,
a feature without variance, the records, persistence, the header and the built library."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from regression_coef_expect import max_rel
from regression_coef_perm_expect import coef_perm_expected, min_rel_gap, pvals_of, stack_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ['a', 'nan', 'y3d']
PIN = 1e-10            # helper vs reference fixtures (the generator measured 2.7e-14 at worst)
MIN_GAP = 1e-8         # no count of a fixture is closer to a tie than this
ENTRIES = ('plsx_simpls_coef_perm_test', 'plsx_simpls_coef_perm_begin', 'plsx_simpls_coef_perm_end')
KEYS = ('coefs_pvals', 'coefs_max', 'coefs_pvals_fwe')


@pytest.mark.parametrize('tag', TAGS)
def test_helper_reproduces_the_reference_fixtures(tag):
    g, f = load_golden('simpls_coef_' + tag), load_golden('simpls_coef_perm_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    B, T, n = g['X'].shape[1], g['Y'].shape[1], f['permsamples'].shape[1]
    assert f['ref_count'].shape == (B, T) and f['ref_max'].shape == (T, n)
    assert np.array_equal(np.sort(f['permsamples'], axis=0), np.broadcast_to(np.arange(len(g['X']))[:, None], (len(g['X']), n)))
    want = coef_perm_expected(g['X'], g['Y'], f['permsamples'], k, c, aggfunc=aggfunc)
    gap = min_rel_gap(want['coefs'], want['perms'])
    err = max_rel(want['coefs_max'], f['ref_max'])
    print('simpls_coef_perm_{}: oracle vs reference coefs_max {:.3e}, smallest gap {:.3e} (fixture {:.3e})'.format(
        tag, err, gap, float(f['min_gap'])))
    assert err <= PIN, (tag, err)
    assert gap > MIN_GAP and float(f['min_gap']) > MIN_GAP
    assert np.array_equal(want['count'], f['ref_count'])
    assert np.array_equal(want['coefs_pvals'], f['ref_pvals'])
    assert np.array_equal(want['coefs_pvals_fwe'], f['ref_pvals_fwe'])
    # the family-wise p-value is never below the uncorrected one where the scale is common to both sides
    assert np.all(f['ref_pvals_fwe'] >= f['ref_pvals']) and f['ref_pvals'].min() >= 1 / (n + 1) and f['ref_pvals'].max() <= 1


def test_front_end_formulas_match_the_helper():
    """regression._coef_perm_pvals (sort + searchsorted) and regression._feature_scale against the helper's direct
    counts, ties included."""
    from pypyls_amd import regression as reg
    rs = np.random.RandomState(3)
    B, T, n, S = 40, 3, 25, 12
    obs, perms = rs.randn(B, T), rs.randn(n, B, T)
    perms[4, 7] = obs[7]                                       # an exact tie counts (>=)
    X = rs.randn(S, B)
    X[5] = np.nan
    okx = ~np.isnan(X).all(axis=1)
    Xc = X - np.nanmean(X, axis=0)
    scale = np.sqrt(np.sum(Xc[okx] ** 2, axis=0) / (okx.sum() - 1))
    assert max_rel(reg._feature_scale(X, okx, Xc), scale) <= 1e-15
    assert max_rel(reg._feature_scale(X[okx], np.ones(S - 1, bool)), scale) <= 1e-14
    want = pvals_of(obs, perms, scale)
    got = reg._coef_perm_pvals(obs, want['count'], want['coefs_max'], scale)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key


def test_a_feature_without_variance_has_p_one_in_both_arrays():
    rs = np.random.RandomState(5)
    S, B, T, k, c, n = 30, 20, 2, 3, 2, 12
    X, Y = rs.randn(S, B), rs.randn(S, T)
    X[:, 6] = 0.0
    perms = np.stack([rs.permutation(S) for _ in range(n)], axis=1)
    want = coef_perm_expected(X, Y, perms, k, c)
    assert np.all(want['coefs'][6] == 0.0) and np.all(want['perms'][:, 6] == 0.0)
    assert np.all(want['coefs_pvals'][6] == 1.0) and np.all(want['coefs_pvals_fwe'][6] == 1.0)
    assert want['coefs_pvals'].min() < 1.0              # (... and only there by construction: the others vary)


def test_stack_helper_counts_and_maxima():
    rs = np.random.RandomState(2)
    Xc = rs.randn(9, 5)
    Xc -= Xc.mean(axis=0)
    stack, obs = rs.randn(4, 2, 9), rs.randn(5, 2)
    coef = np.stack([Xc.T @ stack[b].T for b in range(4)])
    for std in (0, 1):
        s = Xc.std(axis=0, ddof=1) if std else np.ones(5)
        count, mx = stack_test(Xc, stack, obs, std)
        assert np.array_equal(count, (s[None, :, None] * np.abs(coef) >= s[None, :, None] * np.abs(obs)[None]).sum(axis=0))
        assert max_rel(mx, (s[None, :, None] * np.abs(coef)).max(axis=1)) <= 1e-14


def test_validation_errors_come_before_any_engine(monkeypatch):
    import pypyls_amd as pls
    from pypyls_amd import engine
    made = []
    monkeypatch.setattr(engine, 'default_engine', lambda *a, **k: made.append(1))
    monkeypatch.setattr(engine.Engine, '__init__', lambda self, *a, **k: made.append(1))
    rs = np.random.RandomState(0)
    X, Y = rs.randn(20, 30), rs.randn(20, 3)
    kw = dict(n_components=4, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match='coef_perm.*coef_components'):
        pls.pls_regression(X, Y, coef_perm=True, n_perm=10, **kw)
    with pytest.raises(ValueError, match='coef_perm.*n_perm'):
        pls.pls_regression(X, Y, coef_components=2, coef_perm=True, n_perm=0, **kw)
    with pytest.raises(ValueError, match='coef_perm'):
        pls.pls_regression(X, Y, coef_components=2, coef_perm='yes', n_perm=10, **kw)
    assert not made


def test_records_declare_the_new_surface():
    from pypyls_amd import structures as st
    assert set(KEYS) <= set(st.PLSPermResults.allowed) and 'coef_perm' in st.PLSInputs.allowed
    assert 'coef_perm' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1, coef_components=1)
    assert st.PLSInputs(X=np.zeros((2, 2)), n_components=1, coef_components=1, coef_perm=True).coef_perm is True
    import inspect
    import pypyls_amd as pls
    assert inspect.signature(pls.pls_regression).parameters['coef_perm'].default is False
    assert '>=' in pls.pls_regression.__doc__ and 'coefs_pvals_fwe' in pls.pls_regression.__doc__


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
    for meth in ('simpls_coef_perm_test', 'simpls_coef_perm_begin', 'simpls_coef_perm_end'):
        assert callable(getattr(engine.Engine, meth))


def test_save_load_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g, f = load_golden('simpls_coef_a'), load_golden('simpls_coef_perm_a')
    k, c = int(g['n_components']), int(g['coef_components'])
    res = PLSResults(x_weights=np.zeros((g['X'].shape[1], k)), inputs=dict(X=g['X'], Y=g['Y'], n_components=k,
                                                                           coef_components=c, coef_perm=True))
    want = dict(coefs_pvals=f['ref_pvals'], coefs_max=f['ref_max'], coefs_pvals_fwe=f['ref_pvals_fwe'])
    res['permres'].update(want)
    back = pls.load_results(pls.save_results(str(tmp_path / 'coef_perm'), res))
    assert bool(back.inputs.coef_perm) is True and int(back.inputs.coef_components) == c
    for key in KEYS:
        assert np.array_equal(back.permres[key], want[key]) and back.permres[key].shape == want[key].shape, key
