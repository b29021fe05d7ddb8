"""pls_regression(vip_components=c, vip_perm=True) on the host (no GPU): the oracle helper against the fixtures the
reference's ``simpls`` wrote (tests/golden/make_vip_perm_golden.py), the front end's p-value formulas on hand-made
counts, validation before any engine exists, the records, persistence, the header and the built library."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from regression_coef_expect import max_rel
from regression_vip_perm_expect import vip_perm_expected, min_rel_gap, pvals_of, stack_series, stack_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ['a', 'nan', 'y3d']
PIN = 1e-10            # helper vs reference fixtures (the generator measured 1.0e-14 at worst)
MIN_GAP = 1e-8         # no count of a fixture is closer to a tie than this
ENTRIES = ('plsx_simpls_vip_perm_test', 'plsx_simpls_vip_perm_begin', 'plsx_simpls_vip_perm_end')
KEYS = ('vip_pvals', 'vip_max', 'vip_pvals_fwe')


@pytest.mark.parametrize('tag', TAGS)
def test_helper_reproduces_the_reference_fixtures(tag):
    g, p, f = load_golden('simpls_coef_' + tag), load_golden('simpls_coef_perm_' + tag), load_golden('simpls_vip_perm_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    B, n = g['X'].shape[1], p['permsamples'].shape[1]
    assert f['ref_count'].shape == (B,) and f['ref_max'].shape == (n,)
    assert f['ref_pvals'].shape == (B,) and f['ref_pvals_fwe'].shape == (B,)
    want = vip_perm_expected(g['X'], g['Y'], p['permsamples'], k, c, aggfunc=aggfunc)
    gaps = min_rel_gap(want['vip'], want['perms'])
    err = max_rel(want['vip_max'], f['ref_max'])
    print('simpls_vip_perm_{}: oracle vs reference vip_max {:.3e}, smallest gaps {:.3e} / {:.3e} (fixture {:.3e})'.format(
        tag, err, gaps[0], gaps[1], float(f['min_gap'])))
    assert np.isfinite(want['perms']).all()                    # (no permuted fit is degenerate)
    assert err <= PIN, (tag, err)
    assert min(gaps) > MIN_GAP and float(f['min_gap']) > MIN_GAP
    assert np.array_equal(want['count'], f['ref_count'])
    assert np.array_equal(want['vip_pvals'], f['ref_pvals'])
    assert np.array_equal(want['vip_pvals_fwe'], f['ref_pvals_fwe'])
    assert max_rel((want['vip'] ** 2).sum(), float(B)) <= 1e-12 and want['vip_max'].min() >= 1.0
    assert np.all(f['ref_pvals_fwe'] >= f['ref_pvals']) and f['ref_pvals'].min() >= 1 / (n + 1) and f['ref_pvals'].max() <= 1


def test_front_end_formulas_on_hand_made_counts():
    """regression._vip_perm_pvals (sort + searchsorted) against the helper's direct counts: an exact tie counts (>=), a
    zero maximum -- what the device leaves for a degenerate permuted fit -- is reported as NaN and counts nowhere, a NaN
    observed score gives NaN in both p-value arrays."""
    from pypyls_amd import regression as reg
    rs = np.random.RandomState(3)
    B, n = 40, 25
    obs, perms = np.abs(rs.randn(B)) + 0.5, np.abs(rs.randn(n, B)) + 0.5
    perms[4, 7] = obs[7]                                       # an exact tie with the feature's own score ...
    obs[9] = perms[6].max()                                    # ... and one with a maximum
    perms[11] = np.nan                                         # a degenerate permuted fit
    obs[3] = np.nan
    want = pvals_of(obs, perms)
    assert np.isnan(want['vip_max'][11]) and np.isnan(want['vip_pvals'][3]) and np.isnan(want['vip_pvals_fwe'][3])
    device_max = np.where(np.isnan(want['vip_max']), 0.0, want['vip_max'])
    got = reg._vip_perm_pvals(obs, want['count'], device_max)
    for key in KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    live = ~np.isnan(obs)
    assert got['vip_pvals'][live].min() >= 1 / (n + 1) and got['vip_pvals'][live].max() <= (n - 1 + 1) / (n + 1)
    assert np.all(got['vip_pvals_fwe'][live] >= got['vip_pvals'][live])
    # by hand: three permutations, two features
    tiny = reg._vip_perm_pvals(np.array([1.5, 0.0]), np.array([1, 3]), np.array([2.0, 1.5, 1.2]))
    assert np.array_equal(tiny['vip_pvals'], [2 / 4, 4 / 4]) and np.array_equal(tiny['vip_pvals_fwe'], [3 / 4, 4 / 4])
    assert np.array_equal(tiny['vip_max'], [2.0, 1.5, 1.2])


def test_a_feature_without_variance_has_p_one_in_both_arrays():
    rs = np.random.RandomState(5)
    S, B, T, k, c, n = 30, 20, 2, 3, 2, 12
    X, Y = rs.randn(S, B), rs.randn(S, T)
    X[:, 6] = 0.0
    perms = np.stack([rs.permutation(S) for _ in range(n)], axis=1)
    want = vip_perm_expected(X, Y, perms, k, c)
    assert want['vip'][6] == 0.0 and np.all(want['perms'][:, 6] == 0.0)
    assert want['vip_pvals'][6] == 1.0 and want['vip_pvals_fwe'][6] == 1.0
    assert want['vip_pvals'].min() < 1.0              # (... and only there by construction: the others vary)


def test_stack_helper_counts_and_maxima():
    rs = np.random.RandomState(2)
    Xc = rs.randn(9, 5)
    Xc -= Xc.mean(axis=0)
    stack, obs = rs.randn(4, 2, 9), np.abs(rs.randn(5)) * 6
    stack[2] = np.nan
    v = np.stack([np.sqrt(5 * ((Xc.T @ stack[b].T) ** 2).sum(axis=1)) for b in range(4)])
    assert max_rel(stack_series(Xc, stack)[[0, 1, 3]], v[[0, 1, 3]]) <= 1e-14 and np.isnan(v[2]).all()
    count, mx = stack_test(Xc, stack, obs)
    assert np.array_equal(count, (v[[0, 1, 3]] >= obs[None]).sum(axis=0))
    assert mx[2] == 0.0 and max_rel(mx[[0, 1, 3]], v[[0, 1, 3]].max(axis=1)) <= 1e-14


def test_validation_errors_come_before_any_engine(monkeypatch):
    import pypyls_amd as pls
    from pypyls_amd import engine
    made = []
    monkeypatch.setattr(engine, 'default_engine', lambda *a, **k: made.append(1))
    monkeypatch.setattr(engine.Engine, '__init__', lambda self, *a, **k: made.append(1))
    rs = np.random.RandomState(0)
    X, Y = rs.randn(20, 30), rs.randn(20, 3)
    kw = dict(n_components=4, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match='vip_perm.*vip_components'):
        pls.pls_regression(X, Y, vip_perm=True, n_perm=10, **kw)
    with pytest.raises(ValueError, match='vip_perm.*n_perm'):
        pls.pls_regression(X, Y, vip_components=2, vip_perm=True, n_perm=0, **kw)
    with pytest.raises(ValueError, match='vip_perm'):
        pls.pls_regression(X, Y, vip_components=2, vip_perm='yes', n_perm=10, **kw)
    with pytest.raises(ValueError, match='vip_perm'):
        pls.pls_regression(X, Y, vip_components=2, vip_perm=1, n_perm=10, **kw)
    with pytest.raises(ValueError, match='vip_perm.*vip_components'):
        pls.pls_da(X, np.arange(20) % 3, vip_perm=True, n_perm=10, **kw)
    assert not made


def test_records_declare_the_new_surface():
    from pypyls_amd import structures as st
    assert set(KEYS) <= set(st.PLSPermResults.allowed) and 'vip_perm' in st.PLSInputs.allowed
    assert 'vip_perm' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1, vip_components=1)
    assert st.PLSInputs(X=np.zeros((2, 2)), n_components=1, vip_components=1, vip_perm=True).vip_perm is True
    import inspect
    import pypyls_amd as pls
    for fn in (pls.pls_regression, pls.pls_da):
        assert inspect.signature(fn).parameters['vip_perm'].default is False
        assert 'vip_pvals_fwe' in fn.__doc__
    assert 'vip_p[f] >= vip[f]' in pls.pls_regression.__doc__


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
    for meth in ('simpls_vip_perm_test', 'simpls_vip_perm_begin', 'simpls_vip_perm_end'):
        assert callable(getattr(engine.Engine, meth))


def test_save_load_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g, f = load_golden('simpls_coef_a'), load_golden('simpls_vip_perm_a')
    k, c = int(g['n_components']), int(g['coef_components'])
    res = PLSResults(x_weights=np.zeros((g['X'].shape[1], k)), inputs=dict(X=g['X'], Y=g['Y'], n_components=k,
                                                                           vip_components=c, vip_perm=True))
    want = dict(vip_pvals=f['ref_pvals'], vip_max=f['ref_max'], vip_pvals_fwe=f['ref_pvals_fwe'])
    res['permres'].update(want)
    back = pls.load_results(pls.save_results(str(tmp_path / 'vip_perm'), res))
    assert bool(back.inputs.vip_perm) is True and int(back.inputs.vip_components) == c
    for key in KEYS:
        assert np.array_equal(back.permres[key], want[key]) and back.permres[key].shape == want[key].shape, key
