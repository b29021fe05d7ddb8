"""pls_regression(coef_components=c, coef_ci=True) on the host (no GPU): the oracle helper against the fixtures the
reference's ``simpls(...)['beta']`` wrote (tests/golden/make_coef_ci_golden.py), validation before any engine exists,
the records, persistence, the header and the built library."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from regression_coef_expect import max_rel
from regression_coef_ci_expect import coef_boot, ci_of, coef_ci_expected, stack_ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ['a', 'nan', 'y3d']
PIN = 1e-10            # helper vs reference fixtures (the generator measured 6.1e-15 at worst)
ENTRIES = ('plsx_simpls_coef_keep', 'plsx_simpls_coef_ci')


@pytest.mark.parametrize('tag', TAGS)
def test_helper_reproduces_the_reference_fixtures(tag):
    g, f = load_golden('simpls_coef_' + tag), load_golden('simpls_coef_ci_' + tag)
    k, c, aggfunc = int(g['n_components']), int(g['coef_components']), str(g['aggfunc'])
    B, T = g['X'].shape[1], g['Y'].shape[1]
    assert f['ref_ci'].shape == (len(f['ci']), B, T, 2) and list(f['ci']) == [95, 80]
    boot = coef_boot(g['X'], g['Y'], g['bootsamples'], k, c, aggfunc=aggfunc, third=g.get('third'))
    assert boot.shape == (g['bootsamples'].shape[1], B, T)
    for i, level in enumerate(f['ci']):
        want = ci_of(boot, ci=level)
        err = max_rel(want, f['ref_ci'][i])
        print('simpls_coef_ci_{} ci={:g}: oracle vs reference {:.3e}'.format(tag, level, err))
        assert err <= PIN, (tag, level, err)
        assert np.all(want[..., 0] <= want[..., 1])
    # the two levels nest, and the series are those coefs_stderr is built from: their sums are the fixture's
    assert np.all(f['ref_ci'][0][..., 0] <= f['ref_ci'][1][..., 0]) and np.all(f['ref_ci'][1][..., 1] <= f['ref_ci'][0][..., 1])
    assert max_rel(boot.sum(axis=0), g['ref_bsum']) <= PIN and max_rel((boot ** 2).sum(axis=0), g['ref_bsq']) <= PIN


def test_helper_weights_and_stack_form():
    """Replication counts repeat the matrices; the subject-space form (Xc^T A_b) gives the same series."""
    rs = np.random.RandomState(1)
    boot = rs.randn(5, 7, 3)
    w = np.array([3, 1, 2, 1, 4])
    assert np.array_equal(ci_of(boot, 90, weights=w), ci_of(np.repeat(boot, w, axis=0), 90))
    Xc, stack = rs.randn(11, 7), rs.randn(5, 3, 11)
    want = ci_of(np.stack([Xc.T @ stack[b].T for b in range(5)]), 80)
    assert max_rel(stack_ci(Xc, stack, 80), want) <= 1e-14


def test_validation_errors_come_before_any_engine(monkeypatch):
    import pypyls_amd as pls
    from pypyls_amd import engine
    made = []
    monkeypatch.setattr(engine, 'default_engine', lambda *a, **k: made.append(1))
    monkeypatch.setattr(engine.Engine, '__init__', lambda self, *a, **k: made.append(1))
    rs = np.random.RandomState(0)
    X, Y = rs.randn(20, 30), rs.randn(20, 3)
    kw = dict(n_components=4, n_perm=0, verbose=False)
    with pytest.raises(ValueError, match='coef_ci.*coef_components'):
        pls.pls_regression(X, Y, coef_ci=True, n_boot=10, **kw)
    with pytest.raises(ValueError, match='coef_ci.*n_boot'):
        pls.pls_regression(X, Y, coef_components=2, coef_ci=True, n_boot=0, **kw)
    with pytest.raises(ValueError, match='16384.*no host fallback'):
        pls.pls_regression(X, Y, coef_components=2, coef_ci=True, n_boot=16385, **kw)
    with pytest.raises(ValueError, match='coef_ci'):
        pls.pls_regression(X, Y, coef_components=2, coef_ci='yes', n_boot=10, **kw)
    assert not made


def test_records_declare_the_new_surface():
    from pypyls_amd import structures as st
    assert 'coefs_ci' in st.PLSBootResults.allowed and 'coef_ci' in st.PLSInputs.allowed
    # a record that was not given the keyword holds no trace of it
    assert 'coef_ci' not in st.PLSInputs(X=np.zeros((2, 2)), n_components=1, coef_components=1)
    assert st.PLSInputs(X=np.zeros((2, 2)), n_components=1, coef_components=1, coef_ci=True).coef_ci is True
    import inspect
    import pypyls_amd as pls
    assert inspect.signature(pls.pls_regression).parameters['coef_ci'].default is False


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
    names, i = [], 0
    lib = engine._load()
    while lib.plsx_kernel_class_name(i):
        names.append(lib.plsx_kernel_class_name(i).decode())
        i += 1
    assert {'k_coef_prod', 'k_percentile'} <= set(names), names
    for meth in ('simpls_coef_keep', 'simpls_coef_ci'):
        assert callable(getattr(engine.Engine, meth))


def test_save_load_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g = load_golden('simpls_coef_a')
    k, c = int(g['n_components']), int(g['coef_components'])
    want = coef_ci_expected(g['X'], g['Y'], g['bootsamples'], k, c, ci=90)
    res = PLSResults(x_weights=np.zeros((g['X'].shape[1], k)), inputs=dict(X=g['X'], Y=g['Y'], n_components=k, ci=90,
                                                                           coef_components=c, coef_ci=True))
    res['bootres']['coefs_ci'] = want
    back = pls.load_results(pls.save_results(str(tmp_path / 'coef_ci'), res))
    assert bool(back.inputs.coef_ci) is True and int(back.inputs.coef_components) == c
    assert np.array_equal(back.bootres.coefs_ci, want) and back.bootres.coefs_ci.shape == want.shape
