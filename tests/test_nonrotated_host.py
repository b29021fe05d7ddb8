"""Non-rotated PLS (``contrasts=``) without a GPU: the numpy definition (tests/nonrotated_expect.py) against the SVD it
must reproduce when the contrasts are the SVD's own y_weights, validation before any engine exists, the warning for
non-orthogonal contrasts, the inputs record, the header and the exported symbol, persistence."""
import os
import re
import warnings

import numpy as np
import pytest

from conftest import load_golden, ROOT
from oracle import cpu_ref as ref
import nonrotated_expect as nr

CASES = [('bpls_2g2c', 'behavioral'), ('bpls_2g2c_cov', 'behavioral'), ('bpls_1g3c', 'behavioral'),
         ('mpls_3g2c_mc0', 'meancentered'), ('mpls_3g2c_mc1', 'meancentered'), ('mpls_3g2c_mc2', 'meancentered')]


def _spec(g, method):
    return nr.spec_of(method, list(g['groups']), int(g['n_cond']), bool(g.get('covariance', False)),
                      int(g.get('mean_centering', 0)))


@pytest.mark.parametrize('name,method', CASES)
def test_contrasts_equal_to_the_svd_weights_reproduce_the_svd(name, method):
    g = load_golden(name)
    spec = _spec(g, method)
    X = g['X']
    Y = g['Y'] if method == 'behavioral' else spec.dummy
    U, d, V = ref.decompose(spec, X, Y)
    d = np.diag(d)
    live = d > 1e-8 * d.max()
    xw, sv, yw = nr.original(spec, X, Y, V[:, live])
    assert np.abs(sv - d[live]).max() <= 1e-13 * d.max()
    assert np.abs(xw - U[:, live]).max() <= 1e-12
    assert np.abs(yw - V[:, live]).max() <= 1e-15
    # ... and the permuted statistic of a contrast is the norm of its projection: never above the largest singular value
    perms = g['ref_permres__permsamples'][:, :5]
    sp = nr.perm_singvals(spec, X, Y, yw, perms)
    for i in range(perms.shape[1]):
        Xp, Yp = ref.make_permutation(spec, X, Y, perms[:, i])
        top = np.linalg.svd(ref.gen_covcorr(spec, Xp, Yp, spec.dummy), compute_uv=False)[0]
        assert np.all(sp[:, i] <= top * (1 + 1e-12))


def _no_engine(monkeypatch):
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was created or looked up before the arguments were checked')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def test_validation_errors_come_before_any_engine(monkeypatch):
    import pypyls_amd as pls
    _no_engine(monkeypatch)
    rs = np.random.RandomState(0)
    X, Y = rs.randn(24, 30), rs.randn(24, 2)
    kw = dict(groups=[6, 6], n_cond=2, n_perm=0, n_boot=0, verbose=False)
    good = rs.randn(8, 3)
    bad = {'not 2-D': good[:, 0], 'rows': rs.randn(7, 3), 'no column': np.zeros((8, 0)), 'too many': rs.randn(8, 9),
           'nan': np.where(np.arange(24).reshape(8, 3) == 4, np.nan, good),
           'inf': np.where(np.arange(24).reshape(8, 3) == 4, np.inf, good),
           'zero column': good * np.array([1.0, 0.0, 1.0])}
    for what, C in bad.items():
        with pytest.raises(ValueError):
            pls.behavioral_pls(X, Y, contrasts=C, **kw)
            pytest.fail('accepted contrasts with: ' + what)
    with pytest.raises(ValueError, match='n_split'):
        pls.behavioral_pls(X, Y, contrasts=good, n_split=5, **kw)
    # Lc is bounded by B as well: 3 features, 4 contrasts
    with pytest.raises(ValueError):
        pls.behavioral_pls(X[:, :3], Y, contrasts=rs.randn(8, 4), **kw)
    # mean-centred: T' = groups x conditions
    mkw = dict(groups=[6, 6], n_cond=2, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError):
        pls.meancentered_pls(X, contrasts=rs.randn(8, 2), **mkw)
    with pytest.raises(ValueError, match='n_split'):
        pls.meancentered_pls(X, contrasts=rs.randn(4, 2), n_split=3, **mkw)
    # a valid call gets past the checks and only then asks for an engine
    with pytest.raises(AssertionError, match='engine'):
        pls.meancentered_pls(X, contrasts=np.linalg.qr(rs.randn(4, 2))[0], **mkw)


def test_non_orthogonal_contrasts_warn_once_orthogonal_ones_do_not(monkeypatch):
    import pypyls_amd as pls
    _no_engine(monkeypatch)
    rs = np.random.RandomState(1)
    X = rs.randn(24, 30)
    kw = dict(groups=[6, 6], n_cond=2, n_perm=0, n_boot=0, verbose=False)
    skew = np.array([[1.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [0.0, 0.0]])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        with pytest.raises(AssertionError, match='engine'):
            pls.meancentered_pls(X, contrasts=skew, **kw)
    assert len([w for w in rec if 'not orthogonal' in str(w.message)]) == 1
    ortho = np.array([[1.0, 1.0], [-1.0, 1.0], [1.0, -1.0], [-1.0, -1.0]]) * 3.0     # (scale is normalised away)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        with pytest.raises(AssertionError, match='engine'):
            pls.meancentered_pls(X, contrasts=ortho, **kw)
    assert not [w for w in rec if 'not orthogonal' in str(w.message)]


def test_inputs_hold_the_key_only_when_given():
    from pypyls_amd import structures as st
    from pypyls_amd.plsc import _PLSCRun
    assert 'contrasts' in st.PLSInputs.allowed
    rs = np.random.RandomState(2)
    X, Y = rs.randn(12, 9), rs.randn(12, 2)
    C = np.linalg.qr(rs.randn(4, 2))[0] * 2.0
    run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=0, n_boot=0, contrasts=C)
    assert np.array_equal(run.inputs['contrasts'], C)          # the caller's, not the normalised copy
    assert np.allclose(run.V, C / 2.0, rtol=0, atol=1e-15)
    for kw in ({}, {'contrasts': None}):
        run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=0, n_boot=0, **kw)
        assert 'contrasts' not in run.inputs and run.V is None


def test_header_declares_and_library_exports_the_entry():
    hdr = open(os.path.join(ROOT, 'include', 'plsx.h')).read()
    assert re.search(r'\bint plsx_set_contrasts\s*\(plsx_ctx\* ctx, const double\* d_C, int Lc, void\* stream\)', hdr)
    src = open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')).read()
    assert src.count("'plsx_set_contrasts'") >= 2
    core = open(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_core.hip')).read()
    assert re.search(r'^int plsx_set_contrasts\(', core, re.M)
    from pypyls_amd import _build
    if os.path.exists(_build.lib_path()):
        import ctypes
        assert hasattr(ctypes.CDLL(_build.lib_path()), 'plsx_set_contrasts')
        lib = ctypes.CDLL(_build.lib_path())
        lib.plsx_kernel_class_name.restype = ctypes.c_char_p
        names, i = [], 0
        while lib.plsx_kernel_class_name(i):
            names.append(lib.plsx_kernel_class_name(i).decode())
            i += 1
        assert 'k_contrast' in names, names


def test_save_load_round_trip_keeps_the_contrasts(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    g = load_golden('mpls_3g2c_mc0')
    C = np.linalg.qr(np.random.RandomState(3).randn(6, 2))[0]
    want = nr.run_nonrotated(g['X'], contrasts=C, method='meancentered', groups=list(g['groups']),
                             n_cond=int(g['n_cond']), permsamples=g['ref_permres__permsamples'][:, :4])
    res = PLSResults(x_weights=want['x_weights'], y_weights=want['y_weights'], singvals=want['singvals'],
                     varexp=want['varexp'], permres=dict(pvals=want['permres']['pvals']),
                     inputs=dict(X=g['X'], groups=list(g['groups']), n_cond=int(g['n_cond']), contrasts=C))
    back = pls.load_results(pls.save_results(str(tmp_path / 'nonrot'), res))
    assert np.array_equal(back.inputs.contrasts, C)
    assert np.array_equal(back.singvals, want['singvals'])
    assert back.x_weights.shape == (g['X'].shape[1], 2)
