"""behavioral_pls / meancentered_pls(weights_perm=m): everything that needs no GPU -- the argument checks come before any
engine, the expectation the GPU tests rest on (tests/weights_perm_expect.py) is the rotated permuted weights where the
rotation is exact and reproduces the observed statistic under the identity, the keyword is recorded only when given, the
new entries exist in the header, the ctypes table and the Engine, and the three keys survive save / load."""
import os
import re

import numpy as np
import pytest

import weights_perm_expect as wp
from oracle import cpu_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('plsx_perm_weights_build', 'plsx_perm_weights_test', 'plsx_perm_weights_scale')


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
    kw = dict(groups=[6, 6], n_cond=2, n_boot=0, verbose=False)          # T' = 8 = L
    with pytest.raises(ValueError, match='n_perm'):
        pls.behavioral_pls(X, Y, weights_perm=True, n_perm=0, **kw)
    with pytest.raises(ValueError, match='n_perm'):
        pls.meancentered_pls(X, weights_perm=True, n_perm=0, **kw)
    with pytest.raises(ValueError, match='permindices'):
        pls.behavioral_pls(X, Y, weights_perm=True, n_perm=3, permindices=False, permsamples=rs.randn(3, 24, 2), **kw)
    with pytest.raises(ValueError, match='multiblock'):
        pls.multiblock_pls(X, Y, weights_perm=True, n_perm=10, **kw)
    for bad in (0, 9, -1, 2.0, 'all'):
        with pytest.raises(ValueError, match='weights_perm'):
            pls.behavioral_pls(X, Y, weights_perm=bad, n_perm=10, **kw)
    with pytest.raises(ValueError, match='weights_perm'):
        pls.meancentered_pls(X, weights_perm=5, n_perm=10, **kw)            # L = 4 cells
    # L is bounded by B as well: 3 features
    with pytest.raises(ValueError, match='weights_perm'):
        pls.behavioral_pls(X[:, :3], Y, weights_perm=4, n_perm=10, **kw)
    # with contrasts L is their number
    with pytest.raises(ValueError, match='weights_perm'):
        pls.behavioral_pls(X, Y, weights_perm=3, n_perm=10, contrasts=np.linalg.qr(rs.randn(8, 2))[0], **kw)
    # valid calls get past the checks and only then ask for an engine
    for ok in (True, 1, 8, np.int64(3)):
        with pytest.raises(AssertionError, match='engine'):
            pls.behavioral_pls(X, Y, weights_perm=ok, n_perm=10, **kw)
    with pytest.raises(AssertionError, match='engine'):
        pls.behavioral_pls(X, Y, weights_perm=2, n_perm=10, contrasts=np.linalg.qr(rs.randn(8, 2))[0], **kw)
    with pytest.raises(AssertionError, match='engine'):
        pls.meancentered_pls(X, weights_perm=4, n_perm=10, **kw)
    with pytest.raises(AssertionError, match='engine'):
        pls.behavioral_pls(X, Y, weights_perm=True, n_perm=5, permsamples=wp.random_perms(24, 7, rs), **kw)


def test_inputs_hold_the_key_only_when_given():
    from pypyls_amd import structures as st
    from pypyls_amd.plsc import _PLSCRun
    assert 'weights_perm' in st.PLSInputs.allowed
    for key in ('x_weights_pvals', 'x_weights_max', 'x_weights_pvals_fwe'):
        assert key in st.PLSPermResults.allowed
    rs = np.random.RandomState(2)
    X, Y = rs.randn(12, 9), rs.randn(12, 2)
    run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=5, n_boot=0, weights_perm=True)
    assert run.inputs['weights_perm'] is True and run.wperm_m == 4
    run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=5, n_boot=0, weights_perm=3)
    assert run.inputs['weights_perm'] == 3 and run.wperm_m == 3
    for kw in ({}, {'weights_perm': False}):
        run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=5, n_boot=0, **kw)
        assert 'weights_perm' not in run.inputs and run.wperm_m is None


@pytest.mark.parametrize('method,covariance', [('behavioral', False), ('behavioral', True)])
def test_null_is_the_rotated_permuted_weights_where_the_rotation_is_exact(method, covariance):
    """L = T' = 6 <= B and full rank: Z_p = U_p d_p Q_p with Q_p the Procrustes rotation of the permutation leg (the
    polar factor of V0.T @ V_p, cpu_ref.procrustes), and its column norms are the rotated perm_singval of single_perm."""
    groups, n_cond, T, B = [7, 9], 1, 3, 40
    S = sum(groups) * n_cond
    rs = np.random.RandomState(5)
    X, Y = rs.randn(S, B), rs.randn(S, T)
    spec = wp.spec_of(method, groups, n_cond, covariance=covariance)
    Z, V0 = wp.observed(spec, X, Y)
    assert V0.shape == (6, 6)
    perms = wp.random_perms(S, 4, rs)
    Zp = wp.null(spec, X, Y, perms, V0)
    for p in range(perms.shape[1]):
        Xp, Yp = ref.make_permutation(spec, X, Y, perms[:, p])
        Up, dp, Vp = ref.decompose(spec, Xp, Yp)
        N, _, P = np.linalg.svd(V0.T @ Vp, full_matrices=False)
        rotated = Up @ dp @ (P.T @ N.T)                                         # (B, L)
        assert np.allclose(ref.procrustes(V0, Vp, dp), Vp @ dp @ (P.T @ N.T), rtol=0, atol=1e-12)
        for l in range(6):
            err = min(np.abs(Zp[:, l, p] - s * rotated[:, l]).max() for s in (1.0, -1.0)) / np.abs(Zp[:, :, p]).max()
            assert err <= 1e-10, (p, l, err)
        ssd = ref.single_perm(spec, X, Y, perms[:, p], V0)[0]
        assert np.allclose(np.sqrt((Zp[:, :, p] ** 2).sum(axis=0)), ssd, rtol=1e-10, atol=0)


@pytest.mark.parametrize('method,covariance,mc,contrasts', [
    ('behavioral', False, 0, False), ('behavioral', True, 0, False), ('behavioral', False, 0, True),
    ('meancentered', False, 0, False), ('meancentered', False, 1, False), ('meancentered', False, 2, False)])
def test_identity_permutation_reproduces_the_observed_statistic(method, covariance, mc, contrasts):
    groups, n_cond, T, B = [8, 6], 2, 2, 25
    S = sum(groups) * n_cond
    rs = np.random.RandomState(9)
    X = rs.randn(S, B) * (1.0 + 3.0 * rs.rand(B)) + np.repeat(rs.randn(4, B), np.repeat(groups, n_cond), axis=0)
    Y = None if method == 'meancentered' else rs.randn(S, T)
    spec = wp.spec_of(method, groups, n_cond, covariance=covariance, mean_centering=mc)
    Tp = 4 if method == 'meancentered' else 8
    C = np.linalg.qr(rs.randn(Tp, 3))[0] if contrasts else None
    Z, V0 = wp.observed(spec, X, Y, C)
    live = ref.live_lvs(np.sqrt((Z ** 2).sum(axis=0)))
    Zp = wp.null(spec, X, Y, np.arange(S)[:, None], V0)[:, :, 0]
    err = np.abs(Zp - Z)[:, live].max() / np.abs(Z).max()
    assert err <= 1e-12, err
    # ... and through the subject-space form the device uses: Z_p = W_p @ Xf needs Xf alone from the features
    st = wp.statistics(Z[:, live], Zp[:, live, None], wp.feature_scale(spec, X))
    assert st['count'].min() >= 0 and st['max'].shape == (int(live.sum()), 1)


def test_statistics_against_a_brute_force_loop():
    rs = np.random.RandomState(3)
    B, m, n = 17, 3, 11
    Z, Zp, q = rs.randn(B, m), rs.randn(B, m, n), 1.0 / (0.5 + rs.rand(B))
    q[4] = 0.0                                                                   # a feature without variance
    Z[4], Zp[4] = 0.0, 0.0
    st = wp.statistics(Z, Zp, q)
    for f in range(B):
        for l in range(m):
            c = sum(abs(Zp[f, l, p]) >= abs(Z[f, l]) for p in range(n))
            assert st['count'][f, l] == c and st['pvals'][f, l] == (c + 1) / (n + 1)
            mx = [max(q[g] * abs(Zp[g, l, p]) for g in range(B)) for p in range(n)]
            assert np.array_equal(st['max'][l], mx)
            cf = sum(mx[p] >= q[f] * abs(Z[f, l]) for p in range(n))
            assert st['pvals_fwe'][f, l] == (cf + 1) / (n + 1)
    assert (st['pvals'][4] == 1).all() and (st['pvals_fwe'][4] == 1).all()
    assert st['closeness'] > 0
    from pypyls_amd.plsc import _weights_perm_pvals
    own = _weights_perm_pvals(q[:, None] * np.abs(Z), st['count'], st['max'])
    assert np.array_equal(own['x_weights_pvals'], st['pvals']) and np.array_equal(own['x_weights_pvals_fwe'], st['pvals_fwe'])
    assert own['x_weights_max'] is st['max']


def test_header_engine_and_library_carry_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'plsx.h')).read()
    assert re.search(r'\bint plsx_perm_weights_build\s*\(plsx_ctx\* ctx, const int32_t\* d_perm_idx, int n, '
                     r'const double\* d_V, int m, double\* d_W,', hdr)
    assert re.search(r'\bint plsx_perm_weights_test\s*\(plsx_ctx\* ctx, const int32_t\* d_perm_idx, int n, '
                     r'const double\* d_V, int m, const double\* d_obs,\s+int standardise, int32_t\* d_count, '
                     r'double\* d_max, void\* stream\)', hdr)
    src = open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')).read()
    for name in ENTRIES:
        assert src.count("'{}'".format(name)) >= 2
    from pypyls_amd import _build, engine
    if os.path.exists(_build.lib_path()):
        assert set(ENTRIES) <= set(engine.exported_symbols())
    for meth in ('perm_weights_build', 'perm_weights_test', 'perm_weights_scale'):
        assert callable(getattr(engine.Engine, meth))
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES[:2]:
        assert name in doc


def test_save_load_round_trip_keeps_the_three_keys(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    groups, n_cond, T, B = [5, 4], 1, 2, 9
    S = sum(groups)
    rs = np.random.RandomState(4)
    X, Y = rs.randn(S, B), rs.randn(S, T)
    spec = wp.spec_of('behavioral', groups, n_cond)
    perms = wp.random_perms(S, 7, rs)
    want = wp.expected(spec, X, Y, perms, m=3)
    res = PLSResults(singvals=np.ones(4), permres=dict(
        x_weights_pvals=want['pvals'], x_weights_max=want['max'], x_weights_pvals_fwe=want['pvals_fwe'],
        permsamples=perms), inputs=dict(X=X, Y=Y, groups=groups, n_cond=n_cond, n_perm=7, weights_perm=3))
    back = pls.load_results(pls.save_results(str(tmp_path / 'wperm'), res))
    assert np.array_equal(back.permres.x_weights_pvals, want['pvals']) and back.permres.x_weights_pvals.shape == (B, 3)
    assert np.array_equal(back.permres.x_weights_max, want['max']) and back.permres.x_weights_max.shape == (3, 7)
    assert np.array_equal(back.permres.x_weights_pvals_fwe, want['pvals_fwe'])
    assert int(back.inputs.weights_perm) == 3
