"""behavioral_pls / meancentered_pls(weights_ci=m) without a device: the expectation helpers of
tests/weights_ci_expect.py against a brute-force loop, validation before any engine exists, `inputs` bookkeeping, the
HDF5 round trip of `bootres.x_weights_ci`, the two entries in header, engine and library."""
import os
import re

import numpy as np
import pytest

from oracle import cpu_ref as ref
import weights_ci_expect as wx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('plsx_boot_keep', 'plsx_boot_weights_ci')


def _design(method, seed=0, covariance=False):
    """The 12 x 9 design: two groups of 3 x two conditions."""
    rs = np.random.RandomState(seed)
    spec = wx.spec_of(method, [3, 3], 2, covariance=covariance, mean_centering=0)
    X = rs.randn(12, 9) + 2.0
    Y = rs.randn(12, 2) if method == 'behavioral' else None
    rows = wx.within_cell_rows(spec, 7, rs)
    return spec, X, Y, rows, rs


@pytest.mark.parametrize('method,covariance', [('behavioral', False), ('behavioral', True), ('meancentered', False)])
def test_expectation_helpers_against_a_brute_force_loop(method, covariance):
    spec, X, Y, rows, rs = _design(method, covariance=covariance)
    U, d = wx.original(spec, X, Y)
    Yo = spec.dummy if Y is None else Y
    # weights_boot: single_boot bootstrap by bootstrap
    boot = wx.weights_boot(spec, X, Y, rows.T, U, d)
    B, L = U.shape
    assert boot.shape == (B, L, len(rows))
    for i, r in enumerate(rows):
        want = ref.single_boot(spec, X, Yo, r, U, d)[1]
        assert np.allclose(boot[:, :, i], want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    # ci_of: element by element, and the replication trick
    for ci in (95, 80):
        got = wx.ci_of(boot, ci)
        assert got.shape == (B, L, 2)
        for f in range(B):
            for l in range(L):
                lo, hi = np.percentile(boot[f, l], [(100 - ci) / 2, 100 - (100 - ci) / 2])
                assert got[f, l, 0] == lo and got[f, l, 1] == hi
        assert np.all(got[..., 0] <= got[..., 1])
    w = np.array([3, 1, 2, 1, 1, 4, 2])
    rep = np.concatenate([np.repeat(boot[:, :, i:i + 1], k, axis=-1) for i, k in enumerate(w)], axis=-1)
    assert np.array_equal(wx.ci_of(boot, 90, weights=w), wx.ci_of(rep, 90))
    # stack_ci: R_b^T M_b^T with R_b of the gathered rows, entry by entry
    M = rs.randn(len(rows), 2, spec.dummy.shape[1] * (2 if Y is not None else 1))
    series = wx.stack_series(spec, X, Y, rows, M)
    assert series.shape == (B, 2, len(rows))
    for i, r in enumerate(rows):
        R = ref.gen_covcorr(spec, X[r], Yo[r], spec.dummy)
        for f in range(B):
            for l in range(2):
                want = sum(R[t, f] * M[i, l, t] for t in range(R.shape[0]))
                assert abs(series[f, l, i] - want) <= 1e-12 * max(1.0, np.abs(R).max() * np.abs(M).max() * R.shape[0])
    assert np.array_equal(wx.stack_ci(spec, X, Y, rows, M, 80), wx.ci_of(series, 80))
    # with the rotation operand of the bootstrap's own decomposition the closing entry's series IS weights_boot:
    # U_b = R_b^T M_b, M_b = V_b P N^T of procrustes_live (full rank here)
    if method != 'behavioral':
        return
    full = np.stack([np.concatenate([rs.permutation(np.flatnonzero(c)) for c in spec.dummy.T.astype(bool)])
                     for _ in range(3)])                      # (index rows that keep every cell's three subjects)
    Ms = []
    for r in full:
        Ub, db, Vb = ref.decompose(spec, X[r], Yo[r])
        assert ref.live_lvs(db).all()
        N, _, P = np.linalg.svd(U.T @ Ub, full_matrices=False)
        Ms.append((Vb @ P.T @ N.T).T)
    own = wx.stack_series(spec, X, Y, full, np.stack(Ms))
    want = wx.weights_boot(spec, X, Y, full.T, U, d)
    assert np.allclose(own, want, rtol=0, atol=1e-9 * np.abs(want).max())


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
    kw = dict(groups=[6, 6], n_cond=2, n_perm=0, verbose=False)          # T' = 8 = L
    with pytest.raises(ValueError, match='n_boot'):
        pls.behavioral_pls(X, Y, weights_ci=True, n_boot=0, **kw)
    with pytest.raises(ValueError, match='16384'):
        pls.behavioral_pls(X, Y, weights_ci=True, n_boot=16385, **kw)
    for bad in (0, 9, -1, 2.0, 'all'):
        with pytest.raises(ValueError, match='weights_ci'):
            pls.behavioral_pls(X, Y, weights_ci=bad, n_boot=10, **kw)
    with pytest.raises(ValueError, match='weights_ci'):
        pls.behavioral_pls(X, Y, weights_ci=2, n_boot=10, contrasts=np.linalg.qr(rs.randn(8, 2))[0], **kw)
    with pytest.raises(ValueError, match='weights_ci'):
        pls.meancentered_pls(X, weights_ci=True, n_boot=10, contrasts=np.linalg.qr(rs.randn(4, 2))[0], **kw)
    with pytest.raises(ValueError, match='weights_ci'):
        pls.meancentered_pls(X, weights_ci=5, n_boot=10, **kw)              # L = 4 cells
    with pytest.raises(ValueError, match='n_boot'):
        pls.meancentered_pls(X, weights_ci=True, n_boot=0, **kw)
    with pytest.raises(ValueError, match='multiblock'):
        pls.multiblock_pls(X, Y, weights_ci=True, n_boot=10, **kw)
    # L is bounded by B as well: 3 features
    with pytest.raises(ValueError, match='weights_ci'):
        pls.behavioral_pls(X[:, :3], Y, weights_ci=4, n_boot=10, **kw)
    # the number of bootstraps of a supplied array counts
    with pytest.raises(ValueError, match='16384'):
        pls.behavioral_pls(X, Y, weights_ci=True, n_boot=10, bootsamples=np.zeros((24, 16385), dtype=int), **kw)
    # valid calls get past the checks and only then ask for an engine
    for ok in (True, 1, 8, np.int64(3)):
        with pytest.raises(AssertionError, match='engine'):
            pls.behavioral_pls(X, Y, weights_ci=ok, n_boot=16384, **kw)
    with pytest.raises(AssertionError, match='engine'):
        pls.meancentered_pls(X, weights_ci=4, n_boot=10, **kw)


def test_inputs_hold_the_key_only_when_given():
    from pypyls_amd import structures as st
    from pypyls_amd.plsc import _PLSCRun
    assert 'weights_ci' in st.PLSInputs.allowed and 'x_weights_ci' in st.PLSBootResults.allowed
    rs = np.random.RandomState(2)
    X, Y = rs.randn(12, 9), rs.randn(12, 2)
    run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=0, n_boot=5, weights_ci=True)
    assert run.inputs['weights_ci'] is True and run.weights_m == 4
    run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=0, n_boot=5, weights_ci=3)
    assert run.inputs['weights_ci'] == 3 and run.weights_m == 3
    for kw in ({}, {'weights_ci': False}):
        run = _PLSCRun('behavioral', X, Y, groups=[6], n_cond=2, n_perm=0, n_boot=5, **kw)
        assert 'weights_ci' not in run.inputs and run.weights_m is None


def test_header_engine_and_library_carry_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'plsx.h')).read()
    assert re.search(r'\bint plsx_boot_keep\s*\(plsx_ctx\* ctx, double\* d_M, long long capacity, int m\)', hdr)
    assert re.search(r'\bint plsx_boot_weights_ci\s*\(plsx_ctx\* ctx, const int32_t\* d_boot_idx, const double\* d_M, '
                     r'int n, int m,', hdr)
    src = open(os.path.join(ROOT, 'pypyls_amd', 'engine.py')).read()
    for name in ENTRIES:
        assert src.count("'{}'".format(name)) >= 2
    from pypyls_amd import _build, engine
    if os.path.exists(_build.lib_path()):
        assert set(ENTRIES) <= set(engine.exported_symbols())
        lib = engine._load()
        names, i = [], 0
        while lib.plsx_kernel_class_name(i):
            names.append(lib.plsx_kernel_class_name(i).decode())
            i += 1
        assert 'k_weights_prod' in names, names
    for meth in ('boot_keep', 'boot_weights_ci'):
        assert callable(getattr(engine.Engine, meth))
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        assert name in doc


def test_save_load_round_trip_keeps_the_intervals(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    spec, X, Y, rows, rs = _design('behavioral', seed=4)
    want = wx.weights_ci_expected(spec, X, Y, rows.T, m=3)
    U, d = wx.original(spec, X, Y)
    res = PLSResults(x_weights=U, singvals=np.diag(d), bootres=dict(x_weights_ci=want, bootsamples=rows.T),
                     inputs=dict(X=X, Y=Y, groups=[3, 3], n_cond=2, n_boot=7, weights_ci=3))
    back = pls.load_results(pls.save_results(str(tmp_path / 'wci'), res))
    assert np.array_equal(back.bootres.x_weights_ci, want) and back.bootres.x_weights_ci.shape == (9, 3, 2)
    assert int(back.inputs.weights_ci) == 3
