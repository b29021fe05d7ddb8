"""Multiblock PLS without a GPU: the numpy definition (tests/multiblock_expect.py) against the two analyses it stacks,
the refusals before any engine exists, the seeded draws, the header constant, persistence."""
import os
import re
import warnings

import numpy as np
import pytest

from conftest import ROOT
from oracle import cpu_ref as ref
import multiblock_expect as mb

# (groups, n_cond, T, mean_centering, B): the designs of tests/test_gpu_multiblock.py -- T' = 16, 9, 15, 24, 44
DESIGNS = [([7, 9], 2, 3, 0, 40), ([12], 3, 2, 0, 40), ([6, 5, 8], 1, 4, 1, 40), ([10, 11], 2, 5, 2, 40),
           ([30, 30], 2, 10, 0, 60)]


def _data(groups, n_cond, T, B, seed):
    rs = np.random.RandomState(seed)
    S = sum(groups) * n_cond
    cells = ref.dummy_label(groups, n_cond) - 1
    X = rs.randn(S, B) + 0.3 * cells[:, None] * rs.randn(1, B)
    Y = rs.randn(S, T) + 0.5 * X[:, :1]
    return X, Y


@pytest.mark.parametrize('groups,n_cond,T,mc,B', DESIGNS)
def test_unit_rows_make_the_squared_singular_values_sum_to_tprime(groups, n_cond, T, mc, B):
    X, Y = _data(groups, n_cond, T, B, seed=T)
    specs = mb.specs_of(groups, n_cond, False, mc)
    J = len(groups) * n_cond
    R = mb.R_mb(specs, X, Y)
    assert R.shape == (J + J * T, B)
    assert np.abs(np.sqrt((R ** 2).sum(axis=1)) - 1).max() <= 1e-14
    _, sv, _ = mb.original(specs, X, Y)
    assert abs((sv ** 2).sum() - (J + J * T)) <= 1e-12 * (J + J * T)
    res = mb.run_multiblock(X, Y, groups=groups, n_cond=n_cond, mean_centering=mc)
    assert abs(res['varexp'].sum() - 1) <= 1e-13 and res['y_loadings'].shape == (J + J * T, min(J + J * T, B))


@pytest.mark.parametrize('groups,n_cond,T,mc,B', DESIGNS)
def test_each_block_is_the_row_normalised_matrix_of_its_own_analysis(groups, n_cond, T, mc, B):
    X, Y = _data(groups, n_cond, T, B, seed=10 + T)
    sm, sb = specs = mb.specs_of(groups, n_cond, False, mc)
    J = len(groups) * n_cond
    rs = np.random.RandomState(3)
    perm = rs.permutation(len(X))
    boot = np.concatenate([rs.choice(np.flatnonzero(c), size=int(c.sum())) for c in sb.dummy.T.astype(bool)])
    for kw, (Xt, Xb, Yb) in (({}, (X, X, Y)), (dict(perminds=perm), (X[perm], X, Y[perm])),
                             (dict(bootinds=boot), (X[boot], X[boot], Y[boot]))):
        R = mb.R_mb(specs, X, Y, **kw)
        task = ref.gen_covcorr(sm, Xt, sm.dummy, sm.dummy)
        behav = ref.gen_covcorr(sb, Xb, Yb, sb.dummy)
        # the behaviour rows removed by hand: rownorm of the mean-centred R -- and the reverse
        assert np.array_equal(R[:J], task / np.sqrt((task ** 2).sum(axis=1, keepdims=True)))
        assert np.array_equal(R[J:], behav / np.sqrt((behav ** 2).sum(axis=1, keepdims=True)))
    # the permutation moves rows of X between cells in the task block only: the behaviour block sees the fixed X
    assert np.array_equal(mb.R_mb(specs, X, Y, perminds=perm)[J:], mb.rownorm(ref.gen_covcorr(sb, X, Y[perm], sb.dummy)))
    # a zero row stays zero (a constant feature matrix: every cell mean equals the reference mean)
    Z = mb.R_mb(specs, np.ones_like(X), Y)
    assert np.all(Z[:J] == 0) and np.all(np.isfinite(Z[:J]))


def test_host_cell_means_are_the_mean_centred_gen_covcorr():
    from pypyls_amd import hostmath
    for groups, n_cond, T, mc, B in DESIGNS:
        X, _ = _data(groups, n_cond, T, 7, seed=20 + T)
        sm = mb.specs_of(groups, n_cond, False, mc)[0]
        want = ref.gen_covcorr(sm, X, sm.dummy, sm.dummy)
        got = hostmath.cell_means_centered(X, ref.dummy_label(groups, n_cond) - 1, len(groups), n_cond, mc)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(X).max()


def _no_engine(monkeypatch):
    from pypyls_amd import engine

    def boom(*a, **k):
        raise AssertionError('an engine was created or looked up before the arguments were checked')
    monkeypatch.setattr(engine, 'default_engine', boom)
    monkeypatch.setattr(engine.Engine, '__init__', boom)


def test_every_refusal_comes_before_any_engine(monkeypatch):
    import pypyls_amd as pls
    _no_engine(monkeypatch)
    rs = np.random.RandomState(0)
    X, Y = rs.randn(24, 30), rs.randn(24, 2)
    kw = dict(groups=[6, 6], n_cond=2, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match='n_split'):
        pls.multiblock_pls(X, Y, n_split=5, **kw)
    with pytest.raises(ValueError, match='[Cc]ross-validation'):
        pls.multiblock_pls(X, Y, test_split=10, **kw)
    with pytest.raises(ValueError, match='contrasts'):
        pls.multiblock_pls(X, Y, contrasts=rs.randn(12, 2), **kw)
    with pytest.raises(ValueError, match='permindices'):
        pls.multiblock_pls(X, Y, permindices=False, permsamples=rs.randn(3, 24, 2), **dict(kw, n_perm=3))
    with pytest.raises(ValueError, match='subset of the conditions'):
        pls.multiblock_pls(X, Y, bscan=[0], **kw)
    with pytest.raises(ValueError, match='one group and one condition'):
        pls.multiblock_pls(X, Y, groups=[24], n_cond=1, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match='limit'):                        # T' = 4 + 4 x 400 > 1280
        pls.multiblock_pls(X, rs.randn(24, 400), **kw)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match='`X` contains'):
            pls.multiblock_pls(np.where(np.arange(720).reshape(24, 30) == 7, bad, X), Y, **kw)
        with pytest.raises(ValueError, match='`Y` contains'):
            pls.multiblock_pls(X, np.where(np.arange(48).reshape(24, 2) == 7, bad, Y), **kw)
    with pytest.raises(ValueError, match='samples'):
        pls.multiblock_pls(X, Y, groups=[6, 5], n_cond=2, n_perm=0, n_boot=0, verbose=False)
    with pytest.raises(ValueError, match='same number'):
        pls.multiblock_pls(X, Y[:-1], **kw)
    # the resets of meancentered_pls apply unchanged
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        with pytest.raises(AssertionError, match='engine'):
            pls.multiblock_pls(X, Y, groups=[8, 8, 8], n_cond=1, mean_centering=0, n_perm=0, n_boot=0, verbose=False)
    assert len([w for w in rec if 'Resetting mean_centering to 1' in str(w.message)]) == 1
    # a valid call gets past the checks and only then asks for an engine
    with pytest.raises(AssertionError, match='engine'):
        pls.multiblock_pls(X, Y, bscan=[0, 1], **kw)


def _draws(method, X, Y, L, **kw):
    from pypyls_amd.plsc import _PLSCRun
    run = _PLSCRun(method, X, Y, groups=[6, 6], n_cond=2, n_perm=7, n_boot=5, seed=1234, **kw)
    draws = run._plan_draws(L).start()
    draws.join()
    draws.thread.join()
    return run, run.perm_stream.samples, run.boot_stream.samples


def test_a_seeded_call_draws_the_arrays_of_the_behavioral_call():
    from pypyls_amd import resampling
    rs = np.random.RandomState(1)
    # B = 6 <= J T: both methods have L = B, so the normal((L, L + 10)) block in front of the index arrays is the same
    X, Y = rs.randn(24, 6), rs.randn(24, 2)
    run, perm_m, boot_m = _draws('multiblock', X, Y, 6, mean_centering=0)
    _, perm_b, boot_b = _draws('behavioral', X, Y, 6)
    assert run.inputs['method'] == 'multiblock' and run.inputs['permindices'] is True
    assert np.array_equal(perm_m, perm_b) and np.array_equal(boot_m, boot_b)
    # ... and with L = T' = 12 (B = 30) the order is the existing one: the block, the permutations, the bootstraps
    X = rs.randn(24, 30)
    _, perm_m, boot_m = _draws('multiblock', X, Y, 12)
    want = np.random.RandomState(1234)
    want.normal(size=(12, 22))
    assert np.array_equal(perm_m, resampling.gen_permsamp([6, 6], 2, seed=want, n_perm=7))
    assert np.array_equal(boot_m, resampling.gen_bootsamp([6, 6], 2, seed=want, n_boot=5))


def test_header_declares_the_method_and_the_library_knows_its_kernel_class():
    hdr = open(os.path.join(ROOT, 'include', 'plsx.h')).read()
    assert re.search(r'\bPLSX_MULTIBLOCK\s*=\s*3\b', hdr)
    core = open(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_core.hip')).read()
    assert 'PLSX_MULTIBLOCK' in core
    from pypyls_amd import plsc
    assert plsc._METHOD_CODE['multiblock'] == 3
    import pypyls_amd as pls
    assert callable(pls.multiblock_pls)
    from pypyls_amd import _build
    if os.path.exists(_build.lib_path()):
        import ctypes
        lib = ctypes.CDLL(_build.lib_path())
        lib.plsx_kernel_class_name.restype = ctypes.c_char_p
        names, i = [], 0
        while lib.plsx_kernel_class_name(i):
            names.append(lib.plsx_kernel_class_name(i).decode())
            i += 1
        assert 'k_mb_rownorm' in names, names


def test_save_load_round_trip(tmp_path):
    import pypyls_amd as pls
    from pypyls_amd import io
    from pypyls_amd.structures import PLSResults
    try:
        io._h5py()
    except ImportError as exc:
        pytest.skip('no HDF5 backend: {}'.format(exc))
    groups, n_cond, T, mc, B = DESIGNS[0]
    X, Y = _data(groups, n_cond, T, B, seed=5)
    rs = np.random.RandomState(6)
    perms = np.stack([rs.permutation(len(X)) for _ in range(4)], axis=1)
    want = mb.run_multiblock(X, Y, groups=groups, n_cond=n_cond, mean_centering=mc, permsamples=perms)
    res = PLSResults(x_weights=want['x_weights'], y_weights=want['y_weights'], singvals=want['singvals'],
                     varexp=want['varexp'], y_loadings=want['y_loadings'], y_scores=want['y_scores'],
                     permres=dict(pvals=want['permres']['pvals'], perm_singval=want['permres']['perm_singval']),
                     inputs=dict(X=X, Y=Y, groups=groups, n_cond=n_cond, mean_centering=mc, method='multiblock'))
    back = pls.load_results(pls.save_results(str(tmp_path / 'multiblock'), res))
    assert back.inputs.method == 'multiblock' and int(back.inputs.mean_centering) == mc
    assert np.array_equal(back.singvals, want['singvals'])
    assert np.array_equal(back.y_loadings, want['y_loadings']) and back.y_weights.shape == (16, 16)
    assert np.array_equal(back.permres.perm_singval, want['permres']['perm_singval'])
