"""
Behavioural cross-validation on the device (plsx_crossval_batch: k_cv_src, k_cv_rescale, k_cv_final, the Gram mode
Q = Rs Xc^T, the small solver returning V and d, the batching of crossval_impl, the re-plan of covariance mode) against
the numpy definition of tests/crossval_expect.py, through Engine.set_data / Engine.crossval only.  GPU only.

Tolerance: crossval_expect.TOL per ENTRY of r and of r2 (see there); tests/test_crossval_expect_host.py asserts, without
a GPU, the conditioning of every split of every case that this tolerance rests on.  Every route edge a case claims is
asserted from what the context reports (last_timing, the launches a timed call records), not assumed.
"""
import numpy as np
import pytest

from oracle import cpu_ref as ref
import crossval_expect as cx

pytestmark = pytest.mark.gpu

SMALL = dict(scratch_gb=0.00025, min_batch=8)           # a fixed budget of one group per launch at these shapes
_ENGINES = {}


def _engine(**options):
    """A fresh context without options (what it reports then describes this binding alone); one per option set
    otherwise, kept for the module."""
    from pypyls_amd.engine import Engine
    if not options:
        return Engine()
    key = tuple(sorted(options.items()))
    if key not in _ENGINES:
        scratch = options.pop('scratch_gb', None)
        _ENGINES[key] = Engine(scratch_gb=scratch, options=options)
    return _ENGINES[key]


def _bind(eng, name):
    from pypyls_amd import resampling as rsmp
    case = cx.CASES[name]
    spec, X, Y, masks = cx.problem(name)
    eng.set_data(X, Y, rsmp.cell_of_row(case['groups'], case['n_cond']), len(case['groups']), case['n_cond'], 0,
                 covariance=case['cov'])
    return spec, X, Y, masks


def _plan(eng, m, J):
    """npg, the M-tiles of a block and nb = splits per pass by the rule of crossval_impl (csrc/plsx_split.hip), from
    what the context reports after set_data; launch_groups is taken at its cap, min(Gcap, groups needed), which the
    number of cross-product launches of a timed call then confirms (_passes)."""
    t = eng.last_timing()
    npg, mt = int(t['resamples_per_group']), int(t['m_tiles'])
    gcap = int(t['superbatch']) // npg
    nb = max(1, min(min(gcap, -(-m // npg)) * npg, 256 // max(J, 1)))
    nb = max(nb // npg * npg, npg)
    return npg, mt, nb


def _passes(eng, masks):
    """Cross-product launches of one crossval call = its passes."""
    eng.set_timing(True)
    try:
        out = eng.crossval(masks)
        launches = eng.kernel_timing().get('k_xprod', (0.0, 0))[1]
    finally:
        eng.set_timing(False)
    return launches, out


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('name', list(cx.CASES))
def test_case_against_the_expectation(name):
    case = cx.CASES[name]
    eng = _engine()
    spec, X, Y, masks = _bind(eng, name)
    J, T, m = spec.dummy.shape[1], case['T'], masks.shape[1]
    assert (eng.Tp, eng.L) == (J * T, min(J * T, case['B']))
    npg, mt, nb = _plan(eng, m, J)
    want_r, want_r2, _ = cx.expected(name)
    launches, (r, r2) = _passes(eng, masks)
    print('{}: T\' {} J {} npg {} m_tiles {} nb {} m {} passes {}'.format(name, eng.Tp, J, npg, mt, nb, m, launches))
    if not case['cov']:                                  # (covariance plans its moment rows in for the call only)
        assert launches == -(-m // nb)
    assert r.shape == r2.shape == (T, m)
    cx.assert_entrywise(r, r2, want_r, want_r2, what=name)
    # run-to-run reproducibility: the same call, the same bits
    assert _same_bits(eng.crossval(masks), (r, r2))
    # the edge the case is there for
    if name in ('E1', 'E2', 'E3'):
        assert m > nb and (m - nb) % npg != 0 and launches == 2
    if name == 'E3':
        assert J == 16 and J * npg <= 48 < J * (npg + 1)  # 16 cells: the three moment tiles bound the group
    if name.startswith('E5'):
        assert eng.Tp == T and case['B'] % 128 == 1      # T' = 63, 64 | 65: PLSX_JACOBI_TP = 64 (plsx_common.h)
    if name == 'E8':
        assert eng.Tp > case['B'] == eng.L
    if name == 'E9':
        assert mt == 16 and npg == 1 and 177 <= eng.Tp <= 224
    if name in ('E10', 'E11_corr', 'E11_cov'):
        # The sliced layout is not observable through the ABI.  Derivation: one resample needs ceil(T' / 16) data
        # tiles and two moment tiles per 16 cells in a block of 24 (plan_groups), so T' > 352 never fits and the rows
        # are cut greedily at whole tiles (crossval_expect.slices_of restates the rule; the host test pins it): slice 0
        # ends at row 352, inside the last cell, whose moment row k_cv_rescale takes from slice 0 (cell_momrow).
        assert eng.Tp > 352 and npg == 1
        sl = cx.slices_of(eng.Tp, T, J)
        assert len(sl) == 2 and sl[0][1] == 352 and sl[1][2] == J - 1 and (J - 1) * T < 352 < J * T
    if case['deficient']:
        info = cx.expected(name)[2]
        assert all(i['n_live'] < i['L'] for i in info)


@pytest.mark.parametrize('name', ['E1', 'E2', 'E3'])
def test_passes_are_independent(name):
    """A split's numbers do not depend on the pass it runs in, its place in the pass or the size of the batch."""
    eng = _engine()
    spec, X, Y, masks = _bind(eng, name)
    J, m = spec.dummy.shape[1], masks.shape[1]
    npg, _, nb = _plan(eng, m, J)
    assert m > nb
    full = eng.crossval(masks)
    bits = []
    for i in (nb - 1, nb, m - 1):                        # last of pass 1, first of pass 2, last of all
        one = eng.crossval(masks[:, [i]])
        cx.assert_entrywise(one[0], one[1], full[0][:, [i]], full[1][:, [i]], what='{} split {} alone'.format(name, i))
        bits.append(_same_bits(one, (full[0][:, [i]], full[1][:, [i]])))
    small = _engine(**SMALL)
    _bind(small, name)
    npg_s, _, nb_s = _plan(small, m, J)
    launches, other = _passes(small, masks)
    assert npg_s == npg and nb_s < nb and launches == -(-m // nb_s) > 2
    cx.assert_entrywise(other[0], other[1], full[0], full[1], what='{} in passes of {}'.format(name, nb_s))
    want_r, want_r2, _ = cx.expected(name)
    cx.assert_entrywise(other[0], other[1], want_r, want_r2, what='{} in passes of {} vs expectation'.format(name, nb_s))
    print('{}: single-split bits equal {}; passes of {} vs {}: bits equal {}'.format(
        name, bits, nb_s, nb, _same_bits(other, full)))


@pytest.mark.parametrize('name', ['E4', 'E11_cov', 'E2'])
def test_crossval_leaves_the_context_as_it_found_it(name):
    """Covariance mode plans the per-cell moment rows in for the call and out again (replan_moments): permutations,
    bootstraps, split-half and the cross-covariance give the same bits after a crossval as before it.  E2 (correlation
    mode, no re-plan) is the control."""
    from pypyls_amd import resampling as rsmp
    case = cx.CASES[name]
    eng = _engine()
    spec, X, Y, masks = _bind(eng, name)
    U, d, V = ref.decompose(spec, X, Y)
    eng.set_original(U, np.diag(d), V)
    perms = rsmp.gen_permsamp(case['groups'], case['n_cond'], 3, seed=1)
    boots = rsmp.gen_bootsamp(case['groups'], case['n_cond'], 3, seed=2)
    halves = rsmp.gen_splits(case['groups'], case['n_cond'], 2, seed=3)

    def four():
        usum, usq, dist = eng.boot(boots)
        uc, vc = eng.split_half(halves)
        return [eng.perm(perms), usum.cpu().numpy(), usq.cpu().numpy(), dist, uc, vc, eng.crosscov(ysrc=perms)], \
            eng.last_timing()['resamples_per_group']

    before, npg_before = four()
    r, r2 = eng.crossval(masks)
    want_r, want_r2, _ = cx.expected(name)
    cx.assert_entrywise(r, r2, want_r, want_r2, what=name + ' between the other legs')
    after, npg_after = four()
    for what, a, b in zip(('perm', 'u_sum', 'u_square', 'distrib', 'ucorr', 'vcorr', 'crosscov'), before, after):
        assert np.all(np.isfinite(a)), what
        assert np.array_equal(a, b), what
    assert npg_after == npg_before
    # and the legs still answer correctly (the layout that came back is a working one)
    got = before[0]
    want = np.stack([ref.single_perm(spec, X, Y, perms[:, i], V)[0] for i in range(perms.shape[1])], -1)
    assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max()


@pytest.mark.parametrize('name', ['E6_65', 'E6_127'])
def test_memory_that_held_nan_does_not_reach_the_result(name):
    """Regression.  The rescaled copies Rs (one per split and cell, T'pp x Bpad) are mapped without being cleared and
    k_cv_rescale wrote their B columns only; with S > 64 the product Q = Rs Xc^T runs on the 64 x 64-block Gram
    kernel, which reads the 16-column step that holds column B - 1 in full and masks it on the Xc side alone.  When
    the block had belonged to someone who left a NaN at such a column (B % 16 != 0), every score of the split was NaN:
    seen once on E6_65 inside the whole suite, never alone.  Here blocks of exactly that size are filled with NaN and
    freed right before the call, so that the copies land on them."""
    import ctypes
    import os
    import torch
    path = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
    hip = ctypes.CDLL(path if os.path.exists(path) else 'libamdhip64.so')      # the runtime the process already holds
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    case = cx.CASES[name]
    eng = _engine()
    spec, X, Y, masks = _bind(eng, name)
    assert case['S'] > 64 and case['B'] % 16 != 0
    J, m = spec.dummy.shape[1], masks.shape[1]
    tpp, bpad = -(-eng.Tp // 4) * 4, -(-(eng.B + eng.L) // 128) * 128
    nbytes = m * J * tpp * bpad * 8                      # Rs of the call (crossval_impl)
    host = np.full(nbytes // 8, np.nan)
    blocks = []
    for _ in range(256):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), nbytes) == 0
        assert hip.hipMemcpy(p, host.ctypes.data, nbytes, 1) == 0           # 1 = host to device
        blocks.append(p)
    assert hip.hipDeviceSynchronize() == 0
    for p in blocks:
        assert hip.hipFree(p) == 0
    r, r2 = eng.crossval(masks)
    want_r, want_r2, _ = cx.expected(name)
    cx.assert_entrywise(r, r2, want_r, want_r2, what=name + ' on memory that held NaN')


def test_mean_centred_binding_still_refuses():
    from pypyls_amd.engine import PlsxError
    from pypyls_amd import resampling as rsmp
    rs = np.random.RandomState(0)
    eng = _engine()
    eng.set_data(rs.randn(24, 30), None, rsmp.cell_of_row([6, 6], 2), 2, 2, 1)
    with pytest.raises(PlsxError, match='behavioral PLS'):
        eng.crossval(rs.rand(24, 2) < 0.7)
