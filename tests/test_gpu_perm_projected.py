"""Projected permutations on the device (plsx_core.hip perm_projected, k_build_A_proj, k_xprod epilogue 10,
k_rownorm_finish): rotated permutations of a fixed-X binding with L == T' and every original LV live take their
singular values from the row norms of (V0^T A_p) Xn -- no cross-product scratch, no Gram pass, no small solver.

Reference: oracle.cpu_ref.single_perm per entry, at the 1e-9 the fixed-X permutation tests hold singular values to
(test_gpu_timed_geometry.py, test_gpu_edges.py).  Shapes are the smallest that reach each edge of the route:

* k-steps per LDS stage (stage_ksteps in plsx_xprod.hip): the contraction is padded to a multiple of 8 rows, so the
  k-step count nks = round_up(S, 8) / 4 is even and the stage holds 3 k-steps when 24 divides round_up(S, 8) (S = 24,
  72 below) and 2 otherwise (S = 32, 56).  No S reaches the one-k-step instantiation through plsx_set_data today (it
  guards a change of that padding); it is compiled and launched by the same template and is not run here.
* T' = 50 with T = 50: eight permutations fill the 400 rows of a group, no padding row; T' = 7 and 12 leave padding rows
  inside the last tile (399 and 396 rows); T' = 1 and T' = 2.
* B at the edges of the 64-column block and of the 128-column padding of X.
* n = 1, 7, 8, 9, 65 at eight per group: a partly filled last group, and group counts (2, 9) that leave a partial sweep
  of the block map.
"""
import numpy as np
import pytest

from oracle import cpu_ref as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def _data(S, B, T, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T)
    k = min(B, T)
    Y[:, :k] += 0.4 * X[:, :k]
    return X, Y


def _bind(X, Y, groups, n_cond, options=None, scratch_gb=None, method=0, contrasts=None):
    """A bound engine on the feature-pass permutation route with the device's own decomposition as the original."""
    from pypyls_amd import hostmath, resampling as rsmp
    from pypyls_amd.engine import Engine
    eng = Engine(options=options, scratch_gb=scratch_gb)
    eng.set_data(X, Y, rsmp.cell_of_row(groups, n_cond), len(groups), n_cond, method)
    if contrasts is not None:
        eng.set_contrasts(contrasts)
    xw, sv, yw = eng.decompose()
    xw, yw = hostmath.sign_convention(xw, yw)
    eng.set_original(xw, sv, yw)
    eng.set_perm_path(False)
    return eng, xw, sv, yw


def _timed_perm(eng, perms, rotate=True):
    eng.set_timing(True)
    got = eng.perm(perms, rotate=rotate)
    tm, kt = eng.last_timing(), eng.kernel_timing()
    eng.set_timing(False)
    return got, tm, kt


def _assert_entries(got, want, what):
    rel = np.abs(got - want) / np.abs(want)
    assert np.all(rel <= RTOL), '{}: entry {} rel err {:.3e}'.format(what, np.unravel_index(np.argmax(rel), rel.shape),
                                                                    rel.max())
    return rel.max()


# (S, T, groups, n_cond, B, n)
SHAPES = [
    (72, 50, [72], 1, 129, 65),            # T' = 50 = T, three k-steps per stage, 9 groups: one sweep + a partial one
    (72, 50, [72], 1, 1003, 8),            # one full group
    (72, 50, [72], 1, 65, 1),
    (56, 50, [56], 1, 64, 9),              # two k-steps per stage, 2 groups (partial sweep), the last one with one slot
    (56, 50, [56], 1, 128, 7),
    (32, 7, [32], 1, 127, 7),              # T' = 7: 57 per group, 399 rows
    (32, 6, [16, 16], 1, 63, 65),          # two cells, T' = 12: 33 per group, 396 rows, 2 groups
    (24, 1, [24], 1, 1, 9),                # T' = 1 = B
    (24, 1, [24], 1, 17, 8),
    (24, 2, [24], 1, 17, 7),               # T' = 2
    (24, 1, [12, 12], 1, 63, 8),           # T' = 2 as two cells of one behaviour
    (24, 2, [24], 1, 64, 7),
    (24, 2, [24], 1, 65, 7),
    (24, 2, [24], 1, 127, 7),
    (24, 2, [24], 1, 128, 7),
    (24, 2, [24], 1, 129, 7),
    (24, 2, [24], 1, 1003, 7),
]


@pytest.mark.parametrize('S,T,groups,n_cond,B,n', SHAPES)
def test_shapes_against_oracle(S, T, groups, n_cond, B, n):
    from pypyls_amd import resampling as rsmp
    X, Y = _data(S, B, T, seed=S + T + B)
    eng, xw, sv, yw = _bind(X, Y, groups, n_cond)
    try:
        assert eng.L == eng.Tp, 'the shape is meant to have L == T\''
        perms = rsmp.gen_permsamp(groups, n_cond, n, seed=B, verbose=False)
        got, tm, kt = _timed_perm(eng, perms)
    finally:
        eng.close()
    assert tm['perm_projected'] == 1, tm
    assert 'k_gram' not in kt and 'k_build_A' in kt and kt['k_xprod'][1] >= 1, kt
    spec = ref.Spec('behavioral', groups, n_cond)
    want = np.stack([ref.single_perm(spec, X, Y, perms[:, i], yw)[0] for i in range(n)], -1)
    worst = _assert_entries(got, want, 'S {} T {} groups {} B {} n {}'.format(S, T, groups, B, n))
    print('projected permutations S {} T\' {} B {} n {}: worst entry rel err {:.2e}'.format(S, eng.Tp, B, n, worst))


@pytest.fixture(scope='module')
def case50():
    """T' = 50, B = 129, 19 permutations, their oracle, and the bits of the new route for the whole batch."""
    from pypyls_amd import resampling as rsmp
    S, T, B, n = 72, 50, 129, 19
    X, Y = _data(S, B, T, seed=50)
    perms = rsmp.gen_permsamp([S], 1, n, seed=51, verbose=False)
    eng, xw, sv, yw = _bind(X, Y, [S], 1)
    try:
        got, tm, kt = _timed_perm(eng, perms)
    finally:
        eng.close()
    spec = ref.Spec('behavioral', [S], 1)
    want = np.stack([ref.single_perm(spec, X, Y, perms[:, i], yw)[0] for i in range(n)], -1)
    _assert_entries(got, want, 'case50')
    return dict(X=X, Y=Y, perms=perms, got=got, want=want, yw=yw, tm=tm, kt=kt)


def test_ystack(case50):
    """plsx_perm_batch_y: a stack of pre-permuted Y takes the route and gives the bits of the index rows."""
    c = case50
    eng, _, _, yw = _bind(c['X'], c['Y'], [72], 1)
    try:
        stack = np.stack([c['Y'][c['perms'][:, i]] for i in range(c['perms'].shape[1])])
        eng.set_timing(True)
        got = eng.perm_ystack(stack, rotate=True)
        tm, kt = eng.last_timing(), eng.kernel_timing()
    finally:
        eng.close()
    assert tm['perm_projected'] == 1 and 'k_gram' not in kt, (tm, kt)
    _assert_entries(got, c['want'], 'ystack')
    assert np.array_equal(got, c['got'])


def test_same_bits_alone_elsewhere_small_scratch_and_twice(case50):
    c = case50
    perms = c['perms']
    eng, _, _, _ = _bind(c['X'], c['Y'], [72], 1)
    try:
        again = eng.perm(perms)
        twice = eng.perm(perms)
        alone = np.stack([eng.perm(perms[:, i:i + 1])[:, 0] for i in (0, 7, 8, 18)], -1)
        order = np.r_[np.arange(11, 19), np.arange(0, 11)]            # every permutation in another slot and group
        moved = eng.perm(perms[:, order])
    finally:
        eng.close()
    assert np.array_equal(again, c['got']) and np.array_equal(twice, c['got'])
    assert np.array_equal(alone, c['got'][:, [0, 7, 8, 18]])
    assert np.array_equal(moved, c['got'][:, order])
    # a scratch budget of one group per launch: three launches of 8, 8 and 3
    eng, _, _, _ = _bind(c['X'], c['Y'], [72], 1, scratch_gb=1e-6)
    try:
        got, tm, kt = _timed_perm(eng, perms)
    finally:
        eng.close()
    assert tm['perm_projected'] == 1 and kt['k_xprod'][1] == 3, (tm, kt)
    assert np.array_equal(got, c['got'])


def test_scratch_of_nans(case50):
    """Nothing on the route reads memory it did not write: blocks of the size of the R scratch the Gram route would map
    and of the partial buffer, filled with NaN and freed right before the call."""
    import torch
    c = case50
    n = c['perms'].shape[1]
    groups, Tpp, Bpad = -(-n // 8), 52, 256
    sizes = [groups * 8 * Tpp * Bpad, (Bpad // 64) * groups * 400, groups * 25 * 64 * 18 + 512]
    eng, _, _, _ = _bind(c['X'], c['Y'], [72], 1)
    try:
        for rep in range(2):
            blocks = [torch.full((s,), float('nan'), dtype=torch.float64, device=eng.device) for s in sizes for _ in range(3)]
            torch.cuda.synchronize()
            del blocks
            torch.cuda.empty_cache()
            got = eng.perm(c['perms'])
            assert np.all(np.isfinite(got))
            assert np.array_equal(got, c['got'])
    finally:
        eng.close()


def test_old_route_stays_where_the_condition_fails(case50):
    """no_perm_project, rotate = False, contrasts, a mean-centred binding, a dead original LV: the Gram pass and the
    small solver (the contrast norms for non-rotated PLS) run as before, and the results are those of the library with
    the route switched off."""
    from pypyls_amd import resampling as rsmp
    c = case50
    perms = c['perms']

    def run(options, rotate=True, X=c['X'], Y=c['Y'], groups=(72,), n_cond=1, method=0, contrasts=None, p=perms):
        eng, _, _, _ = _bind(X, Y, list(groups), n_cond, options=options, method=method, contrasts=contrasts)
        try:
            return _timed_perm(eng, p, rotate=rotate)
        finally:
            eng.close()

    off = {'no_perm_project': 1}
    # the switch
    got, tm, kt = run(off)
    assert tm['perm_projected'] == 0 and 'k_gram' in kt and 'k_small' in kt, (tm, kt)
    _assert_entries(got, c['want'], 'no_perm_project')
    rel = np.max(np.abs(got - c['got']) / np.abs(got))
    print('projected route against no_perm_project=1: largest relative difference {:.3e}'.format(rel))
    # rotate = False
    a, tm, kt = run(None, rotate=False)
    b = run(off, rotate=False)[0]
    assert tm['perm_projected'] == 0 and 'k_gram' in kt and 'k_small' in kt, (tm, kt)
    assert np.array_equal(a, b)
    # contrasts (non-rotated PLS)
    V = np.linalg.qr(np.random.RandomState(3).randn(50, 5))[0]
    a, tm, kt = run(None, contrasts=V)
    b = run(off, contrasts=V)[0]
    assert tm['perm_projected'] == 0 and 'k_contrast' in kt, (tm, kt)
    assert np.array_equal(a, b)
    # mean-centred binding
    Xm = c['X'][:48]
    pm = rsmp.gen_permsamp([12, 12], 2, 5, seed=9, verbose=False)
    a, tm, kt = run(None, X=Xm, Y=None, groups=(12, 12), n_cond=2, method=1, p=pm)
    b = run(off, X=Xm, Y=None, groups=(12, 12), n_cond=2, method=1, p=pm)[0]
    assert tm['perm_projected'] == 0 and 'k_gram' in kt and 'k_small' in kt, (tm, kt)
    assert np.array_equal(a, b)
    # a dead original LV: two identical behaviours
    Yd = c['Y'].copy()
    Yd[:, 1] = Yd[:, 0]
    a, tm, kt = run(None, Y=Yd)
    b = run(off, Y=Yd)[0]
    assert tm['perm_projected'] == 0 and 'k_gram' in kt and 'k_small' in kt, (tm, kt)
    assert np.array_equal(a, b, equal_nan=True)


def test_later_calls_do_not_see_the_route(case50):
    """Bootstraps, split-half and cross-validation after a projected permutation call: the bits they give after a
    permutation call on the Gram route."""
    from pypyls_amd import resampling as rsmp
    c = case50
    boots = rsmp.gen_bootsamp([72], 1, 9, seed=61, verbose=False)
    masks = rsmp.gen_splits([72], 1, 4, seed=62)
    cv = np.random.RandomState(63).rand(72, 3) < 0.75
    outs = []
    for options in (None, {'no_perm_project': 1}):
        eng, _, _, _ = _bind(c['X'], c['Y'], [72], 1, options=options)
        try:
            p = eng.perm(c['perms'])
            proj = eng.last_timing()['perm_projected']
            usum, usq, dist = eng.boot(boots)
            uc, vc = eng.split_half(masks)
            r, r2 = eng.crossval(cv)
            outs.append((proj, usum.cpu().numpy(), usq.cpu().numpy(), dist, uc, vc, r, r2))
        finally:
            eng.close()
    assert outs[0][0] == 1 and outs[1][0] == 0
    for a, b, name in zip(outs[0][1:], outs[1][1:], ('usum', 'usq', 'distrib', 'ucorr', 'vcorr', 'r', 'r2')):
        assert np.array_equal(a, b), name
