"""Staging of the dense cross-product blocks (k_xprod): several k-steps per LDS stage, chosen at launch by what
divides the padded k-step count.  The library pads the contraction to a multiple of EIGHT rows (Kpad = round_up(S, 8),
nks = Kpad / 4), so the k-step count is always even: stages hold three k-steps when nks is a multiple of 6 and two
otherwise.  An odd count (7, 9, 1 k-steps -- one k-step per stage, "3 only", a single k-step) cannot be reached through
the library; the launchers keep one k-step per stage only as a guard.  The shapes are the ones where staging can go
wrong, not the workload's: both stage heights with one, two, an even and an odd number of stages, a column count below
one block and counts the block width does not divide, full and partial groups of the 25-tile fixed-X block (T' = 50:
eight permutations fill it).  GPU only."""
import functools

import numpy as np
import pytest

from conftest import assert_close
from oracle import cpu_ref as ref

pytestmark = pytest.mark.gpu

T = 50
# S -> nks = round_up(S, 8) / 4 -> k-steps per stage x stages:
#   24 -> 6 -> 3 x 2      28, 32 -> 8 -> 2 x 4      36 -> 10 -> 2 x 5 (odd stage count)      8, 4 -> 2 -> 2 x 1 (fewer
#   stages than buffers)      16 -> 4 -> 2 x 2      48 -> 12 -> 3 x 4
S_CASES = [24, 28, 32, 36, 8, 4, 16, 48]
# Bpad = round_up(B + L, 128): B = 64 is two 64-column blocks of the 4-wave fixed-X kernel (the second one all padding
# and scores) and one 128-column block of the 8-wave moment kernel; 200 and 1000 are not multiples of either width
B_CASES = [64, 200, 1000]
N_PERM = (8, 9, 17)           # one full group of eight, a group with one resample, a partial sweep of groups
N_BOOT = 9
N_BOOT_WIDE = 130             # > 128 (resample, cell) pairs: the 24-tile moment blocks instead of the 16-tile ones


def _engine():
    from pypyls_amd.engine import Engine, options_from_env
    return Engine(**options_from_env())


@functools.lru_cache(maxsize=None)
def _problem(S, B):
    """Data, decomposition and index arrays of a shape: computed once, shared, never written to."""
    from pypyls_amd import resampling as rsmp
    rs = np.random.RandomState(100 + S)
    X = rs.randn(S, B) + 3.0 * rs.rand(1, B)
    Y = rs.randn(S, T) + 1.5
    Y[:, :T] += 0.5 * X[:, :T]
    spec = ref.Spec('behavioral', [S], 1, False, 0)
    U, d, V = ref.decompose(spec, X, Y)
    perms = rsmp.gen_permsamp([S], 1, max(N_PERM), seed=3)
    for a in (X, Y, U, d, V):
        a.setflags(write=False)
    return X, Y, U, d, V, np.ascontiguousarray(perms)


@functools.lru_cache(maxsize=None)
def _perm_reference(S, B):
    X, Y, U, d, V, perms = _problem(S, B)
    spec = ref.Spec('behavioral', [S], 1, False, 0)
    spec.rotate = True
    want = np.stack([ref.single_perm(spec, X, Y, perms[:, i], V)[0] for i in range(perms.shape[1])], -1)
    want.setflags(write=False)
    return want


def _ready_engine(S, B):
    from pypyls_amd import resampling as rsmp
    X, Y, U, d, V, _ = _problem(S, B)
    eng = _engine()
    eng.set_data(X, Y, rsmp.cell_of_row([S], 1), 1, 1, 0, mean_centering=0, covariance=False)
    eng.set_original(U, np.diag(d), V)
    return eng


@pytest.mark.parametrize('B', B_CASES)
@pytest.mark.parametrize('S', S_CASES)
def test_fixed_x_permutations_every_stage_count(S, B):
    """Permutations through the feature pass (the 25-tile fixed-X blocks) against the oracle's single_perm and
    against the S x S dual route; tolerances of test_gpu_kernels.py::test_dual_perm_path_equals_feature_pass."""
    X, Y, U, d, V, perms = _problem(S, B)
    want = _perm_reference(S, B)
    live = ref.live_lvs(np.diag(d))
    eng = _ready_engine(S, B)
    for n in N_PERM:
        idx = eng._index_rows(perms[:, :n])
        got = {}
        for dual in (True, False):
            eng.set_perm_path(dual)
            out = eng._empty((n, eng.L))
            eng.perm_into(idx, out, rotate=True)
            eng.sync()
            assert bool(eng.last_timing()['dual_perm']) == dual
            got[dual] = out.cpu().numpy().T.copy()
        assert_close(got[True][live], got[False][live], 1e-9, what='dual vs feature pass, n = %d' % n)
        assert_close(got[False][live], want[live][:, :n], 1e-7, what='feature pass vs oracle, n = %d' % n)
        assert_close(got[True][live], want[live][:, :n], 1e-7, what='dual vs oracle, n = %d' % n)


def _boot_case(S, B, n_boot):
    from pypyls_amd import resampling as rsmp
    X, Y, U, d, V, _ = _problem(S, B)
    spec = ref.Spec('behavioral', [S], 1, False, 0)
    boots = np.ascontiguousarray(rsmp.gen_bootsamp([S], 1, n_boot, seed=2))
    live = ref.live_lvs(np.diag(d))
    eng = _ready_engine(S, B)
    idx = eng._index_rows(boots)
    usum, usq = eng._zeros((eng.B, eng.L)), eng._zeros((eng.B, eng.L))
    dist = eng._empty((n_boot, eng.Tp, eng.L))
    eng.boot_begin(n_boot)
    eng.boot_into(idx, usum, usq, dist)
    eng.boot_finish(usum, usq)
    eng.sync()
    ws, wq, wd = np.zeros_like(U), np.zeros_like(U), []
    for i in range(n_boot):
        dd, ub = ref.single_boot(spec, X, Y, boots[:, i], U, d)
        ws += ub
        wq += ub ** 2
        wd.append(dd)
    # (S <= 48 < T' = 50: the decomposition has S - 1 live latent variables; the rest are compared nowhere in the suite)
    assert_close(usum.cpu().numpy()[:, live], ws[:, live], 1e-7, what='u_sum')
    assert_close(usq.cpu().numpy()[:, live], wq[:, live], 1e-7, what='u_square')
    assert_close(dist.cpu().numpy().transpose(1, 2, 0)[:, live], np.stack(wd, -1)[:, live], 1e-7, what='distrib')


@pytest.mark.parametrize('B', B_CASES)
@pytest.mark.parametrize('S', S_CASES)
def test_moment_blocks_every_stage_count(S, B):
    """A handful of bootstraps (their feature moments come from the moment-only blocks) against the oracle's
    single_boot; tolerances of test_gpu_kernels.py for distrib and the two sums."""
    _boot_case(S, B, N_BOOT)


@pytest.mark.parametrize('S', [24, 28, 32, 36])
def test_moment_blocks_24_tiles(S):
    """Enough (resample, cell) pairs for the 192-pair moment blocks: stages of three (S = 24) and of two k-steps."""
    _boot_case(S, 200, N_BOOT_WIDE)
