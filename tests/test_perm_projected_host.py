"""The identity behind the projected permutation route (plsx_core.hip perm_projected), on the host.

A rotated permutation reports ssd_l = || column l of V_p d_p Q ||, Q = P^T N^T the Procrustes rotation of
V0^T V_p = N S P (oracle.cpu_ref.procrustes).  With V0 square and orthogonal and V_p a complete orthonormal basis,
V0^T V_p is orthogonal, Q is its transpose exactly and

    ssd_l^2 = (V0^T V_p d_p^2 V_p^T V0)_ll = (V0^T G_p V0)_ll = || row l of V0^T R_p ||^2,    G_p = R_p R_p^T,

for any rank of G_p.  numpy only; the oracle is the reference.
"""
import numpy as np
import pytest

from oracle import cpu_ref as ref


def _case(S, B, T, groups, n_cond, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B)
    Y = rs.randn(S, T) + 0.3 * X[:, :T]
    spec = ref.Spec('behavioral', groups, n_cond)
    spec.rotate = True
    U, d, V = ref.decompose(spec, X, Y)
    return rs, spec, X, Y, V


def _projected(spec, X, Y, perm, V0):
    """sqrt(diag(V0^T G V0)) and the row norms of V0^T R of one permutation."""
    Xp, Yp = ref.make_permutation(spec, X, Y, perm)
    R = ref.gen_covcorr(spec, Xp, Yp, spec.dummy)
    G = R @ R.T
    quad = np.sqrt(np.maximum(np.einsum('tl,ts,sl->l', V0, G, V0), 0.0))
    rows = np.linalg.norm(V0.T @ R, axis=1)
    return quad, rows


# full rank: T' <= S - 1 in every cell
FULL = [(40, 300, 5, [40], 1, 1), (60, 500, 6, [30, 30], 1, 2), (48, 257, 3, [12, 12], 2, 3)]
# rank-deficient permuted G: T' = J T > S - J (the z-scored rows of a cell span n_j - 1 dimensions)
DEFICIENT = [(12, 300, 14, [12], 1, 4), (16, 200, 9, [8, 8], 1, 5), (9, 120, 9, [9], 1, 6)]


@pytest.mark.parametrize('S,B,T,groups,n_cond,seed', FULL + DEFICIENT)
def test_row_norms_equal_the_rotated_statistic(S, B, T, groups, n_cond, seed):
    """sqrt(diag(V0^T G V0)) against oracle.cpu_ref.single_perm, 1e-12 of the largest value.

    The diagonal is evaluated as the device evaluates it, as the squared row norms of V0^T R (G = R R^T is never
    formed), on every case.  With G formed first the same bound is asserted on the full-rank cases.  On the
    rank-deficient ones the ORIGINAL is rank deficient too (same shape), the statistic of its null LVs is zero, and
    a zero taken as the square root of a quantity that cancels in G only to eps ||G|| comes out as sqrt(eps) ||R||:
    measured up to 9.3e-9 of the largest value on the cases below (the test prints every figure), against 1e-15 for
    the row norms.  No fp64 evaluation through G reaches 1e-12 there, so for those cases the G-formed value is held to 1e-12
    of the largest SQUARED value, where the identity lives, and its distance after the root is printed.  (The device
    route does not take such data: a dead original LV keeps the Gram route, perm_projected in plsx_core.hip.)"""
    rs, spec, X, Y, V0 = _case(S, B, T, groups, n_cond, seed)
    Tp = V0.shape[0]
    assert V0.shape == (Tp, Tp), 'the case must have L == T\''
    assert np.allclose(V0.T @ V0, np.eye(Tp), atol=1e-12)
    deficient = (S, B, T, groups, n_cond, seed) in DEFICIENT
    if deficient:
        assert Tp > S - len(groups) * n_cond, 'the case is meant to be rank deficient'
    for i in range(4):
        perm = rs.permutation(S)
        want = ref.single_perm(spec, X, Y, perm, V0)[0]
        quad, rows = _projected(spec, X, Y, perm, V0)
        tol = 1e-12 * want.max()
        err_rows, err_quad = np.max(np.abs(rows - want)), np.max(np.abs(quad - want))
        print('perm {}: row norms {:.2e}, through G {:.2e} of the largest value'.format(
            i, err_rows / want.max(), err_quad / want.max()))
        assert err_rows <= tol, ('row norms of V0^T R', i, err_rows / want.max())
        if deficient:
            assert np.max(np.abs(quad ** 2 - want ** 2)) <= 1e-12 * want.max() ** 2, ('diag(V0^T G V0)', i)
        else:
            assert err_quad <= tol, ('sqrt(diag(V0^T G V0))', i, err_quad / want.max())


def test_identity_fails_without_a_square_v0():
    """B < T': L = B, V0 and V_p are T' x L, V0^T V_p is no longer orthogonal, the Procrustes rotation is not its
    transpose and the row norms are NOT the rotated statistic -- why the route asks for L == T'."""
    rs = np.random.RandomState(7)
    S, B, T = 40, 4, 6
    X, Y = rs.randn(S, B), rs.randn(S, T)
    spec = ref.Spec('behavioral', [S], 1)
    V0 = ref.decompose(spec, X, Y)[2]
    assert V0.shape == (T, B)
    worst = 0.0
    for i in range(4):
        perm = rs.permutation(S)
        want = ref.single_perm(spec, X, Y, perm, V0)[0]
        quad, rows = _projected(spec, X, Y, perm, V0)
        worst = max(worst, np.max(np.abs(rows - want)) / want.max())
    assert worst > 1e-3, worst


def test_no_perm_project_is_an_option_key():
    """The route switch goes through plsx_set_option and engine.options_from_env (no GPU: the keys come from the library)."""
    from pypyls_amd import engine
    assert 'no_perm_project' in engine.option_names()
    assert engine.options_from_env({'PLSX_NO_PERM_PROJECT': '1'}) == {'options': {'no_perm_project': 1}}
