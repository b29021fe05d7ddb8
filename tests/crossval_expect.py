"""
Behavioural cross-validation in numpy, on the hooks of oracle.cpu_ref: the definition the device path
(plsx_crossval_batch) is tested against (tests/test_crossval_expect_host.py, tests/test_gpu_crossval.py).

For one training mask (True = training row), with the cells of the design in row order:

  R           = gen_covcorr of the training rows                         (T', B)
  U, d, V     = oracle svd(R);  live = d > RANK_RTOL * d.max()
  U_live      = R^T V_live / d_live                                      (B, n_live)
  test rows of cell j:
      pred    = zmap(X_test; mean, std(ddof=1) of the training rows of cell j) @ U_live @ V_live[jT:(j+1)T].T
                + mean of Y over the training rows of cell j
  r, r2       = efficient_corr / r2_score_raw of (Y_test, pred), test rows in row order

With every latent variable live this is oracle.cpu_ref.single_crossval (the reference, literally).  A rank-deficient
training decomposition (a cell with fewer than T + 1 training rows) is where the two part: the reference projects
through the null vectors its SVD happens to return, the device predicts from the live latent variables only
(PLSX_RANK_RTOL = oracle RANK_RTOL), and this module states the device's convention.

The module also holds the cases of the GPU test (shapes at the edges of the device path), their data and masks, and
the per-entry comparison both GPU front-end tests share.
"""
import functools

import numpy as np

from oracle import cpu_ref as ref

#: per entry: |r - want| <= TOL and |r2 - want| <= TOL * max(1, |want|).  What tests/test_gpu_kernels.py asks of the
#: analogous O(1) statistics (split-half ucorr / vcorr).  The device solves on the Gram matrix (error ~ eps * kappa^2)
#: and the prediction uses sum_live u_l v_l^T, which needs no gap BETWEEN live singular values: with kappa <= KAPPA_MAX
#: asserted on the expectation, eps * kappa^2 <= 2.3e-10 -- a 400 x margin for the sums over T' B terms.
TOL = 1e-7
KAPPA_MAX = 1e3


def single(spec, X, Y, mask):
    """One split -> r (T,), r2 (T,), info (n_live, L, kappa, gap)."""
    X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
    mask = np.asarray(mask, dtype=bool)
    T = Y.shape[1]
    dummy = spec.dummy.astype(bool)
    R = ref.gen_covcorr(spec, X[mask], Y[mask], dummy[mask])
    _, d, V = ref.svd(R)
    d = np.diag(d).copy()
    live = d > ref.RANK_RTOL * d.max()
    V_live, d_live = V[:, live], d[live]
    U_live = R.T @ V_live / d_live
    n_live = int(live.sum())
    info = dict(n_live=n_live, L=len(d), kappa=float(d_live.max() / d_live.min()),
                gap=float(d[n_live] / d[0]) if n_live < len(d) else 0.0)
    pred = np.full(Y.shape, np.nan)
    for j in range(dummy.shape[1]):
        tr, te = dummy[:, j] & mask, dummy[:, j] & ~mask
        if not te.any():
            continue
        mu, sd = X[tr].mean(axis=0), X[tr].std(axis=0, ddof=1)
        pred[te] = ((X[te] - mu) / sd) @ U_live @ V_live[j * T:(j + 1) * T].T + Y[tr].mean(axis=0, keepdims=True)
    return ref.efficient_corr(Y[~mask], pred[~mask]), ref.r2_score_raw(Y[~mask], pred[~mask]), info


def crossval(spec, X, Y, masks):
    """masks (S, m) -> pearson_r (T, m), r_squared (T, m), [info per split]."""
    out = [single(spec, X, Y, masks[:, i]) for i in range(masks.shape[1])]
    return np.stack([o[0] for o in out], -1), np.stack([o[1] for o in out], -1), [o[2] for o in out]


def errors(r, r2, want_r, want_r2):
    """Largest per-entry error of r (absolute) and of r2 (relative to max(1, |r2|))."""
    r, r2, want_r, want_r2 = (np.asarray(a, dtype=float) for a in (r, r2, want_r, want_r2))
    assert r.shape == want_r.shape and r2.shape == want_r2.shape, (r.shape, want_r.shape, r2.shape, want_r2.shape)
    assert np.all(np.isfinite(want_r)) and np.all(np.isfinite(want_r2))
    with np.errstate(invalid='ignore'):
        e_r = np.abs(r - want_r)
        e_r2 = np.abs(r2 - want_r2) / np.maximum(1.0, np.abs(want_r2))
    e_r[~np.isfinite(r)] = np.inf
    e_r2[~np.isfinite(r2)] = np.inf
    return float(e_r.max()), float(e_r2.max())


def assert_entrywise(r, r2, want_r, want_r2, what='', tol=TOL):
    """Every entry within ``tol`` (never norm-wise); prints and returns the largest errors."""
    e_r, e_r2 = errors(r, r2, want_r, want_r2)
    print('{}: max |dr| {:.2e}  max |dr2| / max(1, |r2|) {:.2e}'.format(what, e_r, e_r2))
    assert e_r <= tol, '{}: pearson_r off by {:.3e} in one entry (tol {:g})'.format(what, e_r, tol)
    assert e_r2 <= tol, '{}: r_squared off by {:.3e} in one entry (tol {:g})'.format(what, e_r2, tol)
    return e_r, e_r2


# ---------------------------------------------------------------------------
# the cases: the smallest shapes that reach each edge of the device path
# ---------------------------------------------------------------------------

def _case(S, B, T, groups, n_cond, m, cov=False, deficient=False, seed=0, hand=False):
    return dict(S=S, B=B, T=T, groups=list(groups), n_cond=n_cond, m=m, cov=cov, deficient=deficient, seed=seed,
                hand=hand)


CASES = {
    # J = 1: many splits a group; two passes, the last one ends in a partly filled group
    'E1': _case(60, 150, 4, [60], 1, 250),
    # J = 4, unequal cells; two passes
    'E2': _case(64, 90, 3, [14, 18], 2, 70),
    # J = 16 cells (the moment tiles bound the group); two passes
    'E3': _case(320, 130, 3, [20] * 8, 2, 20),
    # covariance: the moment rows are planned in for the call only
    'E4': _case(56, 70, 3, [12, 16], 2, 12, cov=True),
    # T' = 63 / 64 / 65: Jacobi vs Householder + QL in the mode that returns V and d; B one past a 128-column block
    'E5_63': _case(200, 257, 63, [200], 1, 3),
    'E5_64': _case(200, 257, 64, [200], 1, 3),
    'E5_65': _case(200, 257, 65, [200], 1, 3),
    # S one past / one short of the 64-row blocks of the product Q = Rs Xc^T
    'E6_65': _case(65, 130, 4, [65], 1, 5),
    'E6_127': _case(127, 130, 4, [127], 1, 5),
    # the design of E2 under hand-built, unbalanced masks (hand_masks)
    'E7': _case(64, 90, 3, [14, 18], 2, 4, hand=True),
    # T' = 10 > B = 7: L = B
    'E8': _case(60, 7, 5, [30, 30], 1, 5),
    # T' = 200: the 16-tile block
    'E9': _case(300, 260, 100, [150], 2, 3),
    # T' = 360 > 352: sliced; slice 0 ends at row 352, inside cell 11 (rows 330 .. 359)
    'E10': _case(552, 400, 30, [46] * 3, 4, 2),
    # T' = 400: sliced; cell 3 (rows 300 .. 399) straddles; 105 training rows per cell: full rank
    'E11_corr': _case(560, 450, 100, [140, 140], 2, 2),
    'E11_cov': _case(560, 450, 100, [140, 140], 2, 2, cov=True),
    # rank deficient: 9 training rows per cell (rank 8 each), 32 of 40 latent variables live
    'E12': _case(48, 200, 10, [12, 12], 2, 4, deficient=True),
    # rank deficient, one cell: 12 training rows, 11 of 12 live
    'E13': _case(16, 200, 12, [16], 1, 4, deficient=True),
}
FULL_RANK = [k for k, c in CASES.items() if not c['deficient']]
DEFICIENT = [k for k, c in CASES.items() if c['deficient']]
TEST_SIZE = 0.25


def spec_of(case):
    return ref.Spec('behavioral', case['groups'], case['n_cond'], case['cov'])


def data(S, B, T, seed=0, signal=0.5):
    """As ``_data`` of tests/test_gpu_kernels.py: X columns with a mean offset, Y with signal from X."""
    rs = np.random.RandomState(seed)
    X = rs.randn(S, B) + 3.0 * rs.rand(1, B)
    Y = rs.randn(S, T) + 1.5
    k = min(T, B)
    Y[:, :k] += signal * X[:, :k]
    return X, Y


def split_masks(case, m=None, seed=None):
    """(S, m) training masks from the front-end's own generator (the reference's gen_splits)."""
    from pypyls_amd import resampling as rsmp
    return rsmp.gen_splits(case['groups'], case['n_cond'], case['m'] if m is None else m,
                           seed=case['seed'] + 11 if seed is None else seed, test_size=TEST_SIZE)


def hand_masks(case):
    """Unbalanced masks on the cells of E2 / E7 (14, 14, 18, 18 rows): column 0 leaves cell 0 without a test row,
    column 1 gives cell 1 a single test row, column 2 puts all its test rows into cell 2, column 3 has the minimum of
    three test rows."""
    cells = np.repeat(case['groups'], case['n_cond'])
    start = np.concatenate([[0], np.cumsum(cells)[:-1]])
    test_rows = [
        {1: [0, 5, 13], 2: [2, 9, 17], 3: [1, 4, 8, 16]},
        {0: [3, 6, 12], 1: [7], 2: [0, 10, 11], 3: [5, 13, 17]},
        {2: [1, 4, 8, 12, 15]},
        {0: [2], 1: [11], 3: [6]},
    ]
    masks = np.ones((int(cells.sum()), len(test_rows)), dtype=bool)
    for i, rows in enumerate(test_rows):
        for j, local in rows.items():
            masks[start[j] + np.asarray(local), i] = False
    return masks


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> spec, X, Y, masks of one case, built once and shared: callers do not write to them (X and Y stay writable
    only because the engine hands them to torch.from_numpy, which warns about read-only arrays)."""
    case = CASES[name]
    X, Y = data(case['S'], case['B'], case['T'], seed=case['seed'])
    masks = hand_masks(case) if case['hand'] else split_masks(case)
    masks.setflags(write=False)
    return spec_of(case), X, Y, masks


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> pearson_r (T, m), r_squared (T, m), [info]: computed once and shared by the tests of a session."""
    spec, X, Y, masks = problem(name)
    r, r2, info = crossval(spec, X, Y, masks)
    r.setflags(write=False)
    r2.setflags(write=False)
    return r, r2, info


def slices_of(Tp, T, J):
    """The row slices [(row0, rows, cell0, ncell)] of a resample whose T' rows do not fit one block, as plan_groups
    (csrc/plsx_core.hip) cuts them with the per-cell moment rows planned in: greedily the longest range of whole
    16-row tiles that fits 24 tiles together with two moment tiles per 16 cells it touches.  [] when one block holds
    the resample (T' <= 352 with moment rows)."""
    if -(-Tp // 16) + 2 * -(-J // 16) <= 24 and -(-J // 16) * 16 <= 48:
        return []
    out, a = [], 0
    while a < Tp:
        for dt in range(24, 0, -1):
            b = min(Tp, a + dt * 16)
            ncell = (b - 1) // T - a // T + 1
            t2 = -(-ncell // 16)
            if -(-(b - a) // 16) + 2 * t2 <= 24 and t2 <= 3:
                out.append((a, b - a, a // T, ncell))
                a = b
                break
        else:
            raise ValueError('no slice fits')
    return out
