"""Expected values of pls_da's cross-validated one-vs-rest AUC counts, written on the CPU oracle (oracle/cpu_ref.py:
simpls, get_mask) exactly as tests/discriminant_expect.da_expected forms its predictions.  Shared by
tests/test_discriminant_auc_host.py and tests/test_gpu_discriminant_auc.py; not a test module.

The definition.  For one fit, a component count c and a class g, over the usable test positions: ``pos`` those whose
true class is g (under a permutation the true class of position p is codes[perm[p]], usability get_mask(X, Y[perm])),
``neg`` the others, ``v[p] = yhat_c[p][g]`` the prediction of the raw indicator,

    u2[g]    = sum over i in pos, j in neg of (2 if v[i] > v[j], 1 if v[i] == v[j], else 0)
    pairs[g] = |pos| * |neg|
    auc[g]   = u2[g] / (2 * pairs[g])                NaN where pairs[g] == 0

-- Mann-Whitney with ties counted one half.  A comparison with a NaN prediction is false both ways: such a pair stays
in ``pairs`` and adds nothing to ``u2``.  The macro average is the mean of auc[g] over the classes with pairs[g] > 0,
NaN if there is none.

The comparison these values serve is EXACT integer equality of counts.  What keeps that honest is the pair margin: the
smallest |v[i] - v[j]| over all counted pairs of opposite membership whose gap exceeds ``tie_tol``.  The device's
predictions agree with the oracle's to about 1e-10 (the figure discriminant_expect.py states), so a margin of at least
PAIR_MARGIN = 1e-7, three orders above it, means no ordering can differ; every test that compares counts asserts it
for its own input.  ``tie_tol`` is 0 except where a test plants identical rows: there the oracle calls a gap of at most
tie_tol a tie, and the margin is taken over the remaining pairs."""
import numpy as np

from oracle import cpu_ref as ref

from discriminant_expect import one_hot

PAIR_MARGIN = 1e-7


def pair_counts(v, member, tie_tol=0.0):
    """v (n,) scores, member (n,) bool -> (u2, pairs, margin) of the members against the others."""
    v, member = np.asarray(v, dtype=float), np.asarray(member, dtype=bool)
    vi, vj = v[member][:, None], v[~member][None, :]
    pairs = vi.shape[0] * vj.shape[1]
    if pairs == 0:
        return 0, 0, np.inf
    with np.errstate(invalid='ignore'):
        d = vi - vj                                                   # NaN where either is: neither > nor ==
        tie = np.abs(d) <= tie_tol
        gt = (d > 0) & ~tie
        far = np.abs(d)[~tie & ~np.isnan(d)]
    return int(2 * gt.sum() + tie.sum()), int(pairs), float(far.min()) if far.size else np.inf


def auc_expected(X, codes, masks, k, perm=None, tie_tol=0.0):
    """X (S, B), codes (S,) int class codes 0 .. G - 1, masks (S, n) bool with True = training row, perm (S,) a
    permutation of the rows of Y or None.  Returns dict(counts (G, 2, k, n) int64 -- [class, (u2, pairs), c - 1, split]
    -- and margin, the pair margin)."""
    X, codes = np.asarray(X, dtype=float), np.asarray(codes, dtype=int)
    masks = np.asarray(masks, dtype=bool)
    G = int(codes.max()) + 1
    true = codes if perm is None else codes[np.asarray(perm)]
    Y = one_hot(true, G)
    ok = ref.get_mask(X, Y)
    n = masks.shape[1]
    counts = np.zeros((G, 2, k, n), dtype=np.int64)
    margin = np.inf
    for s in range(n):
        tr, te = masks[:, s] & ok, ~masks[:, s] & ok
        fit = ref.simpls(X[tr], Y[tr], k)
        xm, ym = X[tr].mean(axis=0), Y[tr].mean(axis=0)
        scores = (X[te] - xm) @ fit['x_weights']                     # (n_te, k)
        Q = fit['y_loadings']                                        # (G, k)
        for c in range(1, k + 1):
            pred = ym + scores[:, :c] @ Q[:, :c].T
            for g in range(G):
                u2, pairs, m = pair_counts(pred[:, g], true[te] == g, tie_tol)
                counts[g, 0, c - 1, s], counts[g, 1, c - 1, s] = u2, pairs
                margin = min(margin, m)
    return dict(counts=counts, margin=margin)


def auc_perm_expected(X, codes, masks, k, perms, tie_tol=0.0):
    """perms (S, P): per permutation the counts summed over the splits, (G, 2, k, P), and the smallest pair margin."""
    out = [auc_expected(X, codes, masks, k, perm=perms[:, p], tie_tol=tie_tol) for p in range(perms.shape[1])]
    return dict(counts=np.stack([o['counts'].sum(axis=-1) for o in out], axis=-1),
                margin=min(o['margin'] for o in out))


def auc_of(counts):
    """The definition's last lines, plainly: counts (G, 2, ...) -> (auc (G, ...), macro (...))."""
    counts = np.asarray(counts)
    G, rest = counts.shape[0], counts.shape[2:]
    auc = np.full((G,) + rest, np.nan)
    macro = np.full(rest, np.nan)
    for idx in np.ndindex(*rest):
        vals = []
        for g in range(G):
            u2, pairs = int(counts[(g, 0) + idx]), int(counts[(g, 1) + idx])
            if pairs > 0:
                auc[(g,) + idx] = u2 / (2 * pairs)
                vals.append(auc[(g,) + idx])
        if vals:
            macro[idx] = sum(vals) / len(vals)
    return auc, macro


# the small generator of tests/test_gpu_discriminant.py (_design, EDGES, _edge_case), copied: the same inputs

def design(S, B, sizes, seed, shift=0.6, nan_x=()):
    """Class means shifted on a tenth of the features; rows in random order."""
    rs = np.random.RandomState(seed)
    y = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    X = rs.randn(S, B)
    nf = max(2, B // 10)
    X[:, :nf] += (shift * rs.randn(len(sizes), nf))[y]
    for i in nan_x:
        X[i] = np.nan
    return X, y, rs


EDGES = [  # S, sizes, k, nan rows: lane-stride tails (63, 65, 130), k = 1, 4, 5, the register bounds (G = 2, 3 -> 4; 17 -> 32; 32)
    (63, (33, 30), 1, (5,)),
    (65, (25, 22, 18), 4, (0, 64)),
    (130, tuple([8] * 14 + [6] * 3), 5, (17, 99)),
    (130, tuple([5] * 2 + [4] * 30), 5, (3,)),
]
EDGE_IDS = ['S63-G2-k1', 'S65-G3-k4', 'S130-G17-k5', 'S130-G32-k5']


def edge_case(S, sizes, k, nan_x, seed=0):
    """5 splits: the second block of four waves has three idle ones.  Split 0's test side lacks class 0 altogether."""
    X, y, rs = design(S, 48, sizes, 1000 + S + len(sizes) + seed, nan_x=nan_x)
    masks = np.ones((S, 5), dtype=bool)
    for s in range(5):
        for g in range(len(sizes)):
            rows = np.flatnonzero(y == g)
            if s == 0 and g == 0:
                continue
            masks[rs.choice(rows, size=max(1, int(round(len(rows) * 0.3))), replace=False), s] = False
    return X, y, masks
