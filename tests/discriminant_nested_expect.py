"""Expected values of pls_da's nested cross-validation of n_components (inner_split=, inner_select=), written on the CPU
oracle (oracle/cpu_ref.py) through tests/discriminant_expect.da_expected, tests/discriminant_auc_expect.auc_expected and
tests/regression_nested_expect.fit_scores.  Shared by tests/test_discriminant_nested_host.py and
tests/test_gpu_discriminant_nested.py; not a test module.

Codes as in regression_nested_expect: 1 = training row, 0 = test row, 2 = on neither side; ``codes`` (S, n, 1 + ni),
``[:, s, 0]`` outer split s, ``[:, s, 1:]`` its inner folds.  The definition, per outer split s:

    conf_j (k, G, G)            the confusion of inner fit j = 1 .. ni, as da_expected counts it
    inner_confusion[:, :, c-1]  = sum_j conf_j[c-1]                                        (integers)
    crit[c]                     'accuracy': trace / total, one division; 'balanced_accuracy': balanced() below -- an
                                explicit loop, the recalls added one by one in ascending g from 0.0 (np.sum's pairwise
                                summation would reorder G >= 8 terms); 'mse': inner_mse[c], smallest wins
    ncomp                       the first optimum over c = 1 .. k, a NaN never wins; 0 where the pooled block has no
                                counted row (mse: the minimum is not finite) -- counts zero, scores NaN
    confusion, auc_counts,      the outer fit's at c = ncomp
    r, r2, mse

A fit whose codes hold 2 is handed to da_expected / auc_expected with those rows of X set to NaN: get_mask then keeps
them on neither side, which is what code 2 means.  The counts are compared EXACTLY, so every fit -- the inner ones
included -- contributes to ``margin`` (discriminant_expect.MARGIN) and ``pair_margin``
(discriminant_auc_expect.PAIR_MARGIN); the 'mse' rule has regression_nested_expect.selection_gap on ``inner_mse``."""
import numpy as np

import discriminant_auc_expect as ae
import discriminant_expect as de
import regression_nested_expect as ne

RULES = ('balanced_accuracy', 'accuracy', 'mse')


def accuracy(conf):
    """trace / total of conf (G, G), one division; NaN without a counted row."""
    conf = np.asarray(conf)
    trace, total = int(np.trace(conf)), int(conf.sum())
    return trace / total if total else float('nan')


def balanced(conf):
    """The recalls of the classes with a counted row, added one by one in ascending g starting from 0.0, divided by the
    number of such classes; NaN without one."""
    conf = np.asarray(conf)
    acc, present = 0.0, 0
    for g in range(conf.shape[0]):
        rowsum = int(conf[g].sum())
        if rowsum > 0:
            acc = acc + int(conf[g, g]) / rowsum
            present += 1
    return acc / present if present else float('nan')


def criterion(conf, rule):
    return accuracy(conf) if rule == 'accuracy' else balanced(conf)


def select(crit, smaller=False):
    """crit (k,) of c = 1 .. k: the first optimum, a NaN never wins -> c, or 0 where the optimum is NaN (smaller: not
    finite)."""
    best = 0
    for c in range(1, len(crit)):
        if (crit[c] < crit[best]) if smaller else (crit[c] > crit[best]):
            best = c
    ok = np.isfinite(crit[best]) if smaller else not np.isnan(crit[best])
    return best + 1 if ok else 0


def _fits(X, cls, code_cols, k, perm, auc, tie_tol):
    """The fits of the columns of code_cols (S, m) that share their rows of code 2 -> confusion (G, G, k, m), AUC counts
    (G, 2, k, m) or None, margin, pair margin."""
    code_cols = np.asarray(code_cols)
    off = (code_cols == 2).any(axis=1)
    assert np.array_equal(code_cols == 2, np.broadcast_to(off[:, None], code_cols.shape))
    Xm = np.array(X, dtype=float)
    Xm[off] = np.nan
    d = de.da_expected(Xm, cls, code_cols == 1, k, perm=perm)
    a = ae.auc_expected(Xm, cls, code_cols == 1, k, perm=perm, tie_tol=tie_tol) if auc else None
    return d['confusion'], (a['counts'] if auc else None), d['margin'], (a['margin'] if auc else np.inf)


def nested_da_expected(X, cls, codes, k, rule='balanced_accuracy', perm=None, auc=False, tie_tol=0.0):
    """One arrangement: X (S, B), cls (S,) class codes, codes (S, n, 1 + ni), perm (S,) or None (the true class of
    position p is cls[perm[p]]).  -> dict(inner_confusion (G, G, k, n), inner_mse (k + 1, n), crit (k, n), ncomp (n,),
    confusion (G, G, n), auc_counts (G, 2, n) or None, r, r2 (G, n), mse (n,), margin, pair_margin)."""
    assert rule in RULES, rule
    X, cls, codes = np.asarray(X, dtype=float), np.asarray(cls, dtype=int), np.asarray(codes)
    G, n, ni = int(cls.max()) + 1, codes.shape[1], codes.shape[2] - 1
    Y = de.one_hot(cls if perm is None else cls[np.asarray(perm)], G)
    out = dict(inner_confusion=np.zeros((G, G, k, n), dtype=np.int64), inner_mse=np.zeros((k + 1, n)),
               crit=np.zeros((k, n)), ncomp=np.zeros(n, dtype=np.int64), confusion=np.zeros((G, G, n), dtype=np.int64),
               auc_counts=np.zeros((G, 2, n), dtype=np.int64) if auc else None, r=np.full((G, n), np.nan),
               r2=np.full((G, n), np.nan), mse=np.full(n, np.nan), margin=np.inf, pair_margin=np.inf)
    for s in range(n):
        iconf, _, m_in, _ = _fits(X, cls, codes[:, s, 1:], k, perm, False, tie_tol)
        for j in range(ni):                                          # (integer sums, members ascending)
            out['inner_confusion'][:, :, :, s] += iconf[:, :, :, j]
        acc = np.zeros(k + 1)
        for j in range(1, ni + 1):
            _, _, sse, nte = ne.fit_scores(X, Y, codes[:, s, j], k)
            acc = acc + ne.fit_mse(sse, nte)
        out['inner_mse'][:, s] = acc / ni
        if rule == 'mse':
            out['crit'][:, s] = out['inner_mse'][1:, s]
            c = select(out['crit'][:, s], smaller=True)
        else:
            out['crit'][:, s] = [criterion(out['inner_confusion'][:, :, j, s], rule) for j in range(k)]
            c = select(out['crit'][:, s])
        oconf, oauc, m_out, pm = _fits(X, cls, codes[:, s, :1], k, perm, auc, tie_tol)
        out['margin'] = min(out['margin'], m_in, m_out)
        out['pair_margin'] = min(out['pair_margin'], pm)
        out['ncomp'][s] = c
        if c:
            out['confusion'][:, :, s] = oconf[:, :, c - 1, 0]
            if auc:
                out['auc_counts'][:, :, s] = oauc[:, :, c - 1, 0]
            fr, fr2, sse, nte = ne.fit_scores(X, Y, codes[:, s, 0], k)
            out['r'][:, s], out['r2'][:, s], out['mse'][s] = fr[:, c - 1], fr2[:, c - 1], ne.fit_mse(sse, nte)[c]
    return out


def nested_da_perm_expected(X, cls, codes, k, perms, rule='balanced_accuracy', auc=False, tie_tol=0.0):
    """perms (S, P): the whole procedure per permutation.  -> dict(confusion (G, G, P) and auc_counts (G, 2, P) summed
    over the outer splits, ncomp (k, P) how many outer splits chose c, r, r2 (G, P), mse (P,) the split means, inner_mse
    (k + 1, n, P), choice (n, P) the selected counts, margin, pair_margin)."""
    perms = np.asarray(perms)
    outs = [nested_da_expected(X, cls, codes, k, rule, perm=perms[:, p], auc=auc, tie_tol=tie_tol)
            for p in range(perms.shape[1])]
    cnt = np.zeros((k, len(outs)), dtype=np.int64)
    for p, o in enumerate(outs):
        for c in o['ncomp']:
            if c:
                cnt[c - 1, p] += 1
    return dict(confusion=np.stack([o['confusion'].sum(axis=-1) for o in outs], axis=-1),
                auc_counts=np.stack([o['auc_counts'].sum(axis=-1) for o in outs], axis=-1) if auc else None,
                ncomp=cnt, choice=np.stack([o['ncomp'] for o in outs], axis=-1),
                r=np.stack([ne.split_mean(o['r']) for o in outs], axis=-1),
                r2=np.stack([ne.split_mean(o['r2']) for o in outs], axis=-1),
                mse=np.array([ne.split_mean(o['mse']) for o in outs]),
                inner_mse=np.stack([o['inner_mse'] for o in outs], axis=-1),
                margin=min(o['margin'] for o in outs), pair_margin=min(o['pair_margin'] for o in outs))


def pvals_ge(obs, null):
    """(#{null >= obs} + 1) / (P + 1) over the last axis; NaN where obs is NaN."""
    obs, null = np.asarray(obs, dtype=float), np.asarray(null, dtype=float)
    with np.errstate(invalid='ignore'):
        p = ((null >= obs[..., None]).sum(axis=-1) + 1) / (null.shape[-1] + 1)
    return np.where(np.isnan(obs), np.nan, p)


def scores(conf):
    """conf (G, G, ...) -> accuracy, balanced accuracy of every block, by the two functions above."""
    conf = np.asarray(conf)
    rest = conf.shape[2:]
    acc, bal = np.zeros(rest), np.zeros(rest)
    for idx in np.ndindex(*rest):
        acc[idx], bal[idx] = accuracy(conf[(slice(None), slice(None)) + idx]), balanced(conf[(slice(None), slice(None)) + idx])
    return acc, bal


def given_folds(cls, n, ni, seed, test_frac=0.3):
    """Stratified outer masks (S, n) bool and inner codes (S, n, ni) uint8 drawn with numpy alone: per class about
    test_frac of its rows on the test side, of the whole set for the outer split and of its training rows for a fold."""
    cls = np.asarray(cls)
    rs = np.random.RandomState(seed)
    S = len(cls)
    masks = np.ones((S, n), dtype=bool)
    inner = np.full((S, n, ni), 2, dtype=np.uint8)
    for s in range(n):
        for g in np.unique(cls):
            rows = np.flatnonzero(cls == g)
            masks[rs.choice(rows, size=max(1, int(round(len(rows) * test_frac))), replace=False), s] = False
        for j in range(ni):
            inner[masks[:, s], s, j] = 1
            for g in np.unique(cls):
                rows = np.flatnonzero((cls == g) & masks[:, s])
                inner[rs.choice(rows, size=max(1, int(round(len(rows) * test_frac))), replace=False), s, j] = 0
    return masks, inner
