"""
``pls_da``: PLS discriminant analysis -- SIMPLS on the indicator matrix of the class labels, the class of a row read
off the largest predicted indicator -- with cross-validated accuracy, balanced accuracy and confusion matrices and
their permutation test, and on request the cross-validated one-vs-rest AUC of every class with its own.

The model IS ``pls_regression(X, one_hot(y))``: ``pls_da`` validates the labels, codes them and passes everything on to
that code path, so everything ``pls_regression`` returns (weights, scores, VIP, coefficients with their bootstrap
ratios, intervals and p-values, the regression scores of the cross-validation) is returned unchanged.  What is added:

  * the train / test splits are stratified by class (``resampling.gen_stratified_splits``);
  * the (split) and (permutation, split) fits of the cross-validation are classified where they live, on the device
    (plsx_simpls_set_classes / plsx_simpls_cv_class_begin; csrc/plsx_simpls.h, k_sd_cv_class): only integer confusion
    counts come back, per split for the observed labels and summed over the splits per permutation;
  * ``auc=True``: the same fits also rank their test rows (plsx_simpls_cv_auc_begin; k_sd_cv_auc) -- per class the
    ordered pairs (row of the class, other row) that its predicted indicator puts in the right order, again integers;
  * ``cv_predict=``: the predicted indicators of every held-out row themselves (plsx_simpls_cv_pred_begin;
    k_sd_cv_pred), their first maximum ``cvres.predicted``, and :func:`roc_curve` on the host;
  * ``inner_split=``: nested cross-validation of ``n_components`` -- inner folds inside the training rows of every
    split choose the component count on their pooled confusion counts (or the inner mse), the outer test rows score
    the chosen model (plsx_simpls_cvn_class_begin; k_sd_cvn_class_select, k_sd_cvn_class_reduce);
  * :func:`predict_class` for new rows.

There is no split-half reliability (``n_split``) here: the correlation between two halves of indicator loadings answers
no question anyone asks of a classifier.  Nor ``rotate`` / ``aggfunc`` / 3-D Y, which have no meaning for labels.
"""
import numpy as np

from .regression import _usable_rows, pls_regression, predict

MAX_CLASSES = 32            # the bound of k_sd_cv_class (plsx_simpls_set_classes: PLSX_ERR_UNSUPPORTED beyond it)


def scores_from_confusion(conf):
    """conf (G, G, ...) counts, [true class, predicted class, ...] -> (accuracy, balanced_accuracy), each of shape ``...``.

    ``accuracy = trace / total``; ``balanced_accuracy`` is the mean, over the classes that have at least one counted
    row, of ``conf[g, g] / conf[g, :].sum()`` (the recall of class g) -- a class without a counted row is left out of
    the mean, it does not count as a recall of zero.  No counted row at all gives NaN."""
    conf = np.asarray(conf)
    if conf.ndim < 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError('Expected confusion counts of shape (G, G, ...), got {}'.format(conf.shape))
    conf = conf.astype(np.float64)
    hits = np.einsum('gg...->g...', conf)                            # (G, ...)
    per_class = conf.sum(axis=1)                                     # (G, ...) counted rows of every true class
    with np.errstate(divide='ignore', invalid='ignore'):
        accuracy = hits.sum(axis=0) / per_class.sum(axis=0)
        present = per_class > 0
        recall = np.where(present, hits / np.where(present, per_class, 1.0), 0.0)
        balanced = recall.sum(axis=0) / present.sum(axis=0)
    return accuracy, balanced


def pvals_from_null(observed, null):
    """``(#{null >= observed} + 1) / (P + 1)`` along the last axis of ``null`` (..., P).  ``>=``, not the strict ``>`` of
    ``cvres.pearson_r_pvals``: accuracy is a ratio of small integers, an exact tie between a permutation and the observed
    labels has positive probability, and counting it as "not at least as good" would be anti-conservative."""
    observed, null = np.asarray(observed, dtype=np.float64), np.asarray(null, dtype=np.float64)
    return (np.sum(null >= observed[..., None], axis=-1) + 1) / (null.shape[-1] + 1)


def confusion_results(blocks, perm_blocks=None):
    """The keys ``pls_da`` adds to ``cvres`` from what the device counted: blocks (n, k, G, G) per split and, with
    ``cv_perm``, perm_blocks (P, k, G, G) summed over the splits of every permutation (float64 holding integers)."""
    conf = np.ascontiguousarray(np.rint(np.asarray(blocks)).astype(np.int64).transpose(2, 3, 1, 0))    # (G, G, k, n)
    acc, bal = scores_from_confusion(conf)
    out = dict(confusion=conf, accuracy=acc, balanced_accuracy=bal)
    if perm_blocks is not None:
        pconf = np.ascontiguousarray(np.rint(np.asarray(perm_blocks)).astype(np.int64).transpose(2, 3, 1, 0))
        pacc, pbal = scores_from_confusion(pconf)
        # the pooled statistic: the same functional of the observed data, the confusion summed over the splits
        oacc, obal = scores_from_confusion(conf.sum(axis=-1))
        out.update(perm_confusion=pconf, perm_accuracy=pacc, perm_balanced_accuracy=pbal,
                   accuracy_pvals=pvals_from_null(oacc, pacc), balanced_accuracy_pvals=pvals_from_null(obal, pbal))
    return out


def auc_from_counts(counts):
    """counts (G, 2, ...) -- ``[g, 0] = u2``: over the pairs (counted row of class g, counted row of another class), 2
    where the predicted indicator of class g is larger on the first, 1 where the two are equal; ``[g, 1] = pairs``: the
    number of such pairs -- -> ``(auc, auc_macro)`` of shapes (G, ...) and ``...``.

    ``auc[g] = u2 / (2 pairs)``: the one-vs-rest area under the ROC curve of class g (Mann-Whitney, ties one half), NaN
    where there is no pair -- no counted row of the class, or none of any other.  ``auc_macro`` is the mean of ``auc[g]``
    over the classes that have a pair, NaN if none has."""
    counts = np.asarray(counts)
    if counts.ndim < 2 or counts.shape[1] != 2:
        raise ValueError('Expected AUC counts of shape (G, 2, ...), got {}'.format(counts.shape))
    counts = counts.astype(np.float64)
    u2, pairs = counts[:, 0], counts[:, 1]
    present = pairs > 0
    auc = np.where(present, u2 / np.where(present, 2.0 * pairs, 1.0), np.nan)
    n = present.sum(axis=0)
    macro = np.where(n > 0, np.where(present, auc, 0.0).sum(axis=0) / np.where(n > 0, n, 1), np.nan)
    return auc, macro


def _pvals_nan(observed, null):
    """:func:`pvals_from_null`, NaN where the observed value is NaN (a NaN in the null is not ``>=`` anything)."""
    observed = np.asarray(observed, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        p = pvals_from_null(observed, null)
    return np.where(np.isnan(observed), np.nan, p)


def auc_results(blocks, perm_blocks=None):
    """The keys ``pls_da(auc=True)`` adds to ``cvres`` from what the device counted: blocks (n, k, G, 2) per split and,
    with ``cv_perm``, perm_blocks (P, k, G, 2) summed over the splits of every permutation (float64 holding integers)."""
    cnt = np.ascontiguousarray(np.rint(np.asarray(blocks)).astype(np.int64).transpose(2, 3, 1, 0))     # (G, 2, k, n)
    auc, macro = auc_from_counts(cnt)
    out = dict(auc_counts=cnt, auc=auc, auc_macro=macro)
    if perm_blocks is not None:
        pcnt = np.ascontiguousarray(np.rint(np.asarray(perm_blocks)).astype(np.int64).transpose(2, 3, 1, 0))
        pauc, pmacro = auc_from_counts(pcnt)
        # the pooled statistic: the same functional of the observed data, the counts summed over the splits
        oauc, omacro = auc_from_counts(cnt.sum(axis=-1))
        out.update(perm_auc_counts=pcnt, perm_auc=pauc, perm_auc_macro=pmacro,
                   auc_pvals=_pvals_nan(oauc, pauc), auc_macro_pvals=_pvals_nan(omacro, pmacro))
    return out


INNER_SELECT = ('balanced_accuracy', 'accuracy', 'mse')     # the criteria of the nested selection; the call names one


def nested_criterion(conf, rule):
    """The criterion of the nested selection on one block of counts conf (G, G) [true class, predicted class]:
    ``'accuracy'``: trace / total, one division; ``'balanced_accuracy'``: the recalls ``conf[g, g] / conf[g].sum()`` of
    the classes with a counted row, added one by one in ascending g starting from 0.0, divided by their number -- the
    operations of the device kernel (k_sd_cvn_class_select) in its order, so the two agree to the bit.  NaN for a block
    without a counted row."""
    conf = np.asarray(conf)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1]:
        raise ValueError('Expected confusion counts of shape (G, G), got {}'.format(conf.shape))
    G = conf.shape[0]
    rows = [int(sum(int(v) for v in conf[g])) for g in range(G)]
    with np.errstate(divide='ignore', invalid='ignore'):
        if rule == 'accuracy':
            return float(np.float64(sum(int(conf[g, g]) for g in range(G))) / np.float64(sum(rows)))
        if rule == 'balanced_accuracy':
            acc, present = np.float64(0.0), 0
            for g in range(G):
                if rows[g] > 0:
                    acc = acc + np.float64(int(conf[g, g])) / np.float64(rows[g])
                    present += 1
            return float(acc / np.float64(present))
    raise ValueError("`rule` must be 'accuracy' or 'balanced_accuracy'; got {!r}".format(rule))


def nested_select(crit, smaller=False):
    """The selection rule on crit (k,), the criterion of c = 1 .. k components: the first maximum (``smaller``: the first
    minimum, the rule of the inner mse) -- ties go to the smaller model, a NaN never wins.  -> c, or 0 where the
    optimum is NaN (``smaller``: not finite): the group is undefined."""
    crit = np.asarray(crit, dtype=np.float64)
    best = 0
    for c in range(1, len(crit)):
        if (crit[c] < crit[best]) if smaller else (crit[c] > crit[best]):
            best = c
    ok = np.isfinite(crit[best]) if smaller else not np.isnan(crit[best])
    return best + 1 if ok else 0


def nested_results(blocks, inner_blocks, auc_blocks=None, perm_blocks=None, perm_auc_blocks=None):
    """The keys ``pls_da(inner_split=)`` adds to ``cvres`` from what the device selected and counted: blocks (n, G, G)
    the outer fits' confusion at the selected component count, inner_blocks (n, k, G, G) the confusion pooled over the
    inner folds, auc_blocks (n, G, 2); with ``cv_perm``, perm_blocks (P, G, G) / perm_auc_blocks (P, G, 2) summed over the
    outer splits of every permutation (float64 holding integers)."""
    def ints(a, axes):
        return np.ascontiguousarray(np.rint(np.asarray(a)).astype(np.int64).transpose(axes))
    conf = ints(blocks, (1, 2, 0))                                   # (G, G, n)
    iconf = ints(inner_blocks, (2, 3, 1, 0))                         # (G, G, k, n)
    acc, bal = scores_from_confusion(conf)
    iacc, ibal = scores_from_confusion(iconf)
    out = dict(nested_confusion=conf, nested_accuracy=acc, nested_balanced_accuracy=bal, inner_confusion=iconf,
               inner_accuracy=iacc, inner_balanced_accuracy=ibal)
    if auc_blocks is not None:
        cnt = ints(auc_blocks, (1, 2, 0))                            # (G, 2, n)
        auc, macro = auc_from_counts(cnt)
        out.update(nested_auc_counts=cnt, nested_auc=auc, nested_auc_macro=macro)
    if perm_blocks is not None:
        pconf = ints(perm_blocks, (1, 2, 0))                         # (G, G, P)
        pacc, pbal = scores_from_confusion(pconf)
        # the pooled statistic: the same functional of the observed data, the confusion summed over the outer splits
        oacc, obal = scores_from_confusion(conf.sum(axis=-1))
        out.update(perm_nested_confusion=pconf, perm_nested_accuracy=pacc, perm_nested_balanced_accuracy=pbal,
                   nested_accuracy_pvals=float(_pvals_nan(oacc, pacc)),
                   nested_balanced_accuracy_pvals=float(_pvals_nan(obal, pbal)))
        if auc_blocks is not None and perm_auc_blocks is not None:
            pcnt = ints(perm_auc_blocks, (1, 2, 0))                  # (G, 2, P)
            pauc, pmacro = auc_from_counts(pcnt)
            oauc, omacro = auc_from_counts(out['nested_auc_counts'].sum(axis=-1))
            out.update(perm_nested_auc_counts=pcnt, perm_nested_auc=pauc, perm_nested_auc_macro=pmacro,
                       nested_auc_pvals=_pvals_nan(oauc, pauc), nested_auc_macro_pvals=float(_pvals_nan(omacro, pmacro)))
    return out


def encode_labels(y, S=None):
    """y (S,) labels -> (classes (G,) sorted distinct labels, codes (S,) int64 positions in it).  ValueError for a y that
    is not 1-D (or not of length S), a NaN or None label, fewer than 2 or more than 32 classes."""
    y = np.asarray(y)
    if y.ndim != 1 or (S is not None and len(y) != S):
        raise ValueError('Provided `y` must be a 1-D array of one label per row of `X`{}; got shape {}'
                         .format('' if S is None else ' ({} rows)'.format(S), y.shape))
    if y.dtype == object:
        if any(v is None or (isinstance(v, (float, np.floating)) and np.isnan(v)) for v in y):
            raise ValueError('Provided `y` holds a None or NaN label; drop or label such rows before the call')
    elif y.dtype.kind in 'fc' and np.isnan(y).any():
        raise ValueError('Provided `y` holds a NaN label; drop or label such rows before the call')
    try:
        classes, codes = np.unique(y, return_inverse=True)
    except TypeError as exc:
        raise ValueError('Provided `y` holds labels that cannot be sorted: {}'.format(exc)) from exc
    G = len(classes)
    if G < 2:
        raise ValueError('Provided `y` holds {} distinct label(s); a discriminant analysis needs at least 2 classes'
                         .format(G))
    if G > MAX_CLASSES:
        raise ValueError('Provided `y` holds {} distinct labels; at most {} classes are supported, the bound of the '
                         'device\'s classification kernel (k_sd_cv_class)'.format(G, MAX_CLASSES))
    return classes, codes.reshape(-1).astype(np.int64)


def _label(classes, g):
    """Label g as a plain Python value, for messages."""
    return classes[g].item() if hasattr(classes[g], 'item') else classes[g]


def pls_da(X, y, *, n_components=None, n_perm=5000, n_boot=5000, ci=95, permsamples=None, bootsamples=None, seed=None,
           verbose=True, n_proc=None, test_split=0, test_size=0.25, cvsamples=None, cv_perm=0, cvpermsamples=None,
           coef_components=None, coef_ci=False, coef_perm=False, vip_components=None, auc=False, vip_perm=False,
           cv_predict=False, inner_split=0, innersamples=None, inner_select=None, **kwargs):
    """PLS discriminant analysis of the labels ``y`` (S,) on ``X`` (S, B).

    ``classes = np.unique(y)`` (integers, strings, booleans: anything numpy sorts), ``codes`` the position of every
    label in it, G = len(classes), 2 <= G <= 32.  The model is ``pls_regression(X, Y)`` with ``Y = one_hot(codes)``,
    (S, G) float64: every keyword above means what it means there and goes to the same code path, and every key that
    call returns is returned unchanged -- for the same ``cvsamples`` / ``cvpermsamples`` bit for bit.  ``vip_components``
    gives the usual feature-importance score of PLS-DA -- with ``vip_perm=True`` also its permutation p-values,
    ``permres.vip_pvals`` / ``vip_max`` / ``vip_pvals_fwe``, in place of the "VIP > 1" rule of thumb --,
    ``coef_components`` the model :func:`predict_class` applies.
    Added to the result: ``classes``.

    Cross-validation (``test_split`` > 0): the splits are STRATIFIED -- drawn with ``gen_splits(counts, 1, test_split,
    test_size=test_size)`` on the rows in class-sorted order (a stable argsort of the codes, ``counts`` the class sizes)
    and scattered back, at the place in the call's random stream where ``pls_regression`` draws its own, so every class
    keeps ceil or floor of ``n_g (1 - test_size)`` training rows -- or given as ``cvsamples``.  For a split and a
    component count c the predicted class of a usable test row is the first maximum (``np.argmax``: the lowest index on a
    tie) of its predicted indicators ``yhat_c`` -- training mean plus the first c scores times their y-loadings, the
    prediction ``cvres.pearson_r_ncomp`` scores.  ``cvres`` gains

        confusion          (G, G, k, test_split) int   [true class, predicted class, c - 1, split]
        accuracy           (k, test_split)             trace / total
        balanced_accuracy  (k, test_split)             mean recall over the classes with a counted test row

    (:func:`scores_from_confusion`).  Rows of X that are NaN throughout belong to neither side and are counted nowhere.

    ``auc=True`` (needs ``test_split`` > 0): the same fits also give the one-vs-rest area under the ROC curve of every
    class, which does not depend on where a threshold is placed and so does not move with class imbalance the way
    accuracy does.  For a split, a component count c and a class g, over the pairs (usable test row i of class g, usable
    test row j of another class) and with ``v = yhat_c[:, g]``, ``u2`` counts 2 where ``v[i] > v[j]`` and 1 where
    ``v[i] == v[j]`` (Mann-Whitney, ties one half), ``pairs`` the pairs.  ``cvres`` gains

        auc_counts         (G, 2, k, test_split) int   [class, (u2, pairs), c - 1, split]
        auc                (G, k, test_split)          u2 / (2 pairs); NaN where a split's test side lacks class g or
                                                       holds nothing else
        auc_macro          (k, test_split)             mean over the classes with a pair

    (:func:`auc_from_counts`) and, with ``cv_perm=P``, ``perm_auc_counts`` (G, 2, k, P) summed over the splits of a
    permutation, ``perm_auc`` (G, k, P) / ``perm_auc_macro`` (k, P) = ``auc_from_counts(perm_auc_counts)`` -- the pooled
    statistic -- and ``auc_pvals`` (G, k) / ``auc_macro_pvals`` (k,) against ``auc_from_counts(auc_counts.sum(-1))``, by
    the same ``>=`` rule as below; a NaN observed value gives a NaN p-value.  Without ``auc=True`` nothing is added and
    nothing else changes.

    ``cv_predict`` (needs ``test_split`` > 0; ``True`` for the full model or an int c, 1 <= c <= n_components; False, the
    default: nothing is added and nothing else changes): the predictions themselves.  ``cvres`` gains ``y_pred``
    (S, G, test_split), the predicted RAW indicators ``yhat_c`` of every usable test row of every split -- the values the
    argmax above is taken of and ``auc`` ranks; NaN on every other row --, ``y_pred_ncomp`` (test_split,) int32 and
    ``predicted`` (S, test_split) int32, the index into ``classes`` of the first maximum (-1 off the test rows), from
    which ``confusion[:, :, c - 1, s]`` can be recounted exactly.  :func:`roc_curve` draws the ROC curve of a class and a
    split from them.  ``'nested'`` (needs ``inner_split``): the model of ``nested_ncomp[s]`` components per split, from
    whose ``predicted`` ``nested_confusion[:, :, s]`` can be recounted exactly.

    Nested cross-validation of ``n_components``: ``inner_split=ni`` (needs ``test_split`` > 0; 0, the default: nothing is
    added, nothing is drawn and every array keeps its bits).  Picking the best row of ``balanced_accuracy`` (k,
    test_split) selects and scores on the same test rows.  Here ni inner folds INSIDE the training rows of every split
    choose c, and the split's test rows, which took no part in the choice, score the chosen model.  The inner folds are
    codes ``innersamples`` (S, test_split, ni) uint8 -- 1 = training row, 0 = test row, 2 = on neither side, exactly on
    the outer test rows -- given (needs ``cvsamples``) or drawn, STRATIFIED by class
    (``gen_stratified_splits(codes[rows], ni, test_size=test_size)`` on the training rows of every split, behind
    everything else a seeded call draws).  Per split s and c = 1 .. k the confusion counts of the ni inner fits are
    pooled, ``inner_confusion[:, :, c - 1, s]``, and ``inner_select`` names the criterion on them -- it has no default:
    ``pls_da(inner_split=ni)`` alone is refused as it was before the nested selection existed:

        'balanced_accuracy'  the recalls of the classes with a counted row, added in ascending class order and
                             divided by their number (:func:`nested_criterion`)
        'accuracy'           trace / total
        'mse'                ``inner_mse``, smallest wins: the rule of ``pls_regression(inner_split=)``

    ``nested_ncomp[s]`` is the FIRST optimum over c = 1 .. k (:func:`nested_select`): ties, common on counts, go to the
    smaller model, a NaN never wins; 0 where the pooled block has no counted row (mse: the minimum is not finite) --
    the split is then undefined, its scores NaN, its counts zero, and it counts nowhere under a permutation.  ``cvres``
    gains, at c = ``nested_ncomp[s]``,

        nested_confusion          (G, G, test_split) int
        nested_accuracy           (test_split,)            nested_balanced_accuracy likewise
        nested_auc_counts         (G, 2, test_split) int   with auc=True, and nested_auc (G, test_split), nested_auc_macro
        inner_confusion           (G, G, k, test_split) int, inner_accuracy / inner_balanced_accuracy (k, test_split)

    and the regression keys of the nested call as ``pls_regression`` returns them, at the c THIS selection chose:
    ``nested_ncomp``, ``nested_pearson_r``, ``nested_r_squared``, ``nested_mse``, ``inner_mse``, ``innersamples`` --
    one selection per call.  With ``cv_perm=P`` the WHOLE procedure, selection included, runs per permutation:
    ``perm_nested_confusion`` (G, G, P) summed over the outer splits, ``perm_nested_accuracy`` /
    ``perm_nested_balanced_accuracy`` (P,) the score of that sum, ``perm_nested_ncomp`` (k, P), the scalars
    ``nested_accuracy_pvals`` / ``nested_balanced_accuracy_pvals`` against
    ``scores_from_confusion(nested_confusion.sum(-1))`` by the ``>=`` rule below, with ``auc=True``
    ``perm_nested_auc_counts`` (G, 2, P), ``perm_nested_auc``, ``perm_nested_auc_macro``, ``nested_auc_pvals`` (G,),
    ``nested_auc_macro_pvals`` (a NaN observed value gives a NaN p-value), and the ``perm_nested_pearson_r`` ... keys of
    ``pls_regression``.  Not offered: selection on the AUC, a one-standard-error rule, ``confounds``.

    ``cv_perm=P``: the true class of position p under a permutation is ``codes[perm[p]]``.  The device returns, per
    permutation, the confusion SUMMED over the splits, and ``cvres`` gains ``perm_confusion`` (G, G, k, P),
    ``perm_accuracy`` / ``perm_balanced_accuracy`` (k, P) = ``scores_from_confusion(perm_confusion)`` -- the pooled
    statistic -- and ``accuracy_pvals`` / ``balanced_accuracy_pvals`` (k,), which compare them with the same functional
    of the observed data, ``scores_from_confusion(confusion.sum(-1))``, as ``(#{null >= observed} + 1) / (P + 1)``.  The
    comparison is ``>=``, not the strict ``>`` of ``pearson_r_pvals``: accuracy is discrete, exact ties have positive
    probability, and ``>`` would be anti-conservative.  Every statistic is a function of integer counts: the result does
    not depend on batch sizes, the scratch budget or the number of GPUs.

    Not offered: ``n_split`` (split-half reliability of indicator loadings answers no question), ``rotate``, ``aggfunc``
    and 3-D Y.  Bootstraps resample rows as ``pls_regression`` does (not stratified).

    ValueError, before any engine is created or looked up: a ``y`` that is not 1-D of length S; a NaN or None label;
    fewer than 2 or more than 32 classes (the bound of the device kernel k_sd_cv_class); a class with fewer than 2
    usable rows; ``auc=True`` without ``test_split``; a ``test_size`` that can leave a class without a usable training row; ``cvsamples`` whose training
    side lacks a usable row of some class; an unknown ``inner_select``, one given without ``inner_split``, ``inner_split`` without one; an inner
    fold whose training side lacks a usable row of some class (given folds as they are, drawn ones in the worst case);
    ``n_split``, ``aggfunc`` or ``rotate`` given; and everything ``pls_regression`` refuses."""
    for name in ('n_split', 'aggfunc', 'rotate'):
        if name in kwargs:
            raise ValueError('`pls_da` takes no `{}`: split-half reliability, aggregation of a 3-D Y and rotation are '
                             'not part of a discriminant analysis'.format(name))
    if auc and not (int(test_split or 0) > 0 and (test_size or 0) > 0):
        raise ValueError('`auc=True` needs a cross-validation: the AUC is counted over the test rows of `test_split` > 0 '
                         'splits (with `test_size` > 0)')
    if auc:
        kwargs = dict(kwargs, _auc=True)
    if inner_select is not None and inner_select not in INNER_SELECT:
        raise ValueError('Provided `inner_select` must be one of {}; got {!r}'.format(list(INNER_SELECT), inner_select))
    nested = isinstance(inner_split, (int, np.integer)) and not isinstance(inner_split, (bool, np.bool_)) \
        and inner_split > 0                            # (anything else: pls_regression's own message)
    if inner_select is not None and not nested:
        raise ValueError('`inner_select` needs `inner_split` > 0: it names the criterion the inner folds select by')
    if nested and inner_select is None:
        # (every call that was refused before the nested selection existed is refused still: the criterion is named)
        raise ValueError('`inner_split` is not available for pls_da without `inner_select`: name the criterion the inner '
                         'folds select by, one of {}'.format(list(INNER_SELECT)))
    if nested:
        kwargs = dict(kwargs, inner_select=inner_select)
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError('Expected 2D array for `X`, got {}D array instead'.format(X.ndim))
    S = len(X)
    classes, codes = encode_labels(y, S)
    G = len(classes)
    onehot = np.zeros((S, G), dtype=np.float64)
    onehot[np.arange(S), codes] = 1.0
    usable = _usable_rows(X, onehot)
    n_g = np.bincount(codes, minlength=G)
    ok_g = np.bincount(codes[usable], minlength=G)
    if ok_g.min() < 2:
        g = int(ok_g.argmin())
        raise ValueError('Every class needs at least 2 usable rows; class {!r} has {} ({} of its {} rows are NaN '
                         'throughout)'.format(_label(classes, g), int(ok_g[g]), int(n_g[g] - ok_g[g]), int(n_g[g])))
    n_cv = int(test_split or 0) if (test_size or 0) > 0 else 0
    if n_cv > 0 and 0 < test_size < 1:
        if cvsamples is not None:
            masks = np.asarray(cvsamples)
            if masks.ndim == 2 and masks.shape == (S, n_cv):           # (any other shape: pls_regression's own message)
                tr = masks.astype(bool) & usable[:, None]
                per = np.stack([tr[codes == g].sum(axis=0) for g in range(G)])      # (G, n) usable training rows
                if per.min() < 1:
                    g, s = np.unravel_index(int(per.argmin()), per.shape)
                    raise ValueError('Every cross-validation split needs a usable training row of every class; split {} '
                                     'of `cvsamples` has none of class {!r}'.format(int(s), _label(classes, g)))
        else:
            # the stratified draw keeps ceil or floor of n_g (1 - test_size) training rows of class g; whichever side
            # the masked rows of the class fall on, one usable training row must remain: the worst case is checked
            lo = np.floor(n_g * (1 - test_size)).astype(int) - (n_g - ok_g)
            if lo.min() < 1:
                g = int(lo.argmin())
                raise ValueError('Every cross-validation split needs a usable training row of every class; test_size = '
                                 '{} can leave class {!r} ({} rows, {} of them NaN throughout) without one'
                                 .format(test_size, _label(classes, g), int(n_g[g]), int(n_g[g] - ok_g[g])))
    if nested and n_cv > 0 and 0 < test_size < 1:
        bad_g = n_g - ok_g
        given = np.asarray(innersamples) if innersamples is not None else None
        masks = np.asarray(cvsamples) if cvsamples is not None else None
        if masks is not None and (masks.ndim != 2 or masks.shape != (S, n_cv)):
            masks = None                                             # (pls_regression's own message)
        if given is not None:
            if given.ndim == 3 and given.shape == (S, n_cv, int(inner_split)):   # (any other shape: pls_regression's message)
                tr = (given == 1) & usable[:, None, None]
                per = np.stack([tr[codes == g].sum(axis=0) for g in range(G)])  # (G, n, ni) usable training rows
                if per.min() < 1:
                    g, s, j = np.unravel_index(int(per.argmin()), per.shape)
                    raise ValueError('Every inner fold needs a usable training row of every class; inner fold {} of '
                                     'split {} of `innersamples` has none of class {!r}'
                                     .format(int(j), int(s), _label(classes, g)))
        else:
            # drawn, stratified: an inner fold keeps ceil or floor of m (1 - test_size) training rows of a class with m
            # rows on the outer training side, itself ceil or floor of n_g (1 - test_size) -- or what `cvsamples` leaves
            if masks is not None:
                m_lo = np.stack([masks.astype(bool)[codes == g].sum(axis=0) for g in range(G)]).min(axis=1)
            else:
                m_lo = np.floor(n_g * (1 - test_size)).astype(int)
            lo = np.floor(m_lo * (1 - test_size)).astype(int) - bad_g
            if lo.min() < 1:
                g = int(lo.argmin())
                raise ValueError('Every inner fold needs a usable training row of every class; test_size = {} can leave '
                                 'class {!r} ({} rows, {} of them NaN throughout) without one inside an outer training set'
                                 .format(test_size, _label(classes, g), int(n_g[g]), int(bad_g[g])))
    res = pls_regression(X, onehot, n_components=n_components, n_perm=n_perm, n_boot=n_boot, ci=ci,
                         permsamples=permsamples, bootsamples=bootsamples, seed=seed, verbose=verbose, n_proc=n_proc,
                         test_split=test_split, test_size=test_size, cvsamples=cvsamples, cv_perm=cv_perm,
                         cvpermsamples=cvpermsamples, coef_components=coef_components, coef_ci=coef_ci,
                         coef_perm=coef_perm, vip_components=vip_components, vip_perm=vip_perm, cv_predict=cv_predict,
                         inner_split=inner_split, innersamples=innersamples, _classes=codes, **kwargs)
    res['classes'] = classes
    return res


def roc_points(scores, positive):
    """The ROC curve of ``scores`` (n,) against ``positive`` (n,) bool -> ``(fpr, tpr, thresholds)``: one point per
    distinct score, taken in descending order -- rows with equal scores enter together, so a tie is one point -- after
    the starting point (0, 0) at threshold +inf.  ``tpr[i]`` / ``fpr[i]`` are the shares of the positive / negative rows
    with ``score >= thresholds[i]``; NaN where a side is empty.  NaN scores are dropped.  The trapezoid area under the
    points is the Mann-Whitney AUC with ties counted one half."""
    scores, positive = np.asarray(scores, dtype=np.float64), np.asarray(positive, dtype=bool)
    if scores.ndim != 1 or scores.shape != positive.shape:
        raise ValueError('Expected 1-D `scores` and `positive` of one length, got {} and {}'
                         .format(scores.shape, positive.shape))
    keep = ~np.isnan(scores)
    scores, positive = scores[keep], positive[keep]
    order = np.argsort(-scores, kind='stable')
    scores, positive = scores[order], positive[order]
    last = np.r_[np.flatnonzero(np.diff(scores) != 0), len(scores) - 1] if len(scores) else np.zeros(0, dtype=int)
    tp = np.r_[0, np.cumsum(positive)[last]].astype(np.float64)
    fp = np.r_[0, np.cumsum(~positive)[last]].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        tpr = tp / positive.sum() if positive.sum() else np.full(tp.shape, np.nan)
        fpr = fp / (~positive).sum() if (~positive).sum() else np.full(fp.shape, np.nan)
    return fpr, tpr, np.r_[np.inf, scores[last]]


def roc_curve(results, cls, split):
    """The one-vs-rest ROC curve of class ``cls`` (a label of ``results.classes``) on the test rows of cross-validation
    split ``split`` of a ``pls_da(..., cv_predict=...)`` result -> ``(fpr, tpr, thresholds)`` (:func:`roc_points`), from
    ``cvres.y_pred[:, g, split]`` and the true classes of the test rows.  Its trapezoid area is
    ``cvres.auc[g, y_pred_ncomp[split] - 1, split]``.  Works on a result read back by ``load_results`` too.
    ValueError for a result without ``classes`` or ``cvres.y_pred``, an unknown label, a split out of range."""
    classes = results.get('classes') if hasattr(results, 'get') else None
    cvres = results.get('cvres') if hasattr(results, 'get') else None
    if classes is None or cvres is None or cvres.get('y_pred') is None:
        raise ValueError('`results` holds no out-of-fold predictions: roc_curve needs a pls_da(..., cv_predict=...) result')
    classes, y_pred = np.asarray(classes), np.asarray(cvres['y_pred'])
    hit = np.flatnonzero(classes == cls)
    if len(hit) != 1:
        raise ValueError('`cls` = {!r} is not one of the classes {}'.format(cls, classes.tolist()))
    g = int(hit[0])
    if isinstance(split, (bool, np.bool_)) or int(split) != split or not 0 <= int(split) < y_pred.shape[2]:
        raise ValueError('`split` must be an integer in 0 .. {}; got {!r}'.format(y_pred.shape[2] - 1, split))
    codes = np.asarray(results['inputs']['_classes'] if results['inputs'].get('_classes') is not None
                       else np.argmax(np.asarray(results['inputs']['Y']), axis=1))
    v = y_pred[:, g, int(split)]
    test = ~np.isnan(v)
    return roc_points(v[test], codes[test] == g)


def predict_class(results, X_new, n_components=None):
    """The predicted class (S_new,) of new rows ``X_new`` (S_new, B) under a ``pls_da`` result:
    ``results.classes[np.argmax(predict(results, X_new, n_components), axis=1)]`` -- the first maximum of the predicted
    indicators.  Works on any ``pls_da`` result :func:`predict` works on, also one read back by ``load_results``;
    ``n_components`` as there.  ValueError for a result without ``classes``."""
    classes = results.get('classes') if hasattr(results, 'get') else None
    if classes is None:
        raise ValueError('`results` is not a pls_da result: it holds no `classes`')
    classes = np.asarray(classes)
    yhat = predict(results, X_new, n_components)
    if yhat.shape[1] != len(classes):
        raise ValueError('`results.classes` holds {} labels but the model predicts {} indicators'
                         .format(len(classes), yhat.shape[1]))
    return classes[np.argmax(yhat, axis=1)]
