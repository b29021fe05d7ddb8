"""
``pls_regression`` front-end (SIMPLS) with the reference's keyword surface
(pyls/types/regression.py:432-440) on the MI355X engine.

The per-resample SIMPLS fits run on the device in the S-dimensional dual
space (csrc/plsx_simpls.h); host code mirrors PLSRegression.run_pls
(regression.py:375-428).

Differences from the reference at this commit, on purpose:
  * ``n_perm > 0`` works.  In the reference ``PLSRegression._single_perm`` is
    called with keywords it does not accept (regression.py:329 vs
    base.py:646-648) and raises TypeError; the null statistic implemented here
    is what that method computes when driven directly (variance of the
    permuted Y explained per component, ``original=None`` branch, :369).
  * the caller's X is not centred in place (regression.py:395 mutates it).
  * the leading singular triplet per component is exact, the reference's
    rank-1 randomized SVD is approximate when Y has more than 11 columns
    (SURVEY.md section 0.3).
  * 3-D Y: the reference builds its (2, n_boot) resampling array with
    ``np.array(list(zip(s.T, c.T))).T`` (regression.py:216), which numpy >= 1.24
    rejects; here the equivalent object array is built explicitly.  The
    Rows (or, for 3-D Y, subjects) that are only partly NaN raise
    NotImplementedError (they poison the reference's fit as well).
  * ``test_split > 0`` cross-validates the prediction per component count (the reference forces ``test_split=0``:
    "not implemented for PLSRegression", regression.py:237-238).  Per split (behavioral.py:126-170 with simpls in
    place of the SVD): SIMPLS with ``n_components`` on the training rows, the test rows predicted by the first
    c = 1 .. n_components components plus the intercept, each prediction scored per behaviour
    (plsx_simpls_crossval_batch; csrc/plsx_simpls.h, k_sd_cv_score).
  * ``coef_components=c`` returns the fitted model of the first c components, ``Y ~ intercept + X @ coefs`` (simpls
    computes it as ``beta``, regression.py:149-151, and PLSResults drop it), and bootstraps the coefficients:
    ``bootres.coefs_stderr`` / ``coefs_normed``, one map per behaviour.  The coefficients depend on neither the signs
    nor the order of the components, so their bootstrap needs no alignment (plsx_simpls_coef_begin / _finish;
    csrc/plsx_simpls.h, k_sd_coef).  :func:`predict` applies the model of any ``pls_regression`` result to new rows.
    ``coef_ci=True`` adds ``bootres.coefs_ci``, the percentile interval of every coefficient over the bootstraps: the
    series keeps every bootstrap's coefficients in subject space and one closing pass over the features forms and
    reduces their series chunk by chunk (plsx_simpls_coef_keep / plsx_simpls_coef_ci; csrc/plsx_k_coefci.h).
  * ``cv_perm=P`` tests the cross-validated scores against chance: the whole cross-validation, the same splits, on
    ``(X, Y[perm])`` for P permutations; the (permutation, split) fits are formed, scored against the permuted Y and
    averaged over the splits in a fixed order on the device (plsx_simpls_crossval_perm_batch; csrc/plsx_simpls.h,
    k_sd_cvp_expand / k_sd_cv_score<RC, true> / k_sd_cvp_reduce).
  * ``vip_components=c`` returns the VIP scores (variable importance in projection, the formula of MATLAB's
    ``plsregress`` documentation) of the c-component model, one map per model, and bootstraps them:
    ``bootres.vip_stderr`` / ``vip_ci``.  VIP is a square root of a sum of squares over the components, so every
    bootstrap's scaled dual weights are kept in subject space and one closing pass over the features forms and reduces
    the series chunk by chunk (plsx_simpls_vip_keep / plsx_simpls_vip_ci; csrc/plsx_simpls.h, k_sd_vip;
    csrc/plsx_k_vip.h).  :func:`vip` computes the scores of any ``pls_regression`` result.  ``vip_perm=True`` tests
    them against permuted behaviour -- ``permres.vip_pvals`` / ``vip_max`` / ``vip_pvals_fwe`` --: the scores of every
    permutation's fit are formed tile by tile along the permutation batches, counted against the observed ones and
    reduced to their maxima over the features in registers (plsx_simpls_vip_perm_begin / _end; k_vip_perm_prod).
  * ``n_split=n`` runs the split-half reliability of the components (the reference forces ``n_split=0``: "not
    implemented for PLSRegression", regression.py:237-238): BasePLS.split_half (base.py:366-397, 704-770) with the
    x_weights and y_loadings of SIMPLS in place of the singular vectors, for the observed data and for every
    permutation, in dual space -- no pass over the features (plsx_simpls_split_half_batch; csrc/plsx_simpls.h,
    k_sd_sh_prep / k_sd_sh_expand / k_sd_sh_score).
  * ``_classes`` (build-only, set by :func:`pypyls_amd.discriminant.pls_da`): Y is the indicator matrix of these class
    codes; the splits are drawn stratified and the cross-validation also returns confusion counts
    (plsx_simpls_set_classes / plsx_simpls_cv_class_begin; csrc/plsx_simpls.h, k_sd_cv_class).
  * ``_auc`` (build-only, set by ``pls_da(auc=True)``; needs ``_classes``): the cross-validation also returns the
    one-vs-rest AUC counts of every class (plsx_simpls_cv_auc_begin; k_sd_cv_auc).
  * ``cv_predict``: the out-of-fold predictions of the observed cross-validated fits themselves, one slot per split
    written behind the scoring kernels (plsx_simpls_cv_pred_begin; csrc/plsx_simpls.h, k_sd_cv_pred).
"""
import warnings

import numpy as np

from . import hostmath, parallel, resampling
from .plsc import _host_array
from .structures import PLSInputs, PLSResults


def resid_yscores(x_scores, y_scores):
    """Residualise column c of y_scores against x_scores columns < c, two
    rounds of modified Gram-Schmidt (regression.py:9-45)."""
    x_scores = np.array(x_scores, dtype=float)
    y_scores = np.array(y_scores, dtype=float)
    for comp in range(x_scores.shape[1]):
        ui = y_scores[:, comp].copy()
        for _ in range(2):
            for j in range(comp):
                tj = x_scores[:, j]
                ui -= (tj @ ui) * tj
        y_scores[:, comp] = ui
    return y_scores


_AGGFUNCS = dict(mean=np.mean, median=np.median, sum=np.sum)


def _row_ok(A):
    """False for all-NaN rows (get_mask, regression.py:48-53); rows that are
    only partly NaN cannot be handled (they poison the reference as well)."""
    nan = np.isnan(A)
    allnan, anynan = nan.all(axis=1), nan.any(axis=1)
    if np.any(anynan & ~allnan):
        raise NotImplementedError(
            'rows with some (not all) NaN entries are not supported: the reference masks only rows that are NaN '
            'throughout (get_mask, pyls/types/regression.py:48-53) and lets a partly-NaN row poison the whole fit '
            '(NaN weights, :313, :324-325); impute or drop such rows before the call')
    return ~allnan


def _usable_rows(X, Y_agg):
    """get_mask (regression.py:48-53) without a pass over the whole of X: only rows whose first entry is NaN can be
    NaN throughout."""
    ok = ~np.isnan(Y_agg).all(axis=1)
    cand = np.flatnonzero(np.isnan(X[:, 0])) if X.shape[1] else np.zeros(0, dtype=int)
    if len(cand):
        ok[cand[np.isnan(X[cand]).all(axis=1)]] = False
    return ok


def _check_cvsplits(masks, usable, k, B):
    """masks (S, n) bool, True = training row; usable (S,) bool: every split needs two usable test rows (Pearson r)
    and enough usable training rows for k components."""
    n_tr = (masks & usable[:, None]).sum(axis=0)
    n_te = (~masks & usable[:, None]).sum(axis=0)
    if len(n_te) and n_te.min() < 2:
        raise ValueError('Every cross-validation split needs at least 2 usable test rows; split {} has {}'
                         .format(int(n_te.argmin()), int(n_te.min())))
    if len(n_tr) and k > min(int(n_tr.min()) - 1, B):
        raise ValueError('Provided `n_components` cannot be greater than {} when cross-validating: the smallest '
                         'training set has {} usable rows'.format(max(min(int(n_tr.min()) - 1, B), 0), int(n_tr.min())))


def _draw_inner_codes(cvmasks, inner_split, rs, test_size, classes=None):
    """The inner folds of a nested cross-validation, drawn from the generator ``rs``: for s = 0 .. n - 1
    ``gen_splits([n_tr_s], 1, inner_split, seed=rs, test_size=test_size)`` on the training rows of outer split s
    (``cvmasks`` (S, n) bool, True = training row) in ascending row order, scattered back -> (S, n, inner_split) uint8
    codes: 1 = inner training row, 0 = inner test row, 2 = on neither side (the outer test rows).  ``classes`` (S,) class
    codes (pls_da): the draw is stratified, ``gen_stratified_splits(classes[rows], inner_split, ...)`` at the same place."""
    cvmasks = np.asarray(cvmasks, dtype=bool)
    S, n = cvmasks.shape
    codes = np.full((S, n, int(inner_split)), 2, dtype=np.uint8)
    for s in range(n):
        rows = np.flatnonzero(cvmasks[:, s])
        if classes is not None:
            codes[rows, s, :] = resampling.gen_stratified_splits(np.asarray(classes)[rows], inner_split, seed=rs,
                                                                 test_size=test_size)
        else:
            codes[rows, s, :] = resampling.gen_splits([len(rows)], 1, inner_split, seed=rs, test_size=test_size)
    return codes


def nested_codes(cvmasks, innersamples):
    """(S, n, 1 + ni) uint8 codes of a nested cross-validation as the device takes them: ``[:, s, 0]`` outer split s
    (1 / 0), ``[:, s, 1:]`` its inner folds."""
    cvmasks = np.asarray(cvmasks, dtype=bool)
    return np.concatenate([cvmasks[:, :, None].astype(np.uint8), np.asarray(innersamples, dtype=np.uint8)], axis=2)


def _check_cv_predict(cv_predict, k, test_split, test_size, inner_split, da):
    """``cv_predict=`` of :func:`pls_regression` / ``pls_da`` -> None (not asked for), the component count 1 .. k of the
    returned predictions, or 0 for ``'nested'``: the count the nested selection chooses per outer split.  ValueError
    for anything else, without cross-validation, and for ``'nested'`` without ``inner_split``."""
    if cv_predict is None or (isinstance(cv_predict, (bool, np.bool_)) and not cv_predict):
        return None
    if isinstance(cv_predict, (bool, np.bool_)):
        c = int(k)
    elif isinstance(cv_predict, str) and cv_predict == 'nested':
        if da and not inner_split:
            raise ValueError("`cv_predict='nested'` is not available for pls_da without `inner_split` > 0 and "
                             '`inner_select`: the component count of every outer split is the one its inner folds choose')
        if not inner_split:
            raise ValueError("`cv_predict='nested'` needs `inner_split` > 0: the component count of every outer split "
                             'is the one its inner folds choose')
        c = 0
    elif isinstance(cv_predict, (int, np.integer)) and 1 <= int(cv_predict) <= int(k):
        c = int(cv_predict)
    else:
        raise ValueError("Provided `cv_predict` must be True, an integer in 1 .. n_components = {}{}; got {!r}"
                         .format(k, '' if da else " or 'nested'", cv_predict))
    if not (int(test_split or 0) > 0 and (test_size or 0) > 0):
        raise ValueError('`cv_predict` needs cross-validation: the predictions are those of the test rows of `test_split` '
                         '> 0 splits with `test_size` > 0; got test_split = {!r}, test_size = {!r}'
                         .format(test_split, test_size))
    return c


def pls_regression(X, Y, *, n_components=None, n_perm=5000, n_boot=5000, rotate=True, ci=95,
                   aggfunc='mean', permsamples=None, bootsamples=None, seed=None, verbose=True,
                   n_proc=None, test_split=0, test_size=0.25, cvsamples=None, coef_components=None, coef_ci=False,
                   cv_perm=0, cvpermsamples=None, vip_components=None, coef_perm=False, n_split=0, confounds=None,
                   vip_perm=False, inner_split=0, innersamples=None, cv_predict=False, **kwargs):
    """PLS regression of Y (S, T) or (S, T, C) on X (S, B) with SIMPLS; see
    pyls.pls_regression.  ``n_proc``: GPUs of this node to shard the resamples over (one process, team.py);
    ``device_ids=[...]`` names them.

    Missing data: rows of X or Y that are NaN THROUGHOUT are masked like the reference's ``get_mask`` masks them
    (pyls/types/regression.py:48-53).  A row that is only PARTLY NaN raises NotImplementedError here; in the
    reference it is not masked and turns the weights of the whole fit into NaN (regression.py:313, 324-325) --
    a behavioural difference of this drop-in, on purpose: impute or drop such rows first.

    Cross-validation: ``test_split`` train / test splits (0, the default, or ``test_size=0``: none), drawn with
    ``gen_splits([S], 1, test_split, test_size=test_size)`` after everything else the call draws, or given as
    ``cvsamples`` (S, test_split) bool, True = training row.  ``cvres`` then holds ``pearson_r`` / ``r_squared``
    (T, test_split) of the full model, ``pearson_r_ncomp`` / ``r_squared_ncomp`` (T, n_components, test_split) of the
    nested models, ``mse`` (n_components + 1, test_split) -- row 0 the intercept-only model -- and ``cvsamples``.
    Masked rows belong to neither side.

    Model coefficients: ``coef_components=c`` (1 <= c <= n_components; None, the default: nothing is added) returns
    ``coefs`` (B, T) ``= x_weights[:, :c] @ y_loadings[:, :c].T`` (with masked rows: simpls' own y_loadings, centred
    over the rows of the fit) and ``intercept`` (T,) of the c-component model
    ``Y ~ intercept + X @ coefs`` (means over the rows the fit used; 3-D Y: of the aggregated Y) and, with
    ``n_boot > 0``, ``bootres.coefs_stderr`` / ``bootres.coefs_normed`` (B, T): the standard error of the coefficients
    over the bootstraps and the coefficients over it, with the original added back (n = n_boot + 1) as for
    ``x_weights_normed``.  No random draw is added or moved.  :func:`predict` applies the model to new rows.

    ``coef_ci=True`` (needs ``coef_components`` and ``n_boot > 0``; False, the default: nothing is added and no memory
    is taken) adds ``bootres.coefs_ci`` (B, T, 2), ``[..., 0]`` the lower and ``[..., 1]`` the upper bound of the
    ``ci`` % percentile interval of every coefficient over the ``n_boot`` bootstraps (numpy's linear interpolation;
    as for ``y_loadings_ci`` the original fit is not added to the series).  The (B, T, n_boot) coefficients exist on the
    device only, one chunk of features at a time; what is kept is 8 T S n_boot bytes (on every GPU of a team: the
    closing pass runs on the first).  ``n_boot`` <= 16384.  Every other array of the call keeps its bits.

    ``coef_perm=True`` (needs ``coef_components`` and ``n_perm > 0``; False, the default: nothing is added) tests the
    coefficients against permuted behaviour.  The c-component model is fitted on ``(X, Y[perm_p])`` for the SAME
    permutations as ``permres.permsamples`` (3-D Y: the aggregated Y is permuted; rows that are NaN throughout: position
    p is usable iff row p of X and row perm[p] of Y are), giving coefficients ``b_p`` (B, T) that exist on the device
    only, one tile at a time.  ``permres`` gains ``coefs_pvals`` (B, T), the uncorrected two-sided p-value
    ``(#{p : |b_p[f, t]| >= |coefs[f, t]|} + 1) / (n_perm + 1)``; ``coefs_max`` (T, n_perm), the null of the single-step
    max statistic per behaviour, ``max_f s_f |b_p[f, t]|`` with ``s_f`` the standard deviation of feature f over the
    usable rows of X (so the maximum runs over standardised coefficients); and ``coefs_pvals_fwe`` (B, T) =
    ``(#{p : coefs_max[t, p] >= s_f |coefs[f, t]|} + 1) / (n_perm + 1)``, the maxT p-value of Westfall & Young,
    family-wise over the features of one behaviour (for a family that spans the behaviours too, compare against
    ``coefs_max.max(axis=0)``).  The comparison is ``>=``, not the strict ``>`` of ``permres.pvals``: a feature without
    variance has ``coefs = b_p = 0`` exactly and comes out at p = 1, not 1 / (n_perm + 1); everywhere else an exact
    tie has probability zero.  Every other array of the call keeps its bits.

    Permutation test of the cross-validation: ``cv_perm=P`` (needs cross-validation; 0, the default: nothing is added,
    no memory is taken) repeats the whole cross-validation -- the SAME splits -- on ``(X, Y[perm])`` for P permutations
    of the rows of Y (3-D Y: of the aggregated Y), drawn with ``gen_permsamp([S], 1, P)`` after everything else the call
    draws, the split masks included, or given as ``cvpermsamples`` (S, P), one permutation of 0 .. S-1 per column.  The
    null statistic of a permutation is the plain mean over the splits.  ``cvres`` gains ``perm_pearson_r`` /
    ``perm_r_squared`` (T, n_components, P), ``perm_mse`` (n_components + 1, P), ``pearson_r_pvals`` /
    ``r_squared_pvals`` (T, n_components) = (#{null > observed split-mean} + 1) / (P + 1), ``mse_pvals``
    (n_components + 1,) = (#{null < observed} + 1) / (P + 1) -- smaller is better -- and ``cvpermsamples``.  With rows
    that are NaN throughout, position p is usable under a permutation iff row p of X and row perm[p] of Y are; a
    (permutation, split) pair with fewer than two usable test rows gives NaN.  The P x test_split fits run and are
    reduced over the splits on the device (plsx_simpls_crossval_perm_batch); only P rows come back.  Every array the
    call returned before keeps its bits.

    Nested cross-validation of ``n_components``: ``inner_split=ni`` (needs cross-validation; 0, the default: nothing is
    added, nothing is drawn, every array keeps its bits).  Reading ``cvres.mse``, picking the best c and quoting
    ``pearson_r_ncomp[:, c - 1]`` selects and scores on the same test rows.  Here ni inner splits INSIDE the training
    rows of every outer split choose c, and the outer test rows, which took no part in the choice, score the chosen
    model.  The inner folds are codes ``innersamples`` (S, test_split, ni) uint8 -- 1 = training row, 0 = test row, 2 =
    on neither side, which is exactly the outer test rows of that split -- given (then ``cvsamples`` must be given too)
    or drawn: one more job at the END of the draw list, for s = 0 .. test_split - 1
    ``gen_splits([n_tr_s], 1, ni, test_size=test_size)`` on the training rows of split s in ascending row order,
    scattered back.  Per outer split s: ``inner_mse[c, s]``, c = 0 .. k, the mean over the inner folds of the fold's
    squared error per usable test row (row 0 the intercept-only model); ``nested_ncomp[s]`` its first minimum over
    c = 1 .. k (a NaN is never smaller; 0 and NaN scores where that minimum is not finite); and ``nested_pearson_r`` /
    ``nested_r_squared`` (T, test_split), ``nested_mse`` (test_split,): the outer fit's ``pearson_r_ncomp`` /
    ``r_squared_ncomp`` / ``mse`` at c = ``nested_ncomp[s]``.  With ``cv_perm=P`` the WHOLE procedure, selection
    included, is repeated under the same ``cvpermsamples``: ``perm_nested_pearson_r`` / ``perm_nested_r_squared`` (T, P)
    and ``perm_nested_mse`` (P,), the plain means over the outer splits, each split at the c selected inside that
    permutation; ``perm_nested_ncomp`` (k, P) int, how many outer splits of a permutation chose c; and
    ``nested_pearson_r_pvals`` / ``nested_r_squared_pvals`` (T,) = (#{null > observed split-mean} + 1) / (P + 1),
    ``nested_mse_pvals`` with ``<`` (a NaN null value counts as not larger / not smaller).  That is
    P x test_split x (1 + ni) fits, selected and reduced on the device (plsx_simpls_crossval_nested_batch,
    plsx_simpls_crossval_nested_perm_batch); ranks and teams shard the permutations.  Refused: ``confounds``.
    (``pls_da`` selects on its counts instead: ``inner_select`` there.)

    Out-of-fold predictions: ``cv_predict`` (needs cross-validation; False, the default: nothing is added, nothing is
    drawn differently, every array keeps its bits) returns the predicted value of every held-out row, which the scores
    above are reductions of: ``True`` for the full model, the one ``cvres.pearson_r`` scores; an int c,
    1 <= c <= n_components, for the c-component model; ``'nested'`` (needs ``inner_split``) for the model of
    ``nested_ncomp[s]`` components per outer split s.  ``cvres`` gains ``y_pred`` (S, T, test_split): for a usable test
    row i of split s ``[1, x_i] @ simpls(X_tr, Y_tr, c)['beta']``, in the units of the Y of the call (3-D Y: of the
    aggregated Y) -- the scale :func:`predict` answers in --, NaN on training rows and on rows that are NaN throughout;
    and ``y_pred_ncomp`` (test_split,) int32, the c of every split.  With ``confounds`` ``y_pred`` predicts the
    fold-residualised test Y from the fold-residualised test X, and ``cvres.y_true`` (S, T, test_split) holds that Y,
    which exists on the device only (NaN off the test rows).  Under ``cv_perm`` only the observed fits are returned.
    One c per call, no predictions of inner folds.  The stack is 8 S T test_split bytes on the device (twice that with
    ``confounds``) and rides in the call's one collective.  A K-fold partition is passed as ``cvsamples``.

    VIP scores: ``vip_components=c`` (1 <= c <= n_components, independent of ``coef_components``; None, the default:
    nothing is added, no memory is taken) returns ``vip`` (B,), the variable importance in projection of the
    c-component model, ``sqrt(B * sum_a ssq_a * x_weights[f, a]**2 / |x_weights[:, a]|**2 / sum_a ssq_a)`` with
    ``ssq_a = |y_loadings[:, a]|**2`` of simpls (:func:`vip`); ``sum(vip**2) == B``.  With ``n_boot > 0`` also
    ``bootres.vip_stderr`` (B,), ``np.std(..., ddof=1)`` of the VIP scores of the ``n_boot`` bootstrap fits (NaN for
    ``n_boot = 1``), and ``bootres.vip_ci`` (B, 2), their ``ci`` % percentile interval (numpy's linear interpolation);
    as for ``coefs_ci`` the original fit is not part of the series.  VIP depends on neither the signs nor the order of
    the components: no alignment.  The (B, n_boot) scores exist on the device only, one chunk of features at a time;
    what is kept is 8 c S n_boot bytes (on every GPU of a team: the closing pass runs on the first).
    ``n_boot`` <= 16384.  Every other array of the call keeps its bits.

    ``vip_perm=True`` (needs ``vip_components`` and ``n_perm > 0``; False, the default: nothing is added) tests the VIP
    scores against permuted behaviour, where the usual "VIP > 1" cut-off flags about the same share of features on pure
    noise as on real signal (``sum(vip**2) == B`` either way).  The c-component model is fitted on ``(X, Y[perm_p])``
    for the SAME permutations as ``permres.permsamples`` -- the fits of ``coef_perm`` (3-D Y: the aggregated Y is
    permuted; rows that are NaN throughout: position p is usable iff row p of X and row perm[p] of Y are; with
    ``confounds`` the rows of Y_r are permuted against X_r) --, giving scores ``vip_p`` (B,) by the formula above that
    exist on the device only, one tile at a time.  ``permres`` gains ``vip_pvals`` (B,), the uncorrected one-sided
    p-value ``(#{p : vip_p[f] >= vip[f]} + 1) / (n_perm + 1)`` (VIP is non-negative and large means important);
    ``vip_max`` (n_perm,) ``= max_f vip_p[f]``, the null of the single-step max statistic (VIP is already comparable
    across features: no feature scale enters); and ``vip_pvals_fwe`` (B,) ``= (#{p : vip_max[p] >= vip[f]} + 1) /
    (n_perm + 1)``, the maxT p-value of Westfall & Young, family-wise over the features.  The comparison is ``>=``: a
    feature without variance has VIP 0 under every arrangement and comes out at p = 1.  A degenerate permuted fit (the
    formula's 0 / 0) counts nowhere and has ``vip_max = NaN``; where ``vip[f]`` is NaN both p-values are NaN.
    Independent of ``coef_components`` and ``coef_perm``.  Every other array of the call keeps its bits.

    Split-half reliability: ``n_split=n`` (0 or None, the default: nothing is added, nothing is drawn) asks whether the
    components replicate between two halves of the cohort, as ``behavioral_pls(n_split=n)`` does (BasePLS.split_half,
    pyls/base.py:366-397, with SIMPLS in place of the SVD).  The k-component fit on all usable rows of an arrangement
    ``(X, Y[perm])`` gives W = x_weights (B, k) and Q = simpls' y_loadings (T, k); each of n random halvings (``gen_splits``
    with ``test_size=0.5``) gives ``D_h = (Y_h - ybar_h).T @ (X_h - xbar_h)`` per half, and
    ``ucorr[c] = efficient_corr(D_1.T @ Q, D_2.T @ Q)[c]`` over the features, ``vcorr[c] = efficient_corr(D_1 @ W,
    D_2 @ W)[c]`` over the behaviours, averaged over the n splits.  ``splitres`` holds the reference's keys with k
    components: ``ucorr`` / ``vcorr`` (k,) of the observed data, ``ucorr_pvals`` / ``vcorr_pvals`` against the same
    statistic of the ``n_perm`` permutations of ``permres.permsamples`` (permutation i halves with the masks of a fresh
    ``RandomState(i)``), and ``*_lolim`` / ``*_uplim``, the ``ci`` % interval of the permuted means.  With ``n_perm = 0``
    only ``ucorr`` and ``vcorr`` are filled (the reference fills nothing then).  3-D Y: the aggregated Y is split.  Rows
    that are NaN throughout belong to neither half (under a permutation: position p is usable iff row p of X and row
    perm[p] of Y are); every half must keep at least 2 usable rows.  With one behaviour (T = 1) ``vcorr`` is NaN, as
    numpy's correlation of single values is.  The observed data's masks are drawn after everything else the call
    draws: every other array of the call keeps its bits.  Per split the device forms two S-long vectors per component
    and multiplies them with K = Xc Xc^T: 4 S^2 k flop, nothing B-sized (plsx_simpls_split_half_batch).

    Confounds: ``confounds=Z`` (S, q) or (S,), 1 <= q <= 15 (None, the default: nothing is added, nothing is drawn
    differently, every array keeps its bits) adjusts the analysis for nuisance variables.  A row is usable iff it is
    usable in X and in Y and Z is not NaN throughout there (a row unusable on either side is unusable on both; a row of Z
    that is non-finite only in part raises).  X and Y are residualised on ``[1, Z]`` over the usable rows, once, on the
    device (plsx_simpls_set_confounds), and the observed fit, ``n_perm``, ``n_boot``, ``n_split``, ``coef_components``,
    ``coef_ci`` and ``vip_components`` run on the residuals (X_r, Y_r): permutations permute rows of Y_r, bootstraps
    resample residual rows -- the confound regression is NOT refitted per bootstrap, a limit of this version -- and a
    seeded call draws what the call without the keyword draws.  The result gains ``confound_mean`` (q,) = zbar and
    ``confound_x`` (q, B) / ``confound_y`` (q, T), the slopes of X and Y on Z - zbar; ``intercept`` stays in the units
    of the raw data (:func:`predict` takes ``confounds=Z_new``).  With ``test_split > 0`` the confound regression is
    fitted on the TRAINING rows of every split and applied to all its rows (cross-validated confound regression, Snoek
    et al. 2019, NeuroImage 184: residuals taken over the whole cohort would leak the test rows into the training
    data): ``cvres`` keeps its keys and shapes, the scores are those of the fold-residualised test Y against its
    prediction from the fold-residualised test X (plsx_simpls_crossval_confound_batch: a rank-2 (q + 1) update of K per
    split, nothing B-sized).  ``cv_perm=P`` permutes the residualised Y and residualises it again per fold, which is
    what Freedman & Lane's arrangement reduces to under the fold's own regression
    (plsx_simpls_crossval_confound_perm_batch).  Refused: Z of the wrong shape, q > 15, Z rank deficient together with
    the intercept on the usable rows or on the training rows of a split, 3-D Y, ``coef_perm=True``, ``cv_perm`` with
    masked rows, and ``pls_da``."""
    from .engine import Engine
    X, Y = np.asarray(X), np.asarray(Y)
    if X.ndim != 2:
        raise ValueError('Expected 2D array for `X`, got {}D array instead'.format(X.ndim))
    max_components = min(len(X) - 1, X.shape[1])
    if n_components is None:
        n_components = max_components
    else:
        n_components = int(n_components)
        if n_components > max_components:
            raise ValueError('Provided `n_components` cannot be greater than {}'
                             .format(max_components))
    if Y.ndim not in (2, 3) or len(X) != len(Y):
        raise ValueError('Provided `X` and `Y` matrices must have the same number of samples. '
                         'Provided matrices differed: X: {}, Y: {}'.format(len(X), len(Y)))
    if coef_components is not None:                # (validated on the host before any engine is created or looked up)
        if isinstance(coef_components, bool) or int(coef_components) != coef_components \
                or not 1 <= int(coef_components) <= n_components:
            raise ValueError('Provided `coef_components` must be an integer in 1 .. n_components = {}; got {!r}'
                             .format(n_components, coef_components))
        coef_components = int(coef_components)
        kwargs['coef_components'] = coef_components        # (recorded in `inputs` only when asked for)
    if isinstance(coef_ci, (bool, np.bool_)):
        coef_ci = bool(coef_ci)
    else:
        raise ValueError('Provided `coef_ci` must be True or False; got {!r}'.format(coef_ci))
    if coef_ci:                                    # (as above: on the host, before any engine)
        if coef_components is None:
            raise ValueError('`coef_ci` needs `coef_components`: the intervals are those of the coefficients of the '
                             'model of that many components')
        if not n_boot or n_boot < 1:
            raise ValueError('`coef_ci` needs bootstraps: n_boot = {!r}'.format(n_boot))
        if n_boot > 16384:
            raise ValueError('`coef_ci` takes n_boot <= 16384, the bound of the device\'s percentile kernels; got {}.  '
                             'There is no host fallback: the (B, T, n_boot) coefficients ({:.1f} GB here) exist on the '
                             'device only, one chunk of features at a time'
                             .format(n_boot, 8.0 * X.shape[1] * Y.shape[1] * n_boot / 2 ** 30))
        kwargs['coef_ci'] = True                   # (recorded in `inputs` only when asked for)
    if isinstance(coef_perm, (bool, np.bool_)):
        coef_perm = bool(coef_perm)
    else:
        raise ValueError('Provided `coef_perm` must be True or False; got {!r}'.format(coef_perm))
    if coef_perm:                                  # (as above: on the host, before any engine)
        if coef_components is None:
            raise ValueError('`coef_perm` needs `coef_components`: the p-values are those of the coefficients of the '
                             'model of that many components')
        if not n_perm or n_perm < 1:
            raise ValueError('`coef_perm` needs permutations: n_perm = {!r}'.format(n_perm))
        kwargs['coef_perm'] = True                 # (recorded in `inputs` only when asked for)
    if vip_components is not None:                 # (as above: on the host, before any engine)
        if isinstance(vip_components, bool) or int(vip_components) != vip_components \
                or not 1 <= int(vip_components) <= n_components:
            raise ValueError('Provided `vip_components` must be an integer in 1 .. n_components = {}; got {!r}'
                             .format(n_components, vip_components))
        vip_components = int(vip_components)
        if n_boot and n_boot > 16384:
            raise ValueError('`vip_components` takes n_boot <= 16384, the bound of the device\'s percentile kernels; got '
                             '{}.  There is no host fallback: the (B, n_boot) VIP scores ({:.1f} GB here) exist on the '
                             'device only, one chunk of features at a time'
                             .format(n_boot, 8.0 * X.shape[1] * n_boot / 2 ** 30))
        kwargs['vip_components'] = vip_components          # (recorded in `inputs` only when asked for)
    if isinstance(vip_perm, (bool, np.bool_)):
        vip_perm = bool(vip_perm)
    else:
        raise ValueError('Provided `vip_perm` must be True or False; got {!r}'.format(vip_perm))
    if vip_perm:                                   # (as above: on the host, before any engine)
        if vip_components is None:
            raise ValueError('`vip_perm` needs `vip_components`: the p-values are those of the VIP scores of the model '
                             'of that many components')
        if not n_perm or n_perm < 1:
            raise ValueError('`vip_perm` needs permutations: n_perm = {!r}'.format(n_perm))
        kwargs['vip_perm'] = True                  # (recorded in `inputs` only when asked for)
    if isinstance(cv_perm, (bool, np.bool_)) or not isinstance(cv_perm, (int, np.integer)) or cv_perm < 0:
        raise ValueError('Provided `cv_perm` must be a non-negative integer; got {!r}'.format(cv_perm))
    cv_perm = int(cv_perm)
    if cv_perm > 0:                                # (as above: on the host, before any engine)
        if not (int(test_split or 0) > 0 and (test_size or 0) > 0):
            raise ValueError('`cv_perm` needs cross-validation: it permutes Y under the splits of `test_split` > 0 with '
                             '`test_size` > 0 (drawn, or given as `cvsamples`); got test_split = {!r}, test_size = {!r}'
                             .format(test_split, test_size))
        kwargs['cv_perm'] = cv_perm                # (recorded in `inputs` only when asked for)
    if isinstance(inner_split, (bool, np.bool_)) or not isinstance(inner_split, (int, np.integer)) or inner_split < 0:
        raise ValueError('Provided `inner_split` must be a non-negative integer; got {!r}'.format(inner_split))
    inner_split = int(inner_split)
    if inner_split == 0 and innersamples is not None:
        raise ValueError('`innersamples` needs `inner_split` > 0, the number of inner folds it holds per outer split')
    if inner_split > 0:                            # (as above: on the host, before any engine)
        if not (int(test_split or 0) > 0 and (test_size or 0) > 0):
            raise ValueError('`inner_split` needs cross-validation: the inner folds lie inside the training rows of the '
                             'splits of `test_split` > 0 with `test_size` > 0; got test_split = {!r}, test_size = {!r}'
                             .format(test_split, test_size))
        if kwargs.get('_classes') is not None and kwargs.get('inner_select') is None:
            raise ValueError('`inner_split` is not available for pls_da without `inner_select`: its confusion and AUC '
                             'counts are selected by the criterion that keyword names')
        if confounds is not None:
            raise ValueError('`inner_split` cannot be combined with `confounds`: the fold-wise confound regression has '
                             'its own K per split (not in this version)')
        kwargs['inner_split'] = inner_split        # (recorded in `inputs` only when asked for)
    cvpred = _check_cv_predict(cv_predict, n_components, test_split, test_size, inner_split,
                               kwargs.get('_classes') is not None)
    if cvpred is not None:                         # (as above: on the host, before any engine)
        kwargs['cv_predict'] = cv_predict if isinstance(cv_predict, str) else \
            (True if isinstance(cv_predict, (bool, np.bool_)) else int(cv_predict))   # (recorded only when asked for)
    if n_split is None:
        n_split = 0
    if isinstance(n_split, (bool, np.bool_)) or not isinstance(n_split, (int, np.integer)) or n_split < 0:
        raise ValueError('Provided `n_split` must be a non-negative integer; got {!r}'.format(n_split))
    n_split = int(n_split)
    S = len(X)
    agg = None
    third = None                                   # (C, n_boot) third-axis resamples for 3-D Y
    bootsamples_out = None
    seed = parallel.shared_seed(seed)              # all ranks draw the same index arrays
    device_ids = kwargs.pop('device_ids', None)
    transport = kwargs.pop('_transport', 'auto')
    if Y.ndim == 3:
        # regression.py:208-235
        if not callable(aggfunc) and aggfunc not in _AGGFUNCS:
            raise ValueError('Provided `aggfunc` must either be callable or one of {}'
                             .format(sorted(_AGGFUNCS)))
        agg = _AGGFUNCS.get(aggfunc, aggfunc)
        C = Y.shape[-1]
        if n_boot > 0:
            if bootsamples is None:
                # both draws restart from `seed`, as the reference's do (:212-215)
                subj = resampling.gen_bootsamp([S], 1, n_boot, seed=seed, verbose=verbose)
                third = resampling.gen_bootsamp([C], 1, n_boot, seed=seed, verbose=verbose)
            else:
                bs = np.asarray(bootsamples, dtype=object) if not isinstance(bootsamples, np.ndarray) \
                    else bootsamples
                ok = bs.shape[0] == 2 and bs.shape[-1] == n_boot
                if ok:
                    subj = np.stack([np.asarray(bs[0][i]) for i in range(n_boot)], axis=-1)
                    third = np.stack([np.asarray(bs[1][i]) for i in range(n_boot)], axis=-1)
                    ok = subj.shape[0] == S and third.shape[0] == C
                if not ok:
                    raise ValueError('Provided bootsamples arrays does not match size of provided '
                                     'input arrays or number of bootstraps requested via `nboot`.')
            packed = np.empty((2, n_boot), dtype=object)
            for i in range(n_boot):
                packed[0, i], packed[1, i] = subj[:, i], third[:, i]
            bootsamples_out, bootsamples = packed, subj
        try:
            Y_agg = agg(Y, axis=-1)
        except TypeError:
            raise TypeError('Provided callable `aggfun` must accept `axis` keyword argument to '
                            'condense an array along the specified axis.')
        if np.isnan(Y).any():
            # a subject is either complete or missing altogether: a value missing in SOME
            # slices would make the aggregated row depend on the resampled third axis
            sub_nan = np.isnan(Y).reshape(S, -1)
            if np.any(sub_nan.any(axis=1) & ~sub_nan.all(axis=1)):
                raise NotImplementedError('3-D Y with partly missing subjects is not supported')
    else:
        Y_agg = Y
        bootsamples_out = None
    # ---- confounds: validated on the host before any engine is created or looked up
    cf = None
    if confounds is not None:
        if kwargs.get('_classes') is not None:
            raise ValueError('`confounds` is not supported by pls_da: residualised class indicators are no classes')
        if Y.ndim == 3:
            raise ValueError('`confounds` needs a 2-D Y: a 3-D Y is aggregated anew for every bootstrap, after which its '
                             'residuals would have to be taken again')
        if coef_perm:
            raise ValueError('`confounds` cannot be combined with `coef_perm=True`: its feature scale is that of the '
                             'raw X')
        Zc = np.asarray(confounds)
        if Zc.ndim == 1:
            Zc = Zc[:, None]
        if Zc.ndim != 2 or len(Zc) != S or Zc.shape[1] < 1 or not (np.issubdtype(Zc.dtype, np.number)
                                                                   or Zc.dtype == bool):
            raise ValueError('Provided `confounds` must be numeric with shape (S, q) or (S,), S = {}; got {}'
                             .format(S, np.shape(confounds)))
        if Zc.shape[1] > 15:
            raise ValueError('Provided `confounds` can have at most 15 columns; got {}'.format(Zc.shape[1]))
        Zc = Zc.astype(np.float64)
        zok = ~np.isnan(Zc).all(axis=1)
        usable = _usable_rows(X, Y_agg) & zok
        if not np.isfinite(Zc[usable]).all():
            raise ValueError('Provided `confounds` must be finite on every usable row (a row that is NaN throughout is '
                             'masked like such a row of X or Y); row {} is not'
                             .format(int(np.flatnonzero(usable & ~np.isfinite(Zc).all(axis=1))[0])))
        if cv_perm > 0 and not usable.all():
            raise ValueError('`confounds` with `cv_perm` needs complete data: {} rows of X, Y or the confounds are NaN '
                             'throughout'.format(int((~usable).sum())))
        zmean = Zc[usable].mean(axis=0)
        Zt = np.c_[np.ones(S), np.where(usable[:, None], Zc - zmean, 0.0)]
        if np.linalg.matrix_rank(Zt[usable]) < Zt.shape[1]:
            raise ValueError('Provided `confounds` are rank deficient together with the intercept on the {} usable rows'
                             .format(int(usable.sum())))
        cf = dict(Z=np.where(usable[:, None], Zc, 0.0), Zt=Zt, usable=usable, zmean=zmean)
        kwargs['confounds'] = Zc                       # (recorded in `inputs` only when given)
    kwargs.update(n_split=n_split)                 # (the reference forces 0, regression.py:238; so does test_split there)
    kwargs.setdefault('permindices', True)
    test_split = int(test_split or 0)
    inputs = PLSInputs(X=X, Y=Y, groups=[S], n_cond=1, n_components=n_components, n_perm=n_perm,
                       n_boot=n_boot, rotate=rotate, ci=ci, aggfunc=aggfunc,
                       permsamples=permsamples, bootsamples=bootsamples_out if Y.ndim == 3 else bootsamples,
                       seed=seed, verbose=verbose, n_proc=n_proc, test_split=test_split, test_size=test_size,
                       **kwargs)
    # ---- cross-validation: validated on the host before any engine is created or looked up
    n_cv = test_split if (test_size or 0) > 0 else 0
    cvmasks = None
    if n_cv > 0:
        if cvsamples is not None:
            cvmasks = np.asarray(cvsamples)
            if cvmasks.ndim != 2 or cvmasks.shape != (S, n_cv):
                raise ValueError('Provided `cvsamples` must have shape (S, test_split) = ({}, {}); got {}'
                                 .format(S, n_cv, cvmasks.shape))
            cvmasks = cvmasks.astype(bool)
            _check_cvsplits(cvmasks, _usable_rows(X, Y_agg) if cf is None else cf['usable'], n_components, X.shape[1])
            if cf is not None:
                _check_cvrank(cf, cvmasks)
        else:
            # gen_splits keeps ceil or floor of S (1 - test_size) training rows.  Whichever side the masked (all-NaN)
            # rows fall on, every split it can draw must pass: the worst case is checked, so nothing is left to
            # check once the masks exist
            n_bad = int((~(_usable_rows(X, Y_agg) if cf is None else cf['usable'])).sum())
            lo_tr = int(np.floor(S * (1 - test_size))) - n_bad
            lo_te = S - int(np.ceil(S * (1 - test_size))) - n_bad
            if kwargs.get('_classes') is not None:
                # (pls_da: the draw is stratified, every class keeps ceil or floor of ITS n_g (1 - test_size) rows)
                n_g = np.bincount(np.asarray(kwargs['_classes']))
                lo_tr = int(np.floor(n_g * (1 - test_size)).sum()) - n_bad
                lo_te = S - int(np.ceil(n_g * (1 - test_size)).sum()) - n_bad
            if lo_te < 2:
                raise ValueError('Every cross-validation split needs at least 2 usable test rows; test_size = {} can '
                                 'leave {} of {} ({} rows are NaN throughout)'.format(test_size, max(lo_te, 0), S, n_bad))
            if n_components > min(lo_tr - 1, X.shape[1]):
                raise ValueError('Provided `n_components` cannot be greater than {} when cross-validating: the '
                                 'smallest training set has {} usable rows'
                                 .format(max(min(lo_tr - 1, X.shape[1]), 0), max(lo_tr, 0)))
    cvperm = None
    if cv_perm > 0:
        if cvpermsamples is not None:
            from .engine import check_index_array as _check_idx
            cvperm = np.asarray(cvpermsamples)
            if cvperm.ndim != 2 or cvperm.shape != (S, cv_perm):
                raise ValueError('Provided `cvpermsamples` must have shape (S, cv_perm) = ({}, {}); got {}'
                                 .format(S, cv_perm, cvperm.shape))
            cvperm = _check_idx(cvperm, S)
            if not np.array_equal(np.sort(cvperm, axis=0), np.broadcast_to(np.arange(S)[:, None], cvperm.shape)):
                bad = int(np.flatnonzero((np.sort(cvperm, axis=0) != np.arange(S)[:, None]).any(axis=0))[0])
                raise ValueError('Provided `cvpermsamples` must hold one permutation of 0 .. {} per column; column {} '
                                 'is not one'.format(S - 1, bad))
        # rows that are NaN throughout: position p is usable iff row p of X and row perm[p] of Y are, so a permutation
        # can leave every masked row of X and of Y on the training side of one split
        ok_y = ~np.isnan(Y_agg).all(axis=1)
        n_bad_p = int((~_usable_rows(X, np.zeros((S, 1)))).sum()) + int((~ok_y).sum())
        lo_tr = (int(cvmasks.sum(axis=0).min()) if cvmasks is not None else int(np.floor(S * (1 - test_size)))) - n_bad_p
        if n_bad_p and n_components > min(lo_tr - 1, X.shape[1]):
            raise ValueError('Provided `n_components` cannot be greater than {} when permuting the cross-validation: '
                             'a permutation can leave {} usable training rows'
                             .format(max(min(lo_tr - 1, X.shape[1]), 0), max(lo_tr, 0)))
    # ---- nested cross-validation: validated on the host before any engine is created or looked up
    inner = None
    if inner_split > 0:
        usable = _usable_rows(X, Y_agg)
        n_bad = int((~usable).sum())
        # (under cv_perm a permutation can leave every masked row of X and of Y on the training side of one fold: the
        # worst-case rule of `cv_perm` above)
        n_bad_tr = n_bad if cv_perm == 0 else \
            int((~_usable_rows(X, np.zeros((S, 1)))).sum()) + int(np.isnan(Y_agg).all(axis=1).sum())
        if innersamples is not None:
            inner = np.asarray(innersamples)
            if inner.ndim != 3 or inner.shape != (S, n_cv, inner_split):
                raise ValueError('Provided `innersamples` must have shape (S, test_split, inner_split) = ({}, {}, {}); '
                                 'got {}'.format(S, n_cv, inner_split, inner.shape))
            if cvmasks is None:
                raise ValueError('`innersamples` needs `cvsamples`: the inner folds lie inside the training rows of given '
                                 'outer splits')
            if not np.isin(inner, (0, 1, 2)).all():
                raise ValueError('Provided `innersamples` must hold the codes 0 (test row), 1 (training row) and 2 (on '
                                 'neither side) only')
            inner = inner.astype(np.uint8)
            leak = (inner == 2) != ~cvmasks[:, :, None]
            if leak.any():
                p, s_, j = (int(v[0]) for v in np.nonzero(leak))
                raise ValueError('Provided `innersamples` must hold 2 exactly on the outer test rows of its split: an '
                                 'inner fold that touches outer test rows leaks them into the selection; row {} of '
                                 'inner fold {} of split {} does not'.format(p, j, s_))
            te = ((inner == 0) & usable[:, None, None]).sum(axis=0)
            tr = (inner == 1).sum(axis=0) - (n_bad_tr if cv_perm > 0 and n_bad_tr
                                             else ((inner == 1) & ~usable[:, None, None]).sum(axis=0))
            lo_te_in, lo_tr_in = int(te.min()), int(tr.min())
        else:
            # drawn: gen_splits keeps ceil or floor of n (1 - test_size) training rows, of the S rows and again of an
            # outer training set; the worst case over both is checked
            n_out = [int(cvmasks.sum(axis=0).min()), int(cvmasks.sum(axis=0).max())] if cvmasks is not None else \
                [int(np.floor(S * (1 - test_size))), int(np.ceil(S * (1 - test_size)))]
            lo_tr_in = int(np.floor(n_out[0] * (1 - test_size))) - n_bad_tr
            lo_te_in = min(nt - int(np.ceil(nt * (1 - test_size))) for nt in range(n_out[0], n_out[1] + 1)) - n_bad
            if kwargs.get('_classes') is not None:
                # (pls_da: both draws are stratified -- every class keeps ceil or floor of ITS rows, of the S rows and
                # again of an outer training set; the worst case per class, summed)
                cls_ = np.asarray(kwargs['_classes'])
                if cvmasks is not None:
                    m_gs = np.stack([cvmasks[cls_ == g].sum(axis=0) for g in range(int(cls_.max()) + 1)])   # (G, n)
                    lo_tr_in = int(np.floor(m_gs * (1 - test_size)).sum(axis=0).min()) - n_bad_tr
                    lo_te_in = int((m_gs - np.ceil(m_gs * (1 - test_size))).sum(axis=0).min()) - n_bad
                else:
                    n_g = np.bincount(cls_)
                    opts = np.stack([np.floor(n_g * (1 - test_size)), np.ceil(n_g * (1 - test_size))])      # (2, G)
                    lo_tr_in = int(np.floor(opts * (1 - test_size)).min(axis=0).sum()) - n_bad_tr
                    lo_te_in = int((opts - np.ceil(opts * (1 - test_size))).min(axis=0).sum()) - n_bad
        if lo_te_in < 2:
            raise ValueError('Every inner fold needs at least 2 usable test rows; {} of {} ({} rows are NaN throughout)'
                             .format('`innersamples` leaves' if inner is not None else
                                     'test_size = {} can leave'.format(test_size), max(lo_te_in, 0), S, n_bad))
        if n_components > min(lo_tr_in - 1, X.shape[1]):
            raise ValueError('Provided `n_components` cannot be greater than {} with `inner_split`: the smallest inner '
                             'training set has {} usable rows'
                             .format(max(min(lo_tr_in - 1, X.shape[1]), 0), max(lo_tr_in, 0)))
    # ---- split-half: validated on the host before any engine is created or looked up
    sh = None
    if n_split > 0:
        sh = dict(n=n_split, masks=None, perm_given=None)
        usable = _usable_rows(X, Y_agg)
        # under a permutation position p is usable iff row p of X and row perm[p] of Y are: a permutation can put every
        # masked row of X and of Y into one half
        n_bad = int((~usable).sum())
        n_bad_p = int((~_usable_rows(X, np.zeros((S, 1)))).sum()) + int(np.isnan(Y_agg).all(axis=1).sum())
        worst = n_bad_p if (n_perm or 0) > 0 else n_bad
        given = kwargs.get('_splitsamples')
        if given is not None:
            given = np.asarray(given)
            if given.ndim != 2 or given.shape != (S, n_split):
                raise ValueError('Provided `_splitsamples` must have shape (S, n_split) = ({}, {}); got {}'
                                 .format(S, n_split, given.shape))
            given = given.astype(bool)
            halves = np.minimum((given & usable[:, None]).sum(axis=0), (~given & usable[:, None]).sum(axis=0))
            if int(halves.min()) < 2:
                raise ValueError('Every split half needs at least 2 usable rows; split {} leaves {} ({} of {} rows are '
                                 'NaN throughout)'.format(int(halves.argmin()), int(halves.min()), n_bad, S))
            sh['masks'] = given
        pgiven = kwargs.get('_perm_splitsamples')
        if pgiven is not None and (n_perm or 0) > 0:
            pgiven = np.asarray(pgiven)
            if pgiven.ndim != 3 or pgiven.shape != (n_perm, S, n_split):
                raise ValueError('Provided `_perm_splitsamples` must have shape (n_perm, S, n_split) = ({}, {}, {}); '
                                 'got {}'.format(n_perm, S, n_split, pgiven.shape))
            sh['perm_given'] = pgiven = pgiven.astype(bool)
            lo_half = int(min(pgiven.sum(axis=1).min(), (~pgiven).sum(axis=1).min())) - n_bad_p
            if given is None:
                lo_half = min(lo_half, S // 2 - n_bad)
        else:
            lo_half = S // 2 - worst                   # gen_splits keeps ceil or floor of S / 2 rows in the first half
        if (given is None or (n_perm or 0) > 0) and lo_half < 2:
            raise ValueError('Every split half needs at least 2 usable rows; a split can leave {} of {} ({} rows of X or '
                             'Y are NaN throughout)'.format(max(lo_half, 0), S, worst))
    rs = resampling.check_random_state(seed)
    k = n_components
    B, T = X.shape[1], Y_agg.shape[1]

    # ---- everything drawn from `rs`, in the reference's order, on one host thread that
    # ---- starts before the data goes to the device (resampling.DrawThread): the rank-1
    # ---- randomized SVD's normal((min(B, T), 11)) per component (regression.py:103 ->
    # ---- compute.py:43-50), the permutation arrays, the bootstrap arrays
    from .engine import check_index_array

    def svd_seed_draws(r):
        for _ in range(k):
            r.normal(size=(min(B, T), 11))
    jobs = [svd_seed_draws]
    pstream = bstream = None
    if n_perm > 0:
        if permsamples is None:
            pstream = resampling.IndexStream('perm', [S], 1, n_perm)
            jobs.append(pstream.draw)
        else:
            ps = np.asarray(permsamples)
            if ps.ndim != 2 or ps.shape[0] != S:
                raise ValueError('resampling array must have shape (S, n) with S = {}; got {}'.format(S, ps.shape))
            pstream = resampling.IndexStream.of_array(check_index_array(ps, S))
    if n_boot > 0:
        if bootsamples is None:
            bstream = resampling.IndexStream('boot', [S], 1, n_boot)
            jobs.append(bstream.draw)
        else:
            bs = np.asarray(bootsamples)
            if bs.ndim != 2 or bs.shape[0] != S:
                raise ValueError('resampling array must have shape (S, n) with S = {}; got {}'.format(S, bs.shape))
            bstream = resampling.IndexStream.of_array(check_index_array(bs, S))
    cv = None
    if n_cv > 0:
        cv = dict(n=n_cv, masks=cvmasks, classes=kwargs.get('_classes'), given=cvmasks)
        cv['auc'] = bool(kwargs.get('_auc')) and cv['classes'] is not None
        cv['pred'] = cvpred                            # None, the component count of cv_predict=, or 0: the nested one
        if cvmasks is None:
            # one more job at the END of the list: what a seeded call drew before, it draws still
            def cv_draw(r):
                if cv['classes'] is not None:              # (pls_da: stratified by the class codes, at the same place)
                    cv['masks'] = resampling.gen_stratified_splits(cv['classes'], n_cv, seed=r, test_size=test_size)
                else:
                    cv['masks'] = resampling.gen_splits([S], 1, n_cv, seed=r, test_size=test_size)
            jobs.append(cv_draw)
        if cv_perm > 0:
            # ... and the permutations of the cross-validation one more, behind the split masks
            if cvperm is None:
                cv['pstream'] = resampling.IndexStream('perm', [S], 1, cv_perm)
                jobs.append(cv['pstream'].draw)
            else:
                cv['pstream'] = resampling.IndexStream.of_array(cvperm)
            cv['perm_given'] = cvperm
    if sh is not None and sh['masks'] is None:
        # the observed data's split masks: one more job at the END of the list, behind the cross-validation's draws
        # (permutation i takes its masks from a fresh RandomState(i), base.py:705-708: nothing of the call's stream)
        def sh_draw(r):
            sh['masks'] = resampling.gen_splits([S], 1, n_split, seed=r, test_size=0.5)
        jobs.append(sh_draw)
    if inner_split > 0:
        cv['inner'] = inner
        cv['ni'] = inner_split
        cv['inner_select'] = kwargs.get('inner_select')     # (pls_da only; validated there)
        if inner is None:
            # the inner folds: one more job at the END of the list, behind the split-half masks -- per outer split the
            # training rows in ascending row order are split again, everything else holds 2
            def inner_draw(r):
                cv['inner'] = _draw_inner_codes(cv['masks'], inner_split, r, test_size, classes=cv['classes'])
            jobs.append(inner_draw)
    from .engine import default_engine, touch_idle_release
    from . import team as _team
    touch_idle_release()                               # (a pending idle release is pushed back before the engine is looked up)
    eng = kwargs.get('_engine')
    team = None
    if eng is None and kwargs.get('_emulate') is None and parallel._dist() is None:
        # n_proc workers of the reference (pyls/utils.py:252-279) = GPUs of this node, driven from this process
        # (team.py: one context and one host thread per device, ONE all-gather)
        devices = _team.resolve_devices(inputs.get('n_proc'), device_ids)
        if devices is not None and len(devices) > 1:
            team = _team.team_for(devices, transport)
        elif devices is not None:
            eng = default_engine(devices[0])
    draws = resampling.DrawThread(rs, jobs).start()
    try:
        unrefined = 0
        if team is not None:
            res = team.run(lambda rank, world, e: _run_device(
                X, Y, Y_agg, agg, third, inputs, pstream, bstream, draws, permsamples, bootsamples, bootsamples_out,
                k, ci, e, kwargs.get('_phases') if rank == 0 else None, None, team=(rank, team), cv=cv,
                coef_c=coef_components, coef_ci=coef_ci,
                vip_c=vip_components, coef_perm=coef_perm, sh=sh, cf=cf, vip_perm=vip_perm))
            unrefined = team.unrefined
        else:
            eng = eng or default_engine()
            ok = False
            with eng.lock:                             # one analysis at a time per context (shared default engine)
                try:
                    res = _run_device(X, Y, Y_agg, agg, third, inputs, pstream, bstream, draws, permsamples,
                                      bootsamples, bootsamples_out, k, ci, eng, kwargs.get('_phases'),
                                      kwargs.get('_emulate'), cv=cv, coef_c=coef_components, coef_ci=coef_ci,
                                      vip_c=vip_components, coef_perm=coef_perm, sh=sh, cf=cf, vip_perm=vip_perm)
                    ok = True
                finally:
                    if getattr(eng, 'ctx', None):      # nothing of this call leaks into the next one on the context
                        unrefined = eng.end_analysis(warn=ok) or 0
        Engine.warn_unrefined(unrefined, stacklevel=3)  # (outside the finally; attributed to the caller of pls_regression)
        return res
    finally:
        draws.thread.join()
        from .engine import touch_idle_release
        touch_idle_release()                       # (the cached engines are released after IDLE_RELEASE_S idle seconds)


def _run_device(X, Y, Y_agg, agg, third, inputs, pstream, bstream, draws, permsamples, bootsamples,
                bootsamples_out, k, ci, engine, phases=None, emulate=None, team=None, cv=None, coef_c=None,
                coef_ci=False, vip_c=None, coef_perm=False, sh=None, cf=None, vip_perm=False):
    import time
    import torch
    S = len(X)
    t_last = [time.perf_counter()]
    lead = team is None or team[0] == 0                 # the rank that finishes the analysis and speaks for it

    def tick(name):                                     # per-phase wall times (bench.py --mode analysis)
        if phases is None:
            return
        torch.cuda.synchronize(engine.device)
        now = time.perf_counter()
        phases[name] = phases.get(name, 0.0) + 1e3 * (now - t_last[0])
        t_last[0] = now

    # regression.py:395-397 (on copies: the reference centres the caller's X in place)
    Yc = Y_agg.astype(np.float64) - np.nanmean(Y_agg, axis=0, keepdims=True)
    B, T = X.shape[1], Yc.shape[1]
    eng = engine
    clean = bool(np.isfinite(Yc).all())
    if clean:
        # no missing data in Y: bind X as it is -- the device centres it itself (plsx_set_data) -- and let the
        # device say whether X is clean too (a NaN / inf anywhere in a column makes its column mean non-finite):
        # the S x B matrix is not copied, centred or scanned on the host (a host pass over c5's X is 80 ms)
        import torch
        eng.set_data_regression(X, Yc, k)
        clean = bool(torch.isfinite(eng.colmean_dev()).all().item())
    if clean:
        okx = oky = mask = np.ones(S, dtype=bool)
    else:
        Xc = X.astype(np.float64) - np.nanmean(X, axis=0, keepdims=True)
        okx, oky = _row_ok(Xc), _row_ok(Yc)
        mask = okx & oky
        eng.set_data_regression(np.nan_to_num(Xc), np.nan_to_num(Yc), k)
    if cf is not None:
        okx = oky = mask = cf['usable']                # (a row unusable on either side is unusable on both)
    masked = not mask.all()
    if masked:
        eng.simpls_set_row_masks(okx, oky)
    Y_fit = Y_agg                                      # the Y whose rows the fit saw (_fit_yloadings)
    d_gx = d_gy = None
    if cf is not None:
        # X and Y residualised on [1, Z] over the usable rows, on the device, in place; K formed again.  The host
        # arithmetic below reads Y: its residuals (S x T) are formed in numpy, nothing B-sized is
        d_gx, d_gy = eng.simpls_set_confounds(cf['Z'])
        Yc = Y_fit = _residualise(Y_agg.astype(np.float64), cf['Zt'], mask)
    classes = cv.get('classes') if cv is not None else None
    if classes is not None:
        # pls_da: Y is the indicator matrix of these class codes; the cross-validation below also classifies its test
        # rows (plsx_simpls_set_classes / plsx_simpls_cv_class_begin: the confusion counts ride along the batch calls)
        eng.simpls_set_classes(classes)
    res = PLSResults(inputs=inputs)
    tick('h2d_and_bind')

    # the original fit: x_weights (B, k) stay on the device -- sign rule of compute.svd (on r, proportional to the
    # x_weights column, when B > T, otherwise on c: plsx_svd_flip), centring for the sign alignment of the bootstraps,
    # scores -- and come back once, into page-locked memory, while the device resamples
    d_W, pctvar, _ = eng.simpls_decompose_dev()
    eng.simpls_set_original_dev(d_W)
    d_scores = eng.project_dev(d_W)                                # X already centred
    h_W = eng.to_host_async(d_W)
    x_scores = d_scores.cpu().numpy()
    x_scores[~okx] = np.nan                                        # NaN rows stay NaN (X @ W)
    res['x_scores'] = x_scores
    # emulate = (rank, world) of an emulated run on one GPU (bench.py --mode analysis --emulate-world): own shard, the
    # all-gather replaced by a surrogate of the same volume (parallel._surrogate_gather)
    if team is not None:
        rank, world = team[0], team[1].world
    else:
        rank, world = emulate if emulate is not None else parallel.rank_world()
    tick('decompose')

    # this rank's shards (permutations contiguous, bootstraps chunk-cyclic), launched chunk by chunk as the index rows arrive; the
    # results stay on the device until the one collective
    d_perm = d_yl = usum = usq = bsum = bsq = d_keep = d_vkeep = d_cmax = d_ccnt = coefs_obs = None
    d_vmax = d_vcnt = vip_obs = None
    n_perm_tot = pstream.n if pstream is not None else 0
    n_boot_tot = bstream.n if bstream is not None else 0
    from .progress import Bar                            # verbose=True: the reference's bars (pyls/utils.py:128-152)
    show = lead and bool(inputs.get('verbose')) and emulate is None and parallel.rank_world()[0] == 0
    bars = []
    if pstream is not None:
        lo, hi = parallel.shard_bounds(n_perm_tot, rank, world)
        d_perm = eng._zeros((hi - lo, k))
        if coef_perm:
            # the observed coefficients, from the decomposition, uploaded once; each rank opens a series over its own
            # shard: the permutations' coefficients are formed tile by tile along the solver batches, counted against the
            # observed ones and reduced to their maxima over the features (plsx_simpls_coef_perm_begin)
            eng.sync()                                  # (the x_weights are on the host)
            coefs_obs = _model_coefs(_host_array(h_W), Yc[mask].T @ x_scores[mask], x_scores, Y_fit, mask, coef_c)
            d_cobs = eng._dev(coefs_obs, np.float64)
            d_ccnt = torch.zeros((B, T), dtype=torch.int32, device=eng.device)
            d_cmax = eng._zeros((hi - lo, T))
            if hi > lo:
                eng.simpls_coef_perm_begin(coef_c, d_cobs, d_ccnt, d_cmax)
            tick('coefs_perm')                          # (the set-up; the series itself runs inside 'permutations')
        if vip_perm:
            # the same for the VIP scores: the observed ones are the host's `vip`, uploaded once; the permutations' scores
            # are formed tile by tile, counted and reduced to their maxima (plsx_simpls_vip_perm_begin; independent of
            # the coefficient series)
            eng.sync()                                  # (the x_weights are on the host)
            vip_obs = _vip_scores(_host_array(h_W),
                                  _fit_yloadings(Yc[mask].T @ x_scores[mask], x_scores, Y_fit, mask, vip_c), vip_c)
            d_vobs = eng._dev(vip_obs, np.float64)
            d_vcnt = torch.zeros((B,), dtype=torch.int32, device=eng.device)
            d_vmax = eng._zeros((hi - lo,))
            if hi > lo:
                eng.simpls_vip_perm_begin(vip_c, d_vobs, d_vcnt, d_vmax)
            tick('vip_perm')
        bars.append(Bar('Running permutations', hi - lo, show, eng.device))
        # (a solver batch is a latency chain of ~3 k launches whatever its size: few, large chunks -- the first 2048 rows
        # are drawn in 5 ms)
        for a, b in pstream.chunks(lo, hi, first=2048):
            eng.simpls_perm_into(eng.rows_tensor(pstream.rows[a:b]), d_perm[a - lo:b - lo])
            bars[-1].queued(b - a)
        if d_cmax is not None:
            eng.simpls_coef_perm_end()
        if d_vmax is not None:
            eng.simpls_vip_perm_end()
    tick('permutations')
    if bstream is not None:
        bchunks = parallel.shard_chunks(n_boot_tot, rank, world)     # chunk-cyclic share of the bootstraps
        usum, usq = eng._zeros((B, k)), eng._zeros((B, k))
        d_yl = eng._zeros((sum(hi - lo for lo, hi in bchunks), T, k))
        off = 0
        eng.boot_begin(sum(hi - lo for lo, hi in bchunks))     # (plsx_boot_begin: the feature pass may move to boot_finish)
        if coef_c is not None:
            # the coefficients of the coef_c-component model ride along every solver batch (plsx_simpls_coef_begin)
            bsum, bsq = eng._zeros((B, T)), eng._zeros((B, T))
            eng.simpls_coef_begin(coef_c)
            if coef_ci:
                # ... and the series keeps every A_b of this rank's share, (n_local, T, S): the source of the intervals
                d_keep = eng._empty((sum(hi - lo for lo, hi in bchunks), T, S))
                if d_keep.shape[0]:
                    eng.simpls_coef_keep(d_keep)
        if vip_c is not None:
            # the scaled dual weights of the first vip_c components of this rank's share, (n_local, vip_c, S): the source
            # of the VIP series (plsx_simpls_vip_keep; independent of the coefficient series)
            d_vkeep = eng._empty((sum(hi - lo for lo, hi in bchunks), vip_c, S))
            if d_vkeep.shape[0]:
                eng.simpls_vip_keep(d_vkeep)
        bars.append(Bar('Running bootstraps', sum(hi - lo for lo, hi in bchunks), show, eng.device))
        # 3-D Y: a (n, S, T) Y stack per chunk, at most 256 of them and at most 256 MB (S = 24 000, T = 20: 69 rows)
        ylim = max(1, min(256, (256 << 20) // (S * T * 8)))
        for lo, hi in bchunks:
            for a, b in bstream.chunks(lo, hi, first=2048 if third is None else ylim, grow=4 if third is None else 1,
                                       limit=None if third is None else ylim):
                ystack = None
                if third is not None:
                    # Y aggregated over the resampled third axis, NOT centred
                    # (the reference bootstraps the original Y, regression.py:308-310, 408)
                    ystack = np.stack([agg(Y[..., third[:, i]], axis=-1) for i in range(a, b)])
                    if masked:
                        ystack = np.nan_to_num(ystack)         # all-NaN rows are dropped by the row masks
                    ystack = eng._dev(ystack, np.float64)
                eng.simpls_boot_into(eng.rows_tensor(bstream.rows[a:b]), usum, usq,
                                     d_yl[off + a - lo:off + b - lo], ystack=ystack)
                for done in bars:
                    done.poll()
                bars[-1].queued(b - a)
            off += hi - lo
        eng.boot_finish(usum, usq)
    tick('bootstraps')
    if bsum is not None:
        eng.simpls_coef_finish(bsum, bsq)              # each rank closes its own series: ONE pass over the features
        tick('coefs_finish')
    permsamp = bootsamp = None
    if pstream is not None and lead:
        permsamp = np.asarray(permsamples) if permsamples is not None else pstream.samples
    if bstream is not None and lead:
        bootsamp = np.asarray(bootsamples) if bootsamples is not None else bstream.samples
    draws.join()
    for st in (pstream, bstream):
        if st is not None and lead:
            st.warn()
    # cross-validation: this rank's contiguous shard of the splits (the masks exist once the draws are through), in
    # calls of at most one solver batch
    d_cv = d_conf = d_confp = d_auc = d_aucp = d_pred = None
    if cv is not None:
        cvmasks = cv['masks']
        if cf is not None and cv.get('given') is None:
            _check_cvrank(cf, cvmasks)                   # (drawn splits: they exist only now)
        lo, hi = parallel.shard_bounds(cv['n'], rank, world)
        d_cv = [eng._zeros((hi - lo, k, T)), eng._zeros((hi - lo, k, T)), eng._zeros((hi - lo, k + 1, T))]
        if classes is not None:
            # the observed series: one block of confusion counts per split of this rank's shard
            d_conf = torch.zeros((hi - lo, k, T, T), dtype=torch.int32, device=eng.device)
            if hi > lo:
                eng.simpls_cv_class_begin(d_conf)
            if cv['auc']:
                # ... and, beside it, one block of AUC counts (plsx_simpls_cv_auc_begin: an independent series)
                d_auc = torch.zeros((hi - lo, k, T, 2), dtype=torch.int64, device=eng.device)
                if hi > lo:
                    eng.simpls_cv_auc_begin(d_auc)
        if cv.get('pred') is not None:
            # the out-of-fold predictions of this rank's shard: one slot (T, S) per split, appended by the batch calls
            # below -- or, cv_predict='nested', by the outer fits of the nested calls further down -- with the component
            # count of every slot and, on the confound route, the fold-residualised Y beside it
            nbytes = 8 * (hi - lo) * T * S * (2 if cf is not None else 1)
            free = torch.cuda.mem_get_info(eng.device)[0]
            if nbytes > free:
                raise MemoryError('cv_predict: the stack of predictions of {} splits x T = {} x S = {} is {:.3f} GB{}; '
                                  '{:.3f} GB of device memory are free'
                                  .format(hi - lo, T, S, nbytes / 2 ** 30,
                                          ' with the fold-residualised Y beside it' if cf is not None else '',
                                          free / 2 ** 30))
            d_pred = [eng._empty((hi - lo, T, S)), torch.zeros((hi - lo,), dtype=torch.int32, device=eng.device),
                      eng._empty((hi - lo, T, S)) if cf is not None else None]
            if hi > lo and cv['pred'] > 0:
                eng.simpls_cv_pred_begin(cv['pred'], d_pred[0], d_pred[1], d_pred[2])
        bars.append(Bar('Running cross-validation', hi - lo, show, eng.device))
        for a in range(lo, hi, 8192):
            b = min(hi, a + 8192)
            dm = torch.from_numpy(np.ascontiguousarray(cvmasks[:, a:b].T, dtype=np.uint8)).to(eng.device)
            (eng.simpls_crossval_into if cf is None else eng.simpls_crossval_confound_into)(
                dm, *(t[a - lo:b - lo] for t in d_cv))
            for done in bars:
                done.poll()
            bars[-1].queued(b - a)
        if d_conf is not None:
            eng.simpls_cv_class_end()
        if d_auc is not None:
            eng.simpls_cv_auc_end()
        if d_pred is not None and cv['pred'] > 0:
            eng.simpls_cv_pred_end()                   # (before anything else cross-validates on this context)
        tick('crossval')
    # ... and its permutation test: this rank's contiguous shard of the permutations under ALL the splits.  The
    # (permutation, split) fits are formed, scored and reduced over the splits on the device; a rank keeps three rows
    # per permutation.  (Calls of about eight solver batches: the bits do not depend on where a call ends.)
    d_cvp = cvp = None
    if cv is not None and cv.get('pstream') is not None:
        cvp = cv['pstream']
        lo, hi = parallel.shard_bounds(cvp.n, rank, world)
        d_cvp = [eng._zeros((hi - lo, k, T)), eng._zeros((hi - lo, k, T)), eng._zeros((hi - lo, k + 1))]
        bars.append(Bar('Running cross-validation permutations', hi - lo, show, eng.device))
        dm_all = torch.from_numpy(np.ascontiguousarray(cv['masks'].T, dtype=np.uint8)).to(eng.device)
        if classes is not None:
            # the permutation series, opened after the observed one has ended: one block per permutation of this rank's
            # shard, summed over the splits on the device
            d_confp = torch.zeros((hi - lo, k, T, T), dtype=torch.int32, device=eng.device)
            if hi > lo:
                eng.simpls_cv_class_begin(d_confp)
            if cv['auc']:
                d_aucp = torch.zeros((hi - lo, k, T, 2), dtype=torch.int64, device=eng.device)
                if hi > lo:
                    eng.simpls_cv_auc_begin(d_aucp)
        step = max(1, 65536 // cv['n'])
        for a in range(lo, hi, step):
            b = min(hi, a + step)
            cvp.wait(b)
            (eng.simpls_crossval_perm_into if cf is None else eng.simpls_crossval_confound_perm_into)(
                dm_all, eng.rows_tensor(cvp.rows[a:b]), *(t[a - lo:b - lo] for t in d_cvp))
            for done in bars:
                done.poll()
            bars[-1].queued(b - a)
        if d_confp is not None:
            eng.simpls_cv_class_end()
        if d_aucp is not None:
            eng.simpls_cv_auc_end()
        if lead and cv.get('perm_given') is None:
            cvp.warn()
        tick('crossval_perm')
    # nested cross-validation of n_components: the observed pass where the observed cross-validation ran -- this rank's
    # shard of the OUTER splits, each with its inner folds -- and, under cv_perm, this rank's shard of the permutations
    # under all the groups.  Fits, selection and the reduction over the outer splits stay on the device
    # (plsx_simpls_crossval_nested_batch / _perm_batch); a rank keeps 2 T + 1 + k numbers per permutation.
    d_cvn = d_cvnp = d_ncls = d_nclsp = None
    if cv is not None and cv.get('ni'):
        ni = cv['ni']
        codes = nested_codes(cv['masks'], cv['inner'])           # (S, n, 1 + ni)
        d_codes = torch.from_numpy(np.ascontiguousarray(codes.transpose(1, 2, 0))).to(eng.device)
        lo, hi = parallel.shard_bounds(cv['n'], rank, world)
        d_cvn = [eng._zeros((hi - lo, T)), eng._zeros((hi - lo, T)), eng._zeros((hi - lo,)),
                 torch.zeros((hi - lo,), dtype=torch.int32, device=eng.device), eng._zeros((hi - lo, k + 1))]
        step = max(1, 8192 // (1 + ni))
        nested_pred = d_pred is not None and cv['pred'] == 0 and hi > lo
        if nested_pred:
            eng.simpls_cv_pred_begin(0, d_pred[0], d_pred[1], d_pred[2])
        if classes is not None:
            # pls_da: the selection runs on counts, and the selected counts of this rank's outer splits come back -- one
            # confusion block per split, its AUC counts and the pooled inner confusion (plsx_simpls_cvn_class_begin)
            d_ncls = [torch.zeros((hi - lo, T, T), dtype=torch.int32, device=eng.device),
                      torch.zeros((hi - lo, T, 2), dtype=torch.int64, device=eng.device) if cv['auc'] else None,
                      torch.zeros((hi - lo, k, T, T), dtype=torch.int32, device=eng.device)]
            if hi > lo:
                eng.simpls_cvn_class_begin(cv['inner_select'], *d_ncls)
        for a in range(lo, hi, step):
            b = min(hi, a + step)
            eng.simpls_crossval_nested_into(d_codes[a:b], *(t[a - lo:b - lo] for t in d_cvn))
        if d_ncls is not None:
            eng.simpls_cvn_class_end()
        if nested_pred:
            eng.simpls_cv_pred_end()
        tick('crossval_nested')
        if cvp is not None:
            lo, hi = parallel.shard_bounds(cvp.n, rank, world)
            d_cvnp = [eng._zeros((hi - lo, T)), eng._zeros((hi - lo, T)), eng._zeros((hi - lo,)),
                      torch.zeros((hi - lo, k), dtype=torch.int32, device=eng.device)]
            bars.append(Bar('Running nested cross-validation permutations', hi - lo, show, eng.device))
            step = max(1, 65536 // (cv['n'] * (1 + ni)))
            if classes is not None:
                # ... and per permutation of this rank's shard, summed over the outer splits on the device
                d_nclsp = [torch.zeros((hi - lo, T, T), dtype=torch.int32, device=eng.device),
                           torch.zeros((hi - lo, T, 2), dtype=torch.int64, device=eng.device) if cv['auc'] else None]
                if hi > lo:
                    eng.simpls_cvn_class_begin(cv['inner_select'], *d_nclsp)
            for a in range(lo, hi, step):
                b = min(hi, a + step)
                cvp.wait(b)
                eng.simpls_crossval_nested_perm_into(d_codes, eng.rows_tensor(cvp.rows[a:b]),
                                                     *(t[a - lo:b - lo] for t in d_cvnp))
                for done in bars:
                    done.poll()
                bars[-1].queued(b - a)
            if d_nclsp is not None:
                eng.simpls_cvn_class_end()
            tick('crossval_nested_perm')
    # split-half reliability: this rank's contiguous shard of the permutations, block by block as their masks arrive
    # (permutation i: RandomState(i)), the mean over the splits taken on the device in fixed order; the observed
    # arrangement runs on the lead rank.  Per-split values exist in scratch of one block only.
    d_sh = d_sh0 = None
    if sh is not None:
        ns = sh['n']
        if pstream is not None:
            lo, hi = parallel.shard_bounds(n_perm_tot, rank, world)
            d_sh = [eng._zeros((hi - lo, k)), eng._zeros((hi - lo, k))]
            if hi > lo:
                bars.append(Bar('Running split-half resampling of the permutations', hi - lo, show, eng.device))
                mstream = resampling.MaskStream([S], 1, ns, lo, hi, block=128, given=sh['perm_given'])
                try:
                    for a, b, masks in mstream:
                        dm = torch.from_numpy(masks).to(eng.device)
                        uc, vc = eng._empty((b - a, ns, k)), eng._empty((b - a, ns, k))
                        eng.simpls_split_half_into(eng.rows_tensor(pstream.rows[a:b]), dm, uc, vc)
                        eng.mean_splits_into(uc, d_sh[0][a - lo:b - lo])
                        eng.mean_splits_into(vc, d_sh[1][a - lo:b - lo])
                        for done in bars:
                            done.poll()
                        bars[-1].queued(b - a)
                finally:
                    mstream.close()
                if mstream.duplicates and lead:
                    warnings.warn('WARNING: Duplicate split halves used.')
        if lead:
            dm = torch.from_numpy(np.ascontiguousarray(sh['masks'].T[None], dtype=np.uint8)).to(eng.device)
            uc, vc = eng._empty((1, ns, k)), eng._empty((1, ns, k))
            eng.simpls_split_half_into(None, dm, uc, vc)
            d_sh0 = [eng._zeros((1, k)), eng._zeros((1, k))]
            eng.mean_splits_into(uc, d_sh0[0])
            eng.mean_splits_into(vc, d_sh0[1])
        tick('split_half')
    for bar in bars:
        bar.watch()
    try:
        eng.sync()                 # numerical status of the launches above is raised here
    finally:
        for bar in bars:
            bar.close()
    # (the maxima of the coefficient series and of the VIP series ride next to d_perm, contiguous slices like it)
    d_vmax2 = d_vmax[:, None] if d_vmax is not None else None
    slices = [t for t in (d_perm, d_cmax, d_vmax2, d_yl) if t is not None]
    totals = [n for t, n in ((d_perm, n_perm_tot), (d_cmax, n_perm_tot), (d_vmax2, n_perm_tot), (d_yl, n_boot_tot))
              if t is not None]
    cyclic = [len(slices) - 1] if d_yl is not None else []
    if d_cv is not None:                                # the cross-validation rows ride in the same buffer: ONE collective
        slices, totals = slices + d_cv, totals + [cv['n']] * 3
    if d_cvp is not None:                               # ... and the three rows per permutation of its permutation test
        slices, totals = slices + d_cvp, totals + [cvp.n] * 3
    if d_sh is not None:                                # ... and the two rows per permutation of the split-half means
        slices, totals = slices + d_sh, totals + [n_perm_tot] * 2
    if d_conf is not None:                              # ... and the confusion counts of pls_da, as float64: they are exact
        slices, totals = slices + [d_conf.to(torch.float64)], totals + [cv['n']]
    if d_confp is not None:
        slices, totals = slices + [d_confp.to(torch.float64)], totals + [cvp.n]
    for t, n in ((d_auc, cv['n'] if cv is not None else 0), (d_aucp, cvp.n if cvp is not None else 0)):
        if t is not None:                               # ... and the AUC counts, the same way: exact below 2^53
            assert t.numel() == 0 or int(t.max().item()) < 2 ** 53, 'AUC counts beyond 2^53 do not ride as float64'
            slices, totals = slices + [t.to(torch.float64)], totals + [n]
    nest_at = len(slices)
    if d_cvn is not None:                               # ... and the nested scores per outer split, the counts as float64
        slices = slices + [d_cvn[0], d_cvn[1], d_cvn[2][:, None], d_cvn[3].to(torch.float64)[:, None], d_cvn[4]]
        totals = totals + [cv['n']] * 5
    if d_cvnp is not None:                              # ... and their null per permutation
        slices = slices + [d_cvnp[0], d_cvnp[1], d_cvnp[2][:, None], d_cvnp[3].to(torch.float64)]
        totals = totals + [cvp.n] * 4
    ncls_at = len(slices)
    for ts, n in ((d_ncls, cv['n'] if cv is not None else 0), (d_nclsp, cvp.n if cvp is not None else 0)):
        if ts is not None:                              # ... and the selected counts of pls_da, as float64: they are exact
            for t in ts:
                if t is not None:
                    assert t.numel() == 0 or int(t.max().item()) < 2 ** 53, 'counts beyond 2^53 do not ride as float64'
                    slices, totals = slices + [t.to(torch.float64)], totals + [n]
    pred_at = len(slices)
    if d_pred is not None:                              # ... and the out-of-fold predictions, a slot per split
        slices = slices + [d_pred[0], d_pred[1].to(torch.float64)[:, None]] + ([d_pred[2]] if d_pred[2] is not None else [])
        totals = totals + [cv['n']] * (3 if d_pred[2] is not None else 2)
    if d_keep is not None:                              # ... and so does the kept stack, chunk-cyclic like d_yl (its
        slices, totals = slices + [d_keep], totals + [n_boot_tot]      # order is irrelevant to order statistics)
        cyclic = cyclic + [len(slices) - 1]
    if d_vkeep is not None:                             # ... and the kept VIP stack, the same way
        slices, totals = slices + [d_vkeep], totals + [n_boot_tot]
        cyclic = cyclic + [len(slices) - 1]
    sums = [t for t in (usum, usq, bsum, bsq) if t is not None]      # (the coefficient sums join the summed part)
    if d_ccnt is not None:                              # ... and the exceedance counts, as float64: they are exact
        sums = sums + [d_ccnt.to(torch.float64)]
    if d_vcnt is not None:                              # ... and those of the VIP series, the same way
        sums = sums + [d_vcnt.to(torch.float64)[:, None]]
    full, summed = parallel.collect_device(slices, totals, sums, emulate=emulate, cyclic=cyclic, team=team)
    if not lead:
        return None                                     # rank 0 holds everything the ranks computed: it finishes
    d_vstack = full.pop() if d_vkeep is not None else None         # (stay on the device)
    d_stack = full.pop() if d_keep is not None else None
    d_keep = d_vkeep = None
    full = [t.detach().cpu().numpy() for t in full]
    if usum is not None:
        usum, usq = summed[:2]
    if bsum is not None:
        bsum, bsq = summed[2:4]
    tick('collective')
    d_cci = None
    if d_stack is not None:
        # the closing pass over the features, on the lead rank, over the gathered stack (plsx_simpls_coef_ci)
        d_cci = eng.simpls_coef_ci(d_stack.contiguous(), ci=ci)
        tick('coefs_ci')
    d_vci = None
    if d_vstack is not None:
        # the same for the VIP scores (plsx_simpls_vip_ci): standard deviation and interval of every feature's series
        d_vci = eng.simpls_vip_ci(d_vstack.contiguous(), ci=ci)
        tick('vip_ci')
    i = 0
    d_perm = distrib = None
    if pstream is not None:
        d_perm = np.ascontiguousarray(full[i].T)                    # (k, n_perm)
        i += 1
        if d_cmax is not None:
            coefs_max = np.ascontiguousarray(full[i].T)             # (T, n_perm)
            i += 1
        if d_vmax is not None:
            vip_max = np.ascontiguousarray(full[i][:, 0])           # (n_perm,)
            i += 1
    if bstream is not None:
        distrib = np.ascontiguousarray(np.moveaxis(full[i], 0, -1))  # (T, k, n_boot)
        i += 1
    if d_cv is not None:
        cv_r, cv_r2, cv_sse = (np.ascontiguousarray(full[i + j].transpose(2, 1, 0)) for j in range(3))   # (T, k [+ 1], n)
        n_test = (~cv['masks'] & mask[:, None]).sum(axis=0)
        res['cvres'].update(dict(
            pearson_r=np.ascontiguousarray(cv_r[:, k - 1]), r_squared=np.ascontiguousarray(cv_r2[:, k - 1]),
            pearson_r_ncomp=cv_r, r_squared_ncomp=cv_r2, mse=cv_sse.sum(axis=0) / n_test[None, :],
            cvsamples=np.asarray(cv['masks'], dtype=bool)))
        if d_cvp is not None:
            # the null of the split-means: (T, k, P), (T, k, P), (k + 1, P); the observed statistic is the plain mean
            # over the splits of what cvres holds
            P = cvp.n
            null_r, null_r2 = (np.ascontiguousarray(full[i + 3 + j].transpose(2, 1, 0)) for j in range(2))
            null_mse = np.ascontiguousarray(full[i + 5].T)
            obs_r, obs_r2 = cv_r.mean(axis=-1), cv_r2.mean(axis=-1)
            obs_mse = res['cvres']['mse'].mean(axis=-1)
            res['cvres'].update(dict(
                perm_pearson_r=null_r, perm_r_squared=null_r2, perm_mse=null_mse,
                pearson_r_pvals=hostmath.perm_sig(obs_r.ravel(), null_r.reshape(T * k, P)).reshape(T, k),
                r_squared_pvals=hostmath.perm_sig(obs_r2.ravel(), null_r2.reshape(T * k, P)).reshape(T, k),
                mse_pvals=hostmath.perm_sig(-obs_mse, -null_mse),          # (smaller is better: #{null < observed})
                cvpermsamples=np.asarray(cv['perm_given']) if cv.get('perm_given') is not None else cvp.samples))
        if d_conf is not None:
            from .discriminant import confusion_results
            j = i + 3 + (3 if d_cvp is not None else 0) + (2 if d_sh is not None else 0)
            res['cvres'].update(confusion_results(full[j], full[j + 1] if d_confp is not None else None))
            if d_auc is not None:
                from .discriminant import auc_results
                j += 2 if d_confp is not None else 1
                res['cvres'].update(auc_results(full[j], full[j + 1] if d_aucp is not None else None))
        if d_cvn is not None:
            nr, nr2, nmse, nnc, nin = full[nest_at:nest_at + 5]
            res['cvres'].update(dict(
                nested_ncomp=np.rint(nnc[:, 0]).astype(np.int64), nested_pearson_r=np.ascontiguousarray(nr.T),
                nested_r_squared=np.ascontiguousarray(nr2.T), nested_mse=np.ascontiguousarray(nmse[:, 0]),
                inner_mse=np.ascontiguousarray(nin.T), innersamples=np.asarray(cv['inner'], dtype=np.uint8)))
            if d_cvnp is not None:
                # the null of the split means, each permutation with its own selection; the observed statistic is the
                # plain mean over the outer splits of the nested scores
                pr, pr2, pmse, pcnt = full[nest_at + 5:nest_at + 9]
                pr, pr2, pmse = np.ascontiguousarray(pr.T), np.ascontiguousarray(pr2.T), np.ascontiguousarray(pmse[:, 0])
                cr = res['cvres']
                res['cvres'].update(dict(
                    perm_nested_pearson_r=pr, perm_nested_r_squared=pr2, perm_nested_mse=pmse,
                    perm_nested_ncomp=np.ascontiguousarray(np.rint(pcnt).astype(np.int64).T),
                    nested_pearson_r_pvals=hostmath.perm_sig(cr['nested_pearson_r'].mean(axis=-1), pr),
                    nested_r_squared_pvals=hostmath.perm_sig(cr['nested_r_squared'].mean(axis=-1), pr2),
                    nested_mse_pvals=float(hostmath.perm_sig(-np.atleast_1d(cr['nested_mse'].mean()), -pmse[None, :])[0])))
            if d_ncls is not None:
                from .discriminant import nested_results
                nper = 3 if cv['auc'] else 2
                obs = full[ncls_at:ncls_at + nper]
                prm = full[ncls_at + nper:ncls_at + nper + nper - 1] if d_nclsp is not None else None
                res['cvres'].update(nested_results(
                    obs[0], obs[-1], auc_blocks=obs[1] if cv['auc'] else None,
                    perm_blocks=prm[0] if prm is not None else None,
                    perm_auc_blocks=prm[1] if prm is not None and cv['auc'] else None))
    if d_pred is not None:
        # (S, T, n); the centring the front end removed before binding is added back: the units of the Y of the call
        # (not under confounds -- the residuals have no mean -- nor for pls_da, whose slots hold the raw indicators)
        y_pred = np.ascontiguousarray(full[pred_at].transpose(2, 1, 0))
        if cf is None and classes is None:
            y_pred += np.nanmean(Y_agg, axis=0).astype(np.float64)[None, :, None]
        res['cvres'].update(dict(y_pred=y_pred, y_pred_ncomp=np.rint(full[pred_at + 1][:, 0]).astype(np.int32)))
        if d_pred[2] is not None:
            res['cvres']['y_true'] = np.ascontiguousarray(full[pred_at + 2].transpose(2, 1, 0))
        if classes is not None:
            test = ~np.asarray(cv['masks'], dtype=bool) & mask[:, None]
            res['cvres']['predicted'] = np.where(test, np.argmax(np.where(np.isnan(y_pred), -np.inf, y_pred), axis=1),
                                                 -1).astype(np.int32)
    if d_sh0 is not None:
        orig_uc, orig_vc = (t.cpu().numpy()[0] for t in d_sh0)
        res['splitres'].update(dict(ucorr=orig_uc, vcorr=orig_vc))
        if d_sh is not None:
            j = i + (3 if d_cv is not None else 0) + (3 if d_cvp is not None else 0)
            ucorrs, vcorrs = np.ascontiguousarray(full[j].T), np.ascontiguousarray(full[j + 1].T)      # (k, n_perm)
            ull, uul = hostmath.boot_ci(ucorrs, ci=ci)
            vll, vul = hostmath.boot_ci(vcorrs, ci=ci)
            res['splitres'].update(dict(
                ucorr_pvals=hostmath.perm_sig(orig_uc, ucorrs), vcorr_pvals=hostmath.perm_sig(orig_vc, vcorrs),
                ucorr_lolim=ull, vcorr_lolim=vll, ucorr_uplim=uul, vcorr_uplim=vul))
    if permsamp is not None:
        res['permres']['pvals'] = hostmath.perm_sig(pctvar, d_perm)
        res['permres']['permsamples'] = permsamp
        res['permres']['perm_singval'] = d_perm
        if d_cmax is not None:
            cnt = np.rint(summed[-2 if d_vcnt is not None else -1].detach().cpu().numpy()).astype(np.int64)
            res['permres'].update(_coef_perm_pvals(coefs_obs, cnt, coefs_max,
                                                   _feature_scale(X, okx, None if clean else Xc)))
        if d_vmax is not None:
            cnt = np.rint(summed[-1].detach().cpu().numpy()[:, 0]).astype(np.int64)
            res['permres'].update(_vip_perm_pvals(vip_obs, cnt, vip_max))

    res['y_loadings'] = Yc[mask].T @ x_scores[mask]                # regression.py:401
    y_scores = np.full((S, k), np.nan)
    y_scores[mask] = resid_yscores(x_scores[mask], Yc[mask] @ res['y_loadings'])
    res['y_scores'] = y_scores
    res['x_weights'] = _host_array(h_W)
    if coef_c is not None:
        # the model of the first coef_c components (simpls' beta, regression.py:149-151): Y ~ intercept + X @ coefs
        res['coefs'] = coefs_obs if coefs_obs is not None else \
            _model_coefs(res['x_weights'], res['y_loadings'], x_scores, Y_fit, mask, coef_c)
        res['intercept'] = _model_means(X, Y_agg, mask, res['coefs'])
    if vip_c is not None:
        res['vip'] = vip_obs if vip_obs is not None else \
            _vip_scores(res['x_weights'], _fit_yloadings(res['y_loadings'], x_scores, Y_fit, mask, vip_c), vip_c)
    if bootsamp is not None:
        # add the original back, n_boot + 1 (regression.py:409-415)
        d_bsr, d_se = eng.boot_rel_dev(d_W, usum, usq, bootsamp.shape[1] + 1, add_orig=True)
        h_bsr, h_se = eng.to_host_async(d_bsr), eng.to_host_async(d_se)
        eng.sync()
        bsr, se = _host_array(h_bsr), _host_array(h_se)
        res['bootres'].update(dict(
            x_weights_normed=bsr, x_weights_stderr=se, y_loadings=res['y_loadings'],
            y_loadings_boot=distrib,
            y_loadings_ci=np.stack(eng.percentile_ci(distrib, ci=ci), -1),
            bootsamples=bootsamples_out if third is not None else bootsamp))
        if bsum is not None:
            d_cn, d_cse = eng.boot_rel_dev(eng._dev(res['coefs'], np.float64), bsum, bsq, bootsamp.shape[1] + 1,
                                           add_orig=True)
            eng.sync()
            res['bootres'].update(dict(coefs_normed=d_cn.cpu().numpy(), coefs_stderr=d_cse.cpu().numpy()))
        if d_cci is not None:
            res['bootres']['coefs_ci'] = np.stack([d_cci[0].cpu().numpy(), d_cci[1].cpu().numpy()], -1)
        if d_vci is not None:
            res['bootres'].update(dict(vip_stderr=d_vci[0].cpu().numpy(),
                                       vip_ci=np.stack([d_vci[1].cpu().numpy(), d_vci[2].cpu().numpy()], -1)))
    res['varexp'] = pctvar                                          # regression.py:425-426
    if cf is not None:
        res['confound_mean'] = cf['zmean']
        res['confound_x'], res['confound_y'] = d_gx.cpu().numpy(), d_gy.cpu().numpy()
    tick('host_finish')
    return res


def _residualise(A, Zt, rows):
    """A (S, n) residualised on the columns of Zt (S, q + 1: the intercept and the centred confounds) by the least
    squares fit over ``rows`` (bool), applied to every row; rows outside ``rows`` whose Zt is zero keep A."""
    G = np.linalg.lstsq(Zt[rows], A[rows], rcond=None)[0]
    return A - Zt @ G


def _check_cvrank(cf, masks):
    """The confounds must have full column rank, together with the intercept, on the training rows of every split."""
    Zt, usable = cf['Zt'], cf['usable']
    for s in range(masks.shape[1]):
        tr = masks[:, s] & usable
        if np.linalg.matrix_rank(Zt[tr]) < Zt.shape[1]:
            raise ValueError('Provided `confounds` are rank deficient together with the intercept on the {} training '
                             'rows of split {}'.format(int(tr.sum()), s))


def _feature_scale(X, okx, Xc=None):
    """s_f (B,): the standard deviation (n - 1) of every feature over the usable rows of X -- the scale of the
    standardised coefficients of ``coef_perm``.  Xc: the centred X where the caller already holds it (masked rows NaN or
    zero); otherwise X is centred here, a block of columns at a time."""
    S, B = X.shape
    n_x = int(np.sum(okx))
    ss = np.empty(B)
    step = max(1, (32 << 20) // (8 * S))
    for lo in range(0, B, step):
        blk = (Xc if Xc is not None else X)[:, lo:lo + step][okx].astype(np.float64)
        if Xc is None:
            blk = blk - blk.mean(axis=0, keepdims=True)
        ss[lo:lo + step] = np.einsum('sf,sf->f', blk, blk)
    return np.sqrt(ss / (n_x - 1))


def _coef_perm_pvals(coefs, count, coefs_max, scale):
    """The three arrays ``coef_perm`` adds to permres.  coefs (B, T) observed; count (B, T) = #{p : |b_p| >= |coefs|};
    coefs_max (T, n_perm) = max_f s_f |b_p[f, t]|; scale (B,) = s_f.  The maxT p-value counts, per behaviour, the
    maxima at or above the observed standardised magnitude: one sort and one searchsorted per behaviour."""
    n_perm = coefs_max.shape[1]
    obs = scale[:, None] * np.abs(coefs)
    fwe = np.empty(coefs.shape)
    for t in range(coefs.shape[1]):
        null = np.sort(coefs_max[t])
        fwe[:, t] = (n_perm - np.searchsorted(null, obs[:, t], side='left') + 1) / (n_perm + 1)
    return dict(coefs_pvals=(count + 1) / (n_perm + 1), coefs_max=coefs_max, coefs_pvals_fwe=fwe)


def _vip_perm_pvals(vip, count, vip_max):
    """The three arrays ``vip_perm`` adds to permres.  vip (B,) observed; count (B,) = #{p : vip_p >= vip}; vip_max
    (n_perm,) = max_f vip_p[f] as the device leaves it: 0, the identity of its maximum, for a degenerate permuted fit --
    every real fit has max_f vip >= 1 since sum(vip**2) == B -- which is reported as NaN and counts nowhere.  The maxT
    p-value counts the maxima at or above the observed score: one sort and one searchsorted.  Where vip is NaN both
    p-values are NaN."""
    vip = np.asarray(vip, dtype=np.float64)
    n_perm = vip_max.shape[0]
    null = np.sort(vip_max[vip_max > 0])
    nan = np.isnan(vip)
    fwe = (null.shape[0] - np.searchsorted(null, np.where(nan, 0.0, vip), side='left') + 1) / (n_perm + 1)
    return dict(vip_pvals=np.where(nan, np.nan, (count + 1) / (n_perm + 1)),
                vip_max=np.where(vip_max > 0, vip_max, np.nan),
                vip_pvals_fwe=np.where(nan, np.nan, fwe))


def _fit_yloadings(Q, x_scores, Y_agg, mask, c):
    """simpls' own y_loadings (T, c) of the first c components.  Without masked rows that is the result's own
    ``y_loadings``.  With rows that are NaN throughout, X and Y are centred over different rows than the fit uses
    (np.nanmean per matrix, regression.py:395-397), so ``y_loadings`` = Yc^T x_scores carries the product of the two
    offsets; simpls' own are taken from the scores and Y centred over the rows of the fit."""
    Q = np.asarray(Q, dtype=np.float64)
    if not mask.all():
        t = np.asarray(x_scores, dtype=np.float64)[mask][:, :c]
        y = np.asarray(Y_agg, dtype=np.float64)[mask]
        Q = (y - y.mean(axis=0)).T @ (t - t.mean(axis=0))
    return Q[:, :c]


def _model_coefs(W, Q, x_scores, Y_agg, mask, c):
    """coefs (B, T) = W[:, :c] @ Q[:, :c].T with Q simpls' y_loadings (regression.py:149-151; :func:`_fit_yloadings`)."""
    W = np.asarray(W, dtype=np.float64)
    return np.ascontiguousarray(W[:, :c] @ _fit_yloadings(Q, x_scores, Y_agg, mask, c).T)


def _vip_scores(W, Q, c):
    """VIP (B,) of the first c components from x_weights W (B, k) and simpls' y_loadings Q (T, >= c): the formula of
    MATLAB's ``plsregress`` documentation with unit-norm x_scores.  A model that explains nothing or a component of
    zero weight norm gives NaN (0 / 0)."""
    W, Q = np.asarray(W, dtype=np.float64)[:, :c], np.asarray(Q, dtype=np.float64)[:, :c]
    ssq = (Q ** 2).sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sqrt(W.shape[0] * ((W ** 2 / (W ** 2).sum(axis=0)) @ ssq) / ssq.sum())


def _model_means(X, Y_agg, mask, coefs):
    """intercept (T,) = ybar - xbar @ coefs, means over the rows the fit used."""
    X, Y_agg = np.asarray(X, dtype=np.float64), np.asarray(Y_agg, dtype=np.float64)
    if not mask.all():
        X, Y_agg = X[mask], Y_agg[mask]
    return Y_agg.mean(axis=0) - X.mean(axis=0) @ coefs


def _fit_of(results, n_components, default_key, X_new=None):
    """What predict / vip need of a ``pls_regression`` result: W, Q, X, Y aggregated, the mask of the rows of the fit,
    the scores and the component count (``n_components=None``: ``inputs[default_key]``, otherwise all components).
    ``X_new``: new rows, checked against W."""
    inputs = results.get('inputs') if hasattr(results, 'get') else None
    W, Q = (results.get('x_weights'), results.get('y_loadings')) if inputs is not None else (None, None)
    if inputs is None or W is None or Q is None or results.get('singvals') is not None \
            or inputs.get('n_components') is None or inputs.get('X') is None or inputs.get('Y') is None:
        raise ValueError('`results` is not a pls_regression result (x_weights, y_loadings and the inputs X, Y, '
                         'n_components are needed)')
    W, Q = np.asarray(W, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    X, Y = np.asarray(inputs['X'], dtype=np.float64), np.asarray(inputs['Y'], dtype=np.float64)
    if X_new is not None and (X_new.ndim != 2 or X_new.shape[1] != W.shape[0]):
        raise ValueError('`X_new` must have shape (S_new, {}); got {}'.format(W.shape[0], X_new.shape))
    k = W.shape[1]
    if n_components is None:
        n_components = inputs.get(default_key)
        n_components = k if n_components is None else int(n_components)
    if isinstance(n_components, bool) or int(n_components) != n_components or not 1 <= int(n_components) <= k:
        raise ValueError('`n_components` must be an integer in 1 .. {}; got {!r}'.format(k, n_components))
    c = int(n_components)
    if Y.ndim == 3:
        aggfunc = inputs.get('aggfunc')
        aggfunc = aggfunc.decode() if isinstance(aggfunc, bytes) else aggfunc
        if not callable(aggfunc) and aggfunc not in _AGGFUNCS:
            raise ValueError('`results.inputs.aggfunc` must be callable or one of {}'.format(sorted(_AGGFUNCS)))
        Y = _AGGFUNCS.get(aggfunc, aggfunc)(Y, axis=-1)
    mask = ~(np.isnan(X).all(axis=1) | np.isnan(Y).all(axis=1))
    Z = inputs.get('confounds')
    Y_fit = Y
    if Z is not None:
        # a fit with confounds saw the residuals of Y on [1, Z] over its usable rows
        Z = np.asarray(Z, dtype=np.float64).reshape(len(X), -1)
        mask = mask & ~np.isnan(Z).all(axis=1)
        Zt = np.c_[np.ones(len(X)), np.where(mask[:, None], Z - Z[mask].mean(axis=0), 0.0)]
        Y_fit = _residualise(Y, Zt, mask)
    x_scores = results.get('x_scores')
    if x_scores is None and not mask.all():
        x_scores = np.full((len(X), k), np.nan)
        x_scores[mask] = (X[mask] if Z is None else _residualise(X, Zt, mask)[mask]) @ W
    return W, Q, X, Y, mask, x_scores, c, Y_fit


def predict(results, X_new, n_components=None, confounds=None):
    """Predict Y (S_new, T) for new rows ``X_new`` (S_new, B) with the model of the first ``n_components`` SIMPLS
    components of a ``pls_regression`` result: ``intercept + X_new @ coefs`` with
    ``coefs = x_weights[:, :c] @ y_loadings[:, :c].T`` (simpls' ``beta``, pyls/types/regression.py:149-151).

    Works on any ``pls_regression`` result, also one read back by ``load_results``: the means come from
    ``results.inputs`` (X, Y, ``aggfunc``), over the rows the fit used (rows that are NaN throughout are left out).
    ``n_components=None``: the ``coef_components`` the result was computed with, otherwise all components.
    Host numpy: one thin product.

    A fit with ``confounds`` needs the new rows' ``confounds=Z_new`` (S_new, q) and predicts
    ``intercept + X_new @ coefs + (Z_new - confound_mean) @ (confound_y - confound_x @ coefs)``: the model of the
    residuals, written in the raw variables.  ValueError when a fit with confounds is given none, or a fit without
    confounds is given some."""
    X_new = np.asarray(X_new, dtype=np.float64)
    W, Q, X, Y, mask, x_scores, c, Y_fit = _fit_of(results, n_components, 'coef_components', X_new)
    fitted = results['inputs'].get('confounds') is not None
    if fitted and confounds is None:
        raise ValueError('`results` was fitted with confounds: predict needs `confounds=Z_new` for the new rows')
    if not fitted and confounds is not None:
        raise ValueError('`results` was fitted without confounds: predict takes none')
    coefs = _model_coefs(W, Q, x_scores, Y_fit, mask, c)
    out = _model_means(X, Y, mask, coefs) + X_new @ coefs
    if fitted:
        zmean, gx, gy = (results.get(key) for key in ('confound_mean', 'confound_x', 'confound_y'))
        if zmean is None or gx is None or gy is None:
            raise ValueError('`results` was fitted with confounds but lacks confound_mean / confound_x / confound_y')
        zmean, gx, gy = (np.asarray(a, dtype=np.float64) for a in (zmean, gx, gy))
        Z_new = np.asarray(confounds, dtype=np.float64)
        if Z_new.ndim == 1:
            Z_new = Z_new[:, None]
        if Z_new.ndim != 2 or Z_new.shape != (len(X_new), len(zmean)):
            raise ValueError('`confounds` must have shape (S_new, q) = ({}, {}); got {}'
                             .format(len(X_new), len(zmean), Z_new.shape))
        out = out + (Z_new - zmean) @ (gy - gx @ coefs)
    return out


def vip(results, n_components=None):
    """VIP scores (B,), variable importance in projection, of the model of the first ``n_components`` SIMPLS components
    of a ``pls_regression`` result -- the formula of MATLAB's ``plsregress`` documentation with unit-norm x_scores:

        ssq_a  = |y_loadings[:, a]|**2                                                    a = 0 .. c - 1
        vip[f] = sqrt(B * sum_a ssq_a * x_weights[f, a]**2 / |x_weights[:, a]|**2 / sum_a ssq_a)

    so that ``sum(vip**2) == B``; independent of the signs and the order of the components.  The models are nested: a
    k-component fit serves every c <= k.  Works on any ``pls_regression`` result, also one read back by
    ``load_results``; with rows that are NaN throughout the y_loadings are simpls' own, centred over the rows of the
    fit (as for :func:`predict`).  ``n_components=None``: the ``vip_components`` the result was computed with,
    otherwise all components.  ``results.vip`` of ``pls_regression(vip_components=c)`` is this function's value.  Host
    numpy."""
    W, Q, X, Y, mask, x_scores, c, Y_fit = _fit_of(results, n_components, 'vip_components')
    return _vip_scores(W, _fit_yloadings(Q, x_scores, Y_fit, mask, c), c)
