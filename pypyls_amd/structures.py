"""
Result / input containers with the reference's key layout
(pyls/structures.py:146-351, pyls/utils.py:16-125): dictionary objects with
attribute access that silently drop keys they do not know.
"""
import os

import numpy as np


class KeyedRecord(dict):
    """dict with attribute access restricted to ``allowed`` keys."""

    allowed = ()

    def __init__(self, **kwargs):
        super().__init__()
        for key, val in kwargs.items():
            self[key] = val

    def __setitem__(self, key, val):
        if key in type(self).allowed:
            super().__setitem__(key, val)

    def update(self, *args, **kwargs):
        for key, val in dict(*args, **kwargs).items():
            self[key] = val

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key)

    def __setattr__(self, key, val):
        self[key] = val

    def __delattr__(self, key):
        try:
            del self[key]
        except KeyError:
            raise AttributeError(key)

    def __dir__(self):
        return list(self.keys())

    def _filled(self):
        out = set()
        for key, val in self.items():
            if val is None:
                continue
            if isinstance(val, dict) and len(val) == 0:
                continue
            if isinstance(val, KeyedRecord) and not val._filled():
                continue
            out.add(key)
        return out

    def __repr__(self):
        keys = [k for k in type(self).allowed if k in self._filled()]
        return '{}({})'.format(type(self).__name__, ', '.join(keys))

    __str__ = __repr__

    def __eq__(self, other):
        if not isinstance(other, type(self)):
            return False
        if self._filled() != other._filled():
            return False
        for key in self._filled():
            a, b = self[key], other[key]
            if isinstance(a, dict) and isinstance(b, dict):
                if a != b:
                    return False
                continue
            try:
                np.testing.assert_array_almost_equal(a, b)
            except (TypeError, AssertionError):
                return False
        return True

    def __ne__(self, other):
        return not self == other

    __hash__ = None


class PLSInputs(KeyedRecord):
    allowed = (
        'X', 'Y', 'groups', 'n_cond', 'n_perm', 'n_boot', 'n_split',
        'test_split', 'test_size', 'mean_centering', 'covariance', 'rotate',
        'ci', 'seed', 'verbose', 'n_proc', 'bootsamples', 'permsamples',
        'method', 'n_components', 'aggfunc', 'permindices',
        'coef_components',                  # pls_regression: component count of the returned model (only when asked for)
        'coef_ci',                          # pls_regression: percentile intervals of its coefficients (only when asked for)
        'cv_perm',                          # pls_regression: permutations of the cross-validation (only when asked for)
        'coef_perm',                        # pls_regression: permutation p-values of its coefficients (only when asked for)
        'vip_components',                   # pls_regression: component count of the VIP scores (only when asked for)
        'vip_perm',                         # pls_regression: permutation p-values of its VIP scores (only when asked for)
        'contrasts',                        # behavioral_pls / meancentered_pls: non-rotated PLS, (T', Lc) (only when given)
        'weights_ci',                       # behavioral_pls / meancentered_pls: percentile intervals of the x_weights (only when given)
        'weights_perm',                     # behavioral_pls / meancentered_pls: permutation p-values of the x_weights (only when given)
        'confounds',                        # pls_regression / behavioral_pls: the nuisance variables Z (S, q) (only when given)
        'inner_split',                      # pls_regression: inner folds of the nested cross-validation (only when asked for)
        'inner_select',                     # pls_da: the criterion of the nested selection (only when inner_split is given)
        'cv_predict',                       # pls_regression / pls_da / behavioral_pls: the out-of-fold predictions are returned (only when asked for)
        'cv_lv',                            # behavioral_pls: out-of-sample score correlation of the latent variables (only when given)
        # build-only knobs (filtered like any other key): pre-drawn split masks, engine
        '_splitsamples', '_perm_splitsamples', '_cvsplits', '_engine',
        '_classes',                         # pls_da: class code of every row (Y is their indicator matrix)
        '_auc',                             # pls_da(auc=True): the cross-validation also returns AUC counts (only when asked for)
    )

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        # pyls/structures.py:156-172
        if self.get('n_split') == 0:
            self['n_split'] = None
        if self.get('test_split') == 0:
            self['test_split'] = None
        n_proc = self.get('n_proc')
        if n_proc is not None:
            ncpu = os.cpu_count() or 1
            if n_proc == 'max' or n_proc == -1:
                self['n_proc'] = ncpu
            elif n_proc < 0:
                self['n_proc'] = ncpu + 1 + n_proc
        ts = self.get('test_size')
        if ts is not None and (ts < 0 or ts >= 1):
            raise ValueError('test_size must be in [0, 1). Provided value: {}'.format(ts))


class PLSBootResults(KeyedRecord):
    allowed = ('x_weights_normed', 'x_weights_stderr', 'bootsamples',
               'y_loadings', 'y_loadings_boot', 'y_loadings_ci',
               'contrast', 'contrast_boot', 'contrast_ci',
               # pls_regression(coef_components=c): standard error of the model coefficients over the bootstraps and
               # the coefficients over it, (B, T) -- one map per behaviour
               'coefs_stderr', 'coefs_normed',
               # pls_regression(coef_components=c, coef_ci=True): (B, T, 2) lower / upper percentile bound of the
               # coefficients over the n_boot bootstraps (the original is not added to the series, as for y_loadings_ci)
               'coefs_ci',
               # pls_regression(vip_components=c): (B,) standard deviation (ddof = 1) and (B, 2) lower / upper percentile
               # bound of the VIP scores over the n_boot bootstraps (the original is not added to the series)
               'vip_stderr', 'vip_ci',
               # behavioral_pls / meancentered_pls(weights_ci=m): (B, m, 2) lower / upper percentile bound of the rotated
               # bootstrap weights U_b over the n_boot bootstraps, in the units of x_weights @ diag(singvals) -- the
               # numerator of x_weights_normed (the original is not added to the series, as for y_loadings_ci)
               'x_weights_ci')


class PLSPermResults(KeyedRecord):
    # pls_regression(coef_components=c, coef_perm=True): coefs_pvals (B, T) uncorrected two-sided p-values of the
    # coefficients, coefs_max (T, n_perm) the null of the max statistic over standardised coefficients per behaviour,
    # coefs_pvals_fwe (B, T) the maxT p-values (family-wise over the features of one behaviour)
    # pls_regression(vip_components=c, vip_perm=True): vip_pvals (B,) uncorrected one-sided p-values of the VIP scores,
    # vip_max (n_perm,) the null of the max statistic over the features (NaN for a degenerate permuted fit),
    # vip_pvals_fwe (B,) the maxT p-values (family-wise over the features)
    # behavioral_pls / meancentered_pls(weights_perm=m): x_weights_pvals (B, m) uncorrected two-sided p-values of
    # x_weights @ diag(singvals) against Z_p = R_p.T @ y_weights[:, :m], x_weights_max (m, n_perm) the null of the max
    # statistic over the features per latent variable (scaled by the feature's standard deviation outside correlation
    # mode), x_weights_pvals_fwe (B, m) the maxT p-values (family-wise over the features of one latent variable)
    allowed = ('pvals', 'permsamples', 'perm_singval', 'coefs_pvals', 'coefs_max', 'coefs_pvals_fwe',
               'vip_pvals', 'vip_max', 'vip_pvals_fwe', 'x_weights_pvals', 'x_weights_max', 'x_weights_pvals_fwe')


class PLSSplitHalfResults(KeyedRecord):
    allowed = ('ucorr', 'vcorr', 'ucorr_pvals', 'vcorr_pvals',
               'ucorr_uplim', 'vcorr_uplim', 'ucorr_lolim', 'vcorr_lolim')


class PLSCrossValidationResults(KeyedRecord):
    # pearson_r_ncomp / r_squared_ncomp (T, k, n), mse (k + 1, n), cvsamples (S, n): pls_regression's cross-validation
    # per component count (no counterpart in the reference, which cross-validates behavioral PLS only)
    # pls_regression(cv_perm=P): the null of the split-means under permuted Y -- perm_pearson_r / perm_r_squared
    # (T, k, P), perm_mse (k + 1, P) -- its p-values (T, k), (T, k), (k + 1,) and the permutations (S, P)
    # behavioral_pls(cv_lv=m): lv_corr (m, n) the out-of-sample correlation of brain and behaviour scores per latent
    # variable and split; with cv_perm=P: perm_lv_corr (m, P) the split means under permuted Y, lv_corr_pvals (m,)
    allowed = ('pearson_r', 'r_squared', 'pearson_r_ncomp', 'r_squared_ncomp', 'mse', 'cvsamples',
               'lv_corr', 'perm_lv_corr', 'lv_corr_pvals',
               'perm_pearson_r', 'perm_r_squared', 'perm_mse', 'pearson_r_pvals', 'r_squared_pvals', 'mse_pvals',
               'cvpermsamples',
               # pls_da: confusion (G, G, k, n) int [true, predicted, c - 1, split], accuracy / balanced_accuracy (k, n);
               # with cv_perm=P: perm_confusion (G, G, k, P) summed over the splits of a permutation, perm_accuracy /
               # perm_balanced_accuracy (k, P) of that sum, accuracy_pvals / balanced_accuracy_pvals (k,)
               'confusion', 'accuracy', 'balanced_accuracy', 'perm_confusion', 'perm_accuracy',
               'perm_balanced_accuracy', 'accuracy_pvals', 'balanced_accuracy_pvals',
               # pls_da(auc=True): auc_counts (G, 2, k, n) int [class, (u2, pairs), c - 1, split], auc (G, k, n) one-vs-rest
               # AUC = u2 / (2 pairs), auc_macro (k, n) its mean over the classes with a pair; with cv_perm=P:
               # perm_auc_counts (G, 2, k, P) summed over the splits of a permutation, perm_auc (G, k, P) / perm_auc_macro
               # (k, P) of that sum, auc_pvals (G, k) / auc_macro_pvals (k,)
               'auc_counts', 'auc', 'auc_macro', 'perm_auc_counts', 'perm_auc', 'perm_auc_macro', 'auc_pvals',
               'auc_macro_pvals',
               # pls_regression(inner_split=ni): nested cross-validation of n_components -- nested_ncomp (n,) int the
               # component count the ni inner folds of outer split s chose (0: undefined), nested_pearson_r /
               # nested_r_squared (T, n) and nested_mse (n,) the outer test rows' scores at that count, inner_mse
               # (k + 1, n) the mean inner-fold mse per count (row 0 the intercept-only model), innersamples
               # (S, n, ni) uint8 codes (1 = training row, 0 = test row, 2 = on neither side: the outer test rows);
               # with cv_perm=P: perm_nested_pearson_r / perm_nested_r_squared (T, P), perm_nested_mse (P,) the split
               # means with the selection repeated inside every permutation, perm_nested_ncomp (k, P) int how many outer
               # splits of a permutation chose c, nested_pearson_r_pvals / nested_r_squared_pvals (T,), nested_mse_pvals
               'nested_ncomp', 'nested_pearson_r', 'nested_r_squared', 'nested_mse', 'inner_mse', 'innersamples',
               'perm_nested_pearson_r', 'perm_nested_r_squared', 'perm_nested_mse', 'perm_nested_ncomp',
               'nested_pearson_r_pvals', 'nested_r_squared_pvals', 'nested_mse_pvals',
               # pls_da(inner_split=ni): the selection runs on counts (inner_select) -- inner_confusion (G, G, k, n) int the
               # confusion pooled over the inner folds, inner_accuracy / inner_balanced_accuracy (k, n) of it,
               # nested_confusion (G, G, n) int the outer test rows' confusion at nested_ncomp, nested_accuracy /
               # nested_balanced_accuracy (n,); with auc=True nested_auc_counts (G, 2, n) int, nested_auc (G, n),
               # nested_auc_macro (n,); with cv_perm=P: perm_nested_confusion (G, G, P) / perm_nested_auc_counts (G, 2, P)
               # summed over the outer splits of a permutation, their scores (P,) / (G, P) / (P,) and the p-values of
               # the pooled statistic (scalars; nested_auc_pvals (G,))
               'inner_confusion', 'inner_accuracy', 'inner_balanced_accuracy', 'nested_confusion', 'nested_accuracy',
               'nested_balanced_accuracy', 'nested_auc_counts', 'nested_auc', 'nested_auc_macro',
               'perm_nested_confusion', 'perm_nested_accuracy', 'perm_nested_balanced_accuracy',
               'nested_accuracy_pvals', 'nested_balanced_accuracy_pvals', 'perm_nested_auc_counts', 'perm_nested_auc',
               'perm_nested_auc_macro', 'nested_auc_pvals', 'nested_auc_macro_pvals',
               # behavioral_pls(cv_predict=True): y_pred (S, T, n) and, with confounds=, y_true (S, T, n)
               # pls_regression / pls_da(cv_predict=): y_pred (S, T, n) the out-of-fold prediction of every usable test
               # row of every split (NaN elsewhere) by the model of y_pred_ncomp (n,) int32 components, in the units of
               # the Y of the call (pls_da: the predicted indicators); with confounds= the prediction of the
               # fold-residualised test Y, which y_true (S, T, n) holds; pls_da: predicted (S, n) int32, the index into
               # `classes` of the first maximum of the predicted indicators (-1 off the test rows)
               'y_pred', 'y_pred_ncomp', 'y_true', 'predicted')


class PLSResults(KeyedRecord):
    """Top-level result object; layout of pyls/structures.py:198-246."""
    allowed = ('x_weights', 'y_weights', 'x_scores', 'y_scores', 'y_loadings',
               'singvals', 'varexp', 'permres', 'bootres', 'splitres', 'cvres',
               'inputs',
               # pls_regression(coef_components=c): Y ~ intercept (T,) + X @ coefs (B, T)
               'coefs', 'intercept',
               # pls_regression(vip_components=c): (B,) variable importance in projection of the c-component model
               'vip',
               # pls_regression / behavioral_pls(confounds=Z): zbar (q,) over the rows of the fit and the slopes of X (q, B) and of Y
               # (q, T) on Z - zbar; every other array of the result speaks of the residuals
               'confound_mean', 'confound_x', 'confound_y',
               # pls_da: (G,) the sorted distinct labels; column g of Y is the indicator of classes[g]
               'classes')

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self['inputs'] = PLSInputs(**kwargs.get('inputs', kwargs))
        self['bootres'] = PLSBootResults(**kwargs.get('bootres', kwargs))
        self['permres'] = PLSPermResults(**kwargs.get('permres', kwargs))
        self['splitres'] = PLSSplitHalfResults(**kwargs.get('splitres', kwargs))
        self['cvres'] = PLSCrossValidationResults(**kwargs.get('cvres', kwargs))
