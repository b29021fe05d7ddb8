"""Behavioural cross-validation without a GPU: the numpy definition the device is held to (tests/crossval_expect.py)
against the oracle where both are defined, against the reference's goldens, and the conditions -- conditioning,
rank, sizes of the cells -- that the tolerance of tests/test_gpu_crossval.py rests on, for every mask of every case."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, assert_close
from oracle import cpu_ref as ref
import crossval_expect as cx

GOLDENS = ['bpls_cv', 'bpls_2g2c_cv', 'bpls_cv_cov']


def _golden_spec(g):
    return ref.Spec('behavioral', list(g['groups']), int(g['n_cond']), bool(g.get('covariance', False)))


def test_rank_threshold_is_the_librarys():
    """The expectation drops latent variables by the oracle's RANK_RTOL; k_cv_final by PLSX_RANK_RTOL."""
    with open(os.path.join(ROOT, 'pypyls_amd', 'csrc', 'plsx_common.h')) as fh:
        m = re.search(r'#define\s+PLSX_RANK_RTOL\s+(\S+)', fh.read())
    assert m and float(m.group(1)) == ref.RANK_RTOL


@pytest.mark.parametrize('name', cx.FULL_RANK)
def test_full_rank_cases_equal_the_oracle(name):
    """Every latent variable live: the definition is the reference's, to rounding (first 4 masks)."""
    spec, X, Y, masks = cx.problem(name)
    r, r2, info = cx.expected(name)
    k = min(4, masks.shape[1])
    assert all(i['n_live'] == i['L'] for i in info)
    want_r, want_r2 = ref.crossval(spec, X, Y, masks[:, :k])
    e_r, e_r2 = cx.errors(r[:, :k], r2[:, :k], want_r, want_r2)
    print('{}: expectation vs oracle: r {:.1e}, r2 {:.1e}'.format(name, e_r, e_r2))
    assert e_r <= 1e-12 and e_r2 <= 1e-12


@pytest.mark.parametrize('name', GOLDENS)
def test_goldens_of_the_reference(name):
    """The reference's own cvres, at the tolerance tests/test_oracle.py asks of the oracle; and the conditioning the
    per-entry check of the front-end test (tests/test_gpu_frontend.py) rests on."""
    g = load_golden(name)
    r, r2, info = cx.crossval(_golden_spec(g), g['X'], g['Y'], g['cv_splits'])
    assert_close(r, g['ref_cvres__pearson_r'], 1e-9, what='pearson_r')
    assert_close(r2, g['ref_cvres__r_squared'], 1e-9, what='r_squared')
    assert all(i['n_live'] == i['L'] and i['kappa'] <= cx.KAPPA_MAX for i in info), info


@pytest.mark.parametrize('name', list(cx.CASES))
def test_conditions_of_the_gpu_cases(name):
    case = cx.CASES[name]
    spec, X, Y, masks = cx.problem(name)
    r, r2, info = cx.expected(name)
    S, T, J = case['S'], case['T'], spec.dummy.shape[1]
    assert masks.shape == (S, case['m']) and masks.dtype == bool
    assert r.shape == r2.shape == (T, case['m'])
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(r2))
    assert len({masks[:, i].tobytes() for i in range(masks.shape[1])}) == case['m']       # no split twice
    dummy = spec.dummy.astype(bool)
    L = min(J * T, case['B'])
    print('{}: kappa <= {:.3g}, live {} of {}, gap <= {:.1e}'.format(
        name, max(i['kappa'] for i in info), sorted({i['n_live'] for i in info}), L, max(i['gap'] for i in info)))
    for i, inf in enumerate(info):
        tr, te = masks[:, i], ~masks[:, i]
        assert inf['L'] == L
        assert inf['kappa'] <= cx.KAPPA_MAX, (i, inf)
        if case['deficient']:
            # the 1e-6 threshold cannot flip: the null singular values are rounding, the last live one is not
            assert inf['n_live'] < L and inf['gap'] <= 1e-12 and 1.0 / inf['kappa'] >= 1e-3, (i, inf)
        else:
            assert inf['n_live'] == L, (i, inf)
        assert min(int((dummy[:, j] & tr).sum()) for j in range(J)) >= 3
        assert int(te.sum()) >= 3
        assert np.all(Y[te].std(axis=0) > 0.05)                          # no constant test column
        assert np.all(X[tr].std(axis=0) > 0.05)


def test_live_counts_of_the_rank_deficient_cases():
    assert {i['n_live'] for i in cx.expected('E12')[2]} == {32} and cx.expected('E12')[2][0]['L'] == 40
    assert {i['n_live'] for i in cx.expected('E13')[2]} == {11} and cx.expected('E13')[2][0]['L'] == 12


@pytest.mark.parametrize('name', cx.DEFICIENT)
def test_rank_deficient_cases_differ_from_the_literal_reference(name):
    """Why the oracle is not the yardstick there: it projects through the null vectors its SVD returns."""
    spec, X, Y, masks = cx.problem(name)
    r, r2, _ = cx.expected(name)
    with np.errstate(all='ignore'):
        lit_r, lit_r2 = ref.crossval(spec, X, Y, masks)
    diff = np.nanmax(np.abs(r - lit_r))
    print('{}: |expectation - literal reference| = {:.2f} in r'.format(name, diff))
    assert diff > 1e-2


def test_hand_built_masks():
    """E7: one cell without a test row, one with a single test row, one split inside one cell, one of three rows."""
    spec, X, Y, masks = cx.problem('E7')
    dummy = spec.dummy.astype(bool)
    n_test = np.array([[int((dummy[:, j] & ~masks[:, i]).sum()) for j in range(4)] for i in range(4)])
    assert n_test[0, 0] == 0 and np.all(n_test[0, 1:] >= 3)
    assert n_test[1, 1] == 1
    assert np.count_nonzero(n_test[2]) == 1 and n_test[2, 2] >= 3
    assert n_test[3].sum() == 3


def test_slices_of_the_wide_cases():
    """The derivation behind 'a cell straddles two slices' (the layout is not observable through the ABI)."""
    assert cx.slices_of(352, 352, 1) == [] and cx.slices_of(200, 100, 2) == []
    assert cx.slices_of(353, 353, 1) == [(0, 352, 0, 1), (352, 1, 0, 1)]
    assert cx.slices_of(360, 30, 12) == [(0, 352, 0, 12), (352, 8, 11, 1)]          # E10: cell 11 = rows 330 .. 359
    assert cx.slices_of(400, 100, 4) == [(0, 352, 0, 4), (352, 48, 3, 1)]           # E11: cell 3 = rows 300 .. 399


def test_perturbed_definitions_are_far_outside_the_tolerance():
    """What the per-entry 1e-7 separates: a z-map with ddof = 0 moves r2 by far more on the same data."""
    spec, X, Y, masks = cx.problem('E2')
    r, r2, _ = cx.expected('E2')
    mask = masks[:, 0]
    dummy = spec.dummy.astype(bool)
    R = ref.gen_covcorr(spec, X[mask], Y[mask], dummy[mask])
    U, d, V = ref.svd(R)
    pred = np.empty((int((~mask).sum()), Y.shape[1]))
    row = 0
    for j in range(dummy.shape[1]):
        tr, te = dummy[:, j] & mask, dummy[:, j] & ~mask
        z = (X[te] - X[tr].mean(axis=0)) / X[tr].std(axis=0, ddof=0)
        pred[row:row + len(z)] = z @ U @ V[j * 3:(j + 1) * 3].T + Y[tr].mean(axis=0)
        row += len(z)
    off = np.abs(ref.r2_score_raw(Y[~mask], pred) - r2[:, 0]).max()
    assert off > 1e3 * cx.TOL, off
