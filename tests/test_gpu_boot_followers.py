"""Every compiled variant of the bootstrap leg's follower kernels -- k_gram4 / k_gram / k_gram_lds, k_urot and
k_add_splits -- against the oracle, at small ragged shapes.

The bootstrap leg of a correlation-mode analysis is cross-product -> Gram pass -> small solve -> rotation.  The rotation
kernel is compiled once per k-step count ceil(T'/4) = 1..16 (with a 4x4x4 tail variant at 1, 5, 9, 13) plus two
generic variants, the Gram kernel once per row-block count 1..13, and the launch code picks 4- or 8-wave blocks and
cuts 64 or more bootstraps into resample splits whose partial sums k_add_splits adds.  Three sweeps walk them:

* A: T' = 4 n - 3 and 4 n for n = 1..16 at B = 1037 (13 live features in the last wave, one live wave in the last
  block, two column chunks of the Gram pass with a ragged second one), plus two shapes with L < T';
* B: resample splits at B = 1037 -- 97 bootstraps (3 splits of 33, 33, 31) at T' in {4, 20, 24, 50, 64, 80, 137},
  and 63 / 64 / 65 / 200 bootstraps at T' = 50;
* C: the 8-wave blocks at B = 65 613 (513 blocks, the last with 5 live waves), T' in {4, 20, 36, 50, 64}.

Every case pins the path it is written for from ``Engine.last_timing`` (include/plsx.h, plsx_last_timing [12..18]):
when a tuning change moves a threshold the case fails and names the key -- re-pin it, or add a shape that still takes
the path.  A few distinct bootstraps are spread over the slots (replica_expect.slot_map) with a different one on each
side of every split boundary; replicas agree among themselves at 1e-12, ``distrib`` of every slot with its oracle at
1e-9 per LV, sum U / sum U^2 with the replication-weighted oracle sums at 1e-8 per LV, permuted singular values at
1e-9 per permutation, the decomposition at 1e-9 (singular values) / 1e-7 (weights): the tolerances of
test_c4_bench_weak_step_replicated_against_oracle and test_crosscov_and_decompose_behavioral.

Data: replica_expect.synth (bench.py's), one group, one condition, correlation mode, S = 3 T' + 24, seed = T'.  The
oracle is conditioned far inside those tolerances at every shape (profiles/boot_followers_parity.txt has the
perturbation figures and the worst error of every case).  Each case prints its figures before it asserts.
"""
import json

import numpy as np
import pytest

from conftest import assert_close, assert_close_per_lv
from oracle import cpu_ref as ref
from replica_expect import slot_map, rel_per_column, assert_replicas, synth

pytestmark = pytest.mark.gpu

B_SMALL = 1037                  # 64 full waves + one of 13 features; 17 blocks of 4 waves, the last with one live wave
B_WIDE = 65613                  # 65 536 + 77: 4101 feature waves, 513 blocks of 8, the last with 5 live waves

RTOL_REPLICA, RTOL_DISTRIB, RTOL_SUMS, RTOL_PERM, RTOL_SV, RTOL_WEIGHTS = 1e-12, 1e-9, 1e-8, 1e-9, 1e-9, 1e-7
RTOL_TAIL, RTOL_GRAM16 = 1e-12, 1e-9        # test_bootstrap_kernel_variants_agree: tail vs no tail, gram4 vs gram16


def _assert_path(got, pinned, what):
    for key, want in pinned.items():
        assert got.get(key) == want, (
            'path moved: {} reports {} = {} where this test pins {} (full report: {}). The kernel variant this case '
            'is written for no longer runs at this shape: re-pin the case, or move it to a shape that still takes '
            'that path.'.format(what, key, got.get(key), want, got))


def _variant(nks):
    """urot_variant of the compiled-in k-step count nks with L = T': the tail variant exists at nks = 1, 5, 9, 13."""
    return nks + 100 if nks % 4 == 1 else nks


# ----------------------------------------------------------------------------------------------------------------
# one shape: data, engine, oracle
# ----------------------------------------------------------------------------------------------------------------

_ORACLE = {}                                # (T', B) -> (key of the original, {('boot' | 'perm', seed, i): oracle})


class _Shape(object):
    """The synthetic data of one (T', B) bound to a fresh engine, decomposed, with the engine's own decomposition
    (sign convention applied) as the original of both sides."""

    def __init__(self, Tp, B):
        from pypyls_amd import hostmath, resampling as rsmp
        from pypyls_amd.engine import Engine
        self.Tp, self.B, self.S = Tp, B, 3 * Tp + 24
        self.X, self.Y = synth(self.S, B, Tp, seed=Tp)
        self.spec = ref.Spec('behavioral', [self.S], 1)
        self.eng = Engine()
        self.eng.set_data(self.X, self.Y, rsmp.cell_of_row([self.S], 1), 1, 1, 0)
        assert self.eng.Tp == Tp and self.eng.L == min(Tp, B)
        self.raw = self.eng.decompose()
        self.tm_decompose = self.eng.last_timing()
        xw, sv, yw = self.raw
        self.xw, self.yw = hostmath.sign_convention(xw, yw)
        self.sv = sv
        self.eng.set_original(self.xw, self.sv, self.yw)
        self.eng.set_perm_path(False)                   # permutations through the feature pass: k_gram4<NB, 0, true>
        self.live = sv > 1e-4 * sv[0]
        key = (self.xw.tobytes(), self.sv.tobytes())
        if _ORACLE.get((Tp, B), (None,))[0] != key:
            if B >= B_WIDE:
                _ORACLE.clear()                         # (a wide shape's oracle sums are 34 MB each)
            _ORACLE[(Tp, B)] = (key, {})
        self.cache = _ORACLE[(Tp, B)][1]

    def close(self):
        self.eng.close()

    def samples(self, kind, n, seed):
        from pypyls_amd import resampling as rsmp
        gen = rsmp.gen_bootsamp if kind == 'boot' else rsmp.gen_permsamp
        return gen([self.S], 1, n, seed=seed, verbose=False)

    def oracle_boot(self, seed, i, inds):
        k = ('boot', seed, i)
        if k not in self.cache:
            self.cache[k] = ref.single_boot(self.spec, self.X, self.Y, inds, self.xw, np.diag(self.sv))
        return self.cache[k]

    def oracle_perm(self, seed, i, inds):
        k = ('perm', seed, i)
        if k not in self.cache:
            self.cache[k] = ref.single_perm(self.spec, self.X, self.Y, inds, self.yw)[0]
        return self.cache[k]

    def perm(self, perms):
        """-> permuted singular values (L, P) on the feature pass, last_timing()."""
        self.eng.set_timing(True)
        got = self.eng.perm(perms)
        tm = self.eng.last_timing()
        self.eng.set_timing(False)
        return got, tm

    def boot(self, boots):
        """-> sum U, sum U^2 (B, L), distrib (n, T', L), last_timing()."""
        self.eng.set_timing(True)
        usum, usq, dist = self.eng.boot(boots)
        tm = self.eng.last_timing()
        self.eng.set_timing(False)
        return usum.cpu().numpy(), usq.cpu().numpy(), np.moveaxis(dist, -1, 0), tm


def _try(failures, check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError as e:
        failures.append(str(e))


def _worst_per_lv(a, b, keep):
    a, b = np.asarray(a)[..., keep], np.asarray(b)[..., keep]
    axes = tuple(range(a.ndim - 1))
    return float(np.max(np.max(np.abs(a - b), axis=axes) / np.max(np.abs(b), axis=axes)))


def _check_decompose(sh, figs):
    """eng.decompose() (one resample through the Gram pass, the `out` branch of the rotation epilogue) against
    ref.decompose, as test_crosscov_and_decompose_behavioral does."""
    xw, sv, yw = sh.raw
    U, d, V = ref.decompose(sh.spec, sh.X, sh.Y)
    sgn = np.sign(np.sum(xw * U, axis=0))
    figs['decompose'] = dict(singvals=float(np.max(np.abs(sv - np.diag(d))) / np.max(np.diag(d))),
                             x_weights=float(np.max(np.abs(xw * sgn - U)) / np.max(np.abs(U))),
                             y_weights=float(np.max(np.abs(yw * sgn - V)) / np.max(np.abs(V))))
    failures = []
    _try(failures, assert_close, sv, np.diag(d), RTOL_SV, what='decompose singvals')
    _try(failures, assert_close, xw * sgn, U, RTOL_WEIGHTS, what='decompose x_weights (rotation, out branch)')
    _try(failures, assert_close, yw * sgn, V, RTOL_WEIGHTS, what='decompose y_weights')
    return failures


def _check_perm(sh, got, perms, seed, figs, label='perm'):
    """got (L, P) against the oracle of every permutation, per permutation column."""
    want = np.stack([sh.oracle_perm(seed, i, perms[:, i]) for i in range(perms.shape[1])], -1)
    rel = rel_per_column(got, want)
    figs[label] = float(rel.max())
    if np.all(rel <= RTOL_PERM):
        return []
    return ['permutation {} (feature pass) vs oracle: rel err {:.3e} > {:g}'.format(int(np.argmax(rel)), rel.max(),
                                                                                  RTOL_PERM)]


def _check_boot(sh, got, boots_d, seed, which, figs, label='boot'):
    """got = (sum U, sum U^2, distrib (n, T', L)) of the bootstraps boots_d[:, which]: replicas among themselves,
    every slot's distrib with its oracle, the sums with the replication-weighted oracle sums over the live LVs."""
    usum, usq, dist = got
    nd = boots_d.shape[1]
    failures = []
    _try(failures, assert_replicas, dist, which, RTOL_REPLICA, 'bootstrap distrib')
    want_us, want_uq = np.zeros_like(usum), np.zeros_like(usq)
    worst_rep = worst_dist = 0.0
    for d in range(nd):
        wd, wu = sh.oracle_boot(seed, d, boots_d[:, d])
        slots = np.flatnonzero(which == d)
        v = dist[slots]
        worst_rep = max(worst_rep, float(np.max(np.max(np.abs(v - v[:1]), axis=(0, 1)) / np.max(np.abs(v[0]), axis=0))))
        for slot in slots:
            worst_dist = max(worst_dist, _worst_per_lv(dist[slot], wd, slice(None)))
            _try(failures, assert_close_per_lv, dist[slot], wd, 1, RTOL_DISTRIB,
                 what='bootstrap {} distrib in slot {}'.format(d, slot))
        want_us += len(slots) * wu
        want_uq += len(slots) * wu ** 2
    figs[label] = dict(replicas=worst_rep, distrib=worst_dist, usum=_worst_per_lv(usum, want_us, sh.live),
                       usq=_worst_per_lv(usq, want_uq, sh.live))
    _try(failures, assert_close_per_lv, usum, want_us, 1, RTOL_SUMS, what='sum U', keep=sh.live)
    _try(failures, assert_close_per_lv, usq, want_uq, 1, RTOL_SUMS, what='sum U^2', keep=sh.live)
    return failures[:8]


def _check_equal_terms(usum, usq, n, figs):
    """n copies of ONE bootstrap: every element has |usum^2 - n usq| <= 4 (n + 32) 2^-53 n usq.  Each of the two sums
    is a recursive sum of n equal terms plus at most 32 split additions, so each carries a relative error of at most
    (n + 32) 2^-53; the square doubles that of the first, and squaring the term itself adds one rounding.  Fails when
    a resample enters one sum and not the other, or a replica was rotated with a corrupted operand."""
    a, q = usum.astype(np.longdouble), usq.astype(np.longdouble)
    dev = np.abs(a * a - n * q)
    bound = 4.0 * (n + 32) * 2.0 ** -53 * n * q
    with np.errstate(divide='ignore', invalid='ignore'):
        figs['equal_terms_over_bound'] = float(np.max(np.where(q > 0, dev / bound, np.where(dev > 0, np.inf, 0.0))))
    bad = dev > bound
    if not np.any(bad):
        return []
    b, l = np.unravel_index(int(np.argmax(np.where(bad, dev / np.maximum(bound, 1e-300), 0))), bad.shape)
    return ['{} copies of one bootstrap: |usum^2 - n usq| = {:.3e} > bound {:.3e} at feature {}, LV {} ({} elements '
            'above the bound)'.format(n, float(dev[b, l]), float(bound[b, l]), b, l, int(bad.sum()))]


def _slots(n, nd, bounds, seed):
    """slot_map of the first seed from `seed` on whose draw meets its conditions (with a dozen slots a draw can end
    on the resample it began with)."""
    for k in range(50):
        try:
            return slot_map(n, nd, bounds, seed + 7919 * k)
        except AssertionError as e:
            if str(e):                                  # a boundary assertion of slot_map (it names the boundary): a bug
                raise
    raise AssertionError('no slot map of {} slots over {} resamples with boundaries {}'.format(n, nd, bounds))


def _report(case, figs):
    print('boot_followers_parity ' + json.dumps(dict(case=case, **figs), sort_keys=True))


# ----------------------------------------------------------------------------------------------------------------
# the case runner
# ----------------------------------------------------------------------------------------------------------------

def _run_case(case, Tp, B, n, nd, urot, gram_perm, gram_boot, full=True, front=True, routes=False):
    """One shape and one bootstrap count.

    urot: the pinned rotation path of the bootstrap launch (urot_variant, urot_variant_last, urot_waves, urot_splits,
    urot_res_per_split); gram_perm / gram_boot: the pinned Gram pass of the permutation / bootstrap leg (gram_kernel,
    gram_chunks; gram_chunks left out: more than one).  front: decomposition and 4 permutations too.  full (L = T'):
    the decomposition is compared as well.  routes: the bootstraps (and permutations) again with urot_generic and with
    no_gram4, compared with the default route.  n > 12: the geometry is read back from n copies of one bootstrap
    first, and the slot map gets a boundary at every multiple of the reported resamples per split."""
    sh = _Shape(Tp, B)
    figs, failures = {}, []
    try:
        variant_keys = {k: urot[k] for k in ('urot_variant', 'urot_variant_last', 'urot_waves')}

        def assert_gram(tm, pinned, what):
            _assert_path(tm, pinned, what)
            if 'gram_chunks' not in pinned:
                assert tm.get('gram_chunks', 0) > 1, 'path moved: {} reports gram_chunks = {} where this test needs ' \
                    'more than one column chunk (full report: {})'.format(what, tm.get('gram_chunks'), tm)

        if front:
            # decomposition: one resample, the rotation writes U itself
            _assert_path(sh.tm_decompose, dict(variant_keys, urot_splits=1, urot_res_per_split=1),
                         '{} decompose (rotation)'.format(case))
            assert_gram(sh.tm_decompose, gram_perm, '{} decompose (Gram pass)'.format(case))
            if full:
                failures += _check_decompose(sh, figs)
            perms = sh.samples('perm', 4, 1000 + Tp)
            got_p, tm = sh.perm(perms)
            _assert_path(tm, dict(dual_perm=0), '{} permutation leg'.format(case))
            assert_gram(tm, gram_perm, '{} permutation leg (Gram pass)'.format(case))
            failures += _check_perm(sh, got_p, perms, 1000 + Tp, figs)
        boots_d = sh.samples('boot', nd, 2000 + Tp)
        bounds = []
        if n > 12:
            # the geometry, read back from n copies of bootstrap 0 (and the equal-terms bound on their sums)
            usum, usq, dist, tm = sh.boot(boots_d[:, np.zeros(n, int)])
            _assert_path(tm, dict(urot, xprod_launches=1, xprod_resamples=n), '{} bootstrap leg ({} copies)'.format(case, n))
            assert (tm['urot_splits'] > 1) == (n >= 64), tm
            assert_gram(tm, gram_boot, '{} bootstrap leg (Gram pass)'.format(case))
            failures += _check_equal_terms(usum, usq, n, figs)
            _try(failures, assert_replicas, dist, np.zeros(n, int), RTOL_REPLICA,
                 '{} copies of one bootstrap: distrib'.format(n))
            rps = int(tm['urot_res_per_split'])
            bounds = list(range(rps, n, rps))
            assert len(bounds) == int(tm['urot_splits']) - 1, (bounds, tm)
        which = _slots(n, nd, bounds, seed=3000 + Tp + n)
        got_b = sh.boot(boots_d[:, which])
        # (one launch: the engine did not cut the submission, so the splits are those of all n bootstraps)
        _assert_path(got_b[3], dict(urot, xprod_launches=1, xprod_resamples=n), '{} bootstrap leg'.format(case))
        assert_gram(got_b[3], gram_boot, '{} bootstrap leg (Gram pass)'.format(case))
        default_failures = _check_boot(sh, got_b[:3], boots_d, 2000 + Tp, which, figs)
        if routes:
            verdict = {}
            for route, rtol, kernel in (('urot_generic', RTOL_TAIL, 'k_urot compiled-in variant vs generic'),
                                        ('no_gram4', RTOL_GRAM16, 'k_gram4 vs k_gram (16x16x4)')):
                sh.eng.set_option(route, 1)
                alt = sh.boot(boots_d[:, which])
                if route == 'urot_generic':
                    assert alt[3]['urot_variant'] in (0, -1), 'option urot_generic left the compiled-in variant on: ' \
                        '{}'.format(alt[3])
                else:
                    assert alt[3]['gram_kernel'] == 0, 'option no_gram4 left k_gram4 on: {}'.format(alt[3])
                    if front:
                        alt_p, tm = sh.perm(perms)
                        assert tm['gram_kernel'] == 0, tm
                        figs['perm_vs_' + route] = float(np.max(np.abs(alt_p - got_p)) / np.max(np.abs(got_p)))
                        _try(failures, assert_close, got_p, alt_p, rtol, what='permutations: ' + kernel)
                sh.eng.set_option(route, 0)
                figs['boot_vs_' + route] = max(float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
                                               for a, b in zip(got_b[:3], alt[:3]))
                for name, a, b in zip(('sum U', 'sum U^2', 'distrib'), got_b[:3], alt[:3]):
                    _try(failures, assert_close, a, b, rtol, what='{}: {} disagree'.format(name, kernel))
                verdict[route] = _check_boot(sh, alt[:3], boots_d, 2000 + Tp, which, {}, label=route)
            if default_failures:
                # which kernel is off: the route that replaces it agrees with the oracle where the default does not
                default_failures.append('independent routes against the oracle: ' + '; '.join(
                    '{} {}'.format(r, 'FAILS too' if f else 'passes (so the kernel it replaces is the one that is off)')
                    for r, f in verdict.items()))
        failures += default_failures
    finally:
        sh.close()
        _report(case, figs)
    assert not failures, '{}:\n  '.format(case) + '\n  '.join(failures)


# ----------------------------------------------------------------------------------------------------------------
# sweep A: every k-step count, small and ragged
# ----------------------------------------------------------------------------------------------------------------

SWEEP_A = [tp for n in range(1, 17) for tp in (4 * n - 3, 4 * n)]


@pytest.mark.parametrize('Tp', SWEEP_A)
def test_every_k_step_count(Tp):
    """T' = 4 n - 3 (one live row in the last k-step) and 4 n (four), n = 1..16, L = T', B = 1037: k_urot<., n> --
    with the 4x4x4 tail at n in {1, 5, 9, 13}, where the tail tile holds 1 and 4 live columns -- behind
    k_gram4<n, n, true> (n <= 13) or k_gram, and k_gram4<n, 0, true> on the permutation leg; two column chunks.
    12 slots of 4 distinct bootstraps, 4 permutations, the decomposition; again with urot_generic and no_gram4."""
    nks = (Tp + 3) // 4
    urot = dict(urot_variant=_variant(nks), urot_variant_last=_variant(nks), urot_waves=4, urot_splits=1,
                urot_res_per_split=12)
    gram = dict(gram_kernel=nks if nks <= 13 else 0, gram_chunks=2)
    _run_case("sweep A T'={} B={}".format(Tp, B_SMALL), Tp, B_SMALL, 12, 4, urot, gram, gram, routes=True)


def test_tail_columns_on_a_count_without_tail_variant():
    """T' = 24, B = 20: L = 20, so the last of the two L tiles holds 4 live columns (the tail rule) on a k-step count,
    6, that has no tail instantiation: k_urot<2, 6> multiplies it on the 16x16x4 shape.  L != T' also takes the
    bootstrap's Gram pass off k_gram4 (ceil(L / 4) != ceil(T' / 4)).  With L < T' the trailing LVs depend on null
    vectors: permutations and distrib, and the sums over the LVs with sv > 1e-4 sv[0]."""
    urot = dict(urot_variant=6, urot_variant_last=6, urot_waves=4, urot_splits=1, urot_res_per_split=12)
    _run_case("sweep A T'=24 B=20", 24, 20, 12, 4, urot, dict(gram_kernel=6, gram_chunks=1),
              dict(gram_kernel=0, gram_chunks=1), full=False, routes=True)


def test_generic_variant_below_the_compiled_in_limit():
    """T' = 50, B = 37: L = 37 is 3 tiles where 13 k-steps would make 4, so the generic variant (whole operand in
    LDS) runs at a T' <= 64.  Compared as the other L < T' shape."""
    urot = dict(urot_variant=0, urot_variant_last=0, urot_waves=4, urot_splits=1, urot_res_per_split=12)
    _run_case("sweep A T'=50 B=37", 50, 37, 12, 4, urot, dict(gram_kernel=13, gram_chunks=1),
              dict(gram_kernel=0, gram_chunks=1), full=False, routes=True)


# ----------------------------------------------------------------------------------------------------------------
# sweep B: resample splits at small B
# ----------------------------------------------------------------------------------------------------------------

# T' -> (urot_variant of the first chunk of L tiles, of the last, gram_kernel)
SWEEP_B_PATH = {4: (101, 101, 1), 20: (105, 105, 5), 24: (6, 6, 6), 50: (113, 113, 13), 64: (16, 16, 0),
                80: (0, 0, -1),           # 20 k-steps, 5 L tiles: generic, whole operand in LDS (NKS == 0)
                137: (-1, 0, -1)}         # 35 k-steps, L tiles 6 + 3: staged in two pieces of 20 + 15 (NKS < 0), then whole
# bootstraps of one submission -> (splits, resamples per split): min(32, n // 32) splits while the 17 feature blocks
# leave the chip unfilled; 97 -> 33 + 33 + 31, 64 -> 32 + 32, 65 -> 33 + 32, 200 -> 5 x 34 + 30
SPLITS = {63: (1, 63), 64: (2, 32), 65: (2, 33), 97: (3, 33), 200: (6, 34)}
SWEEP_B = [(4, 97), (20, 97), (24, 97), (50, 63), (50, 64), (50, 65), (50, 97), (50, 200), (64, 97), (80, 97),
           (137, 97)]


@pytest.mark.parametrize('Tp,n', SWEEP_B)
def test_resample_splits(Tp, n):
    """n bootstraps in ONE launch (pinned: xprod_launches = 1) built from 5 distinct ones, a different one on each
    side of every split boundary and in the first and last slot: a partial sum written to the wrong split, a split
    that starts one resample early or late, an LDS stage of resample r multiplied with the fragments of r + 1,
    k_add_splits dropping or doubling a split.  First n copies of one bootstrap: the geometry read back, and the
    equal-terms bound on the sums (_check_equal_terms).  n = 63: the same without splits."""
    first, last, gk = SWEEP_B_PATH[Tp]
    splits, rps = SPLITS[n]
    urot = dict(urot_variant=first, urot_variant_last=last, urot_waves=4, urot_splits=splits, urot_res_per_split=rps)
    gram = dict(gram_kernel=gk, gram_chunks=2)
    _run_case("sweep B T'={} n={}".format(Tp, n), Tp, B_SMALL, n, 5, urot, gram, gram, front=(n == 97))


# ----------------------------------------------------------------------------------------------------------------
# sweep C: the 8-wave blocks away from the headline shape
# ----------------------------------------------------------------------------------------------------------------

# T' -> (urot_variant, gram_kernel, gram_chunks of 12 or fewer resamples: 128 chunks asked, columns rounded up to 8 / 16)
SWEEP_C_PATH = {4: (101, 1, 127), 20: (105, 5, 127), 36: (109, 9, 127), 50: (113, 13, 127), 64: (16, 0, 125)}
SWEEP_C = [(4, 12), (20, 12), (36, 12), (50, 12), (50, 70), (64, 12)]


@pytest.mark.parametrize('Tp,n', SWEEP_C)
def test_eight_wave_blocks(Tp, n):
    """B = 65 613: the compiled-in variants run 8 waves a block (B >= 65 536), 513 blocks, the last with 5 live and 3
    idle waves and 13 live features in its last live wave.  12 slots of 4 distinct bootstraps; at T' = 50 also 70
    bootstraps in 2 splits of 35 on those blocks."""
    variant, gk, chunks = SWEEP_C_PATH[Tp]
    splits, rps = (2, 35) if n == 70 else (1, n)
    urot = dict(urot_variant=variant, urot_variant_last=variant, urot_waves=8, urot_splits=splits,
                urot_res_per_split=rps)
    gram = dict(gram_kernel=gk, gram_chunks=chunks)
    gram_boot = dict(gram_kernel=gk) if n == 70 else gram        # (18 blocks of 4: the chunk count follows the chip)
    _run_case("sweep C T'={} n={}".format(Tp, n), Tp, B_WIDE, n, 4, urot, gram, gram_boot, front=(n == 12))
