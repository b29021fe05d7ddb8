"""
Front-ends ``behavioral_pls`` / ``meancentered_pls`` with the keyword surface
and ``PLSResults`` layout of the reference (pyls/types/behavioral.py:231-242,
pyls/types/meancentered.py:182-192), driving the MI355X engine, and
``multiblock_pls`` (no counterpart in the reference: both blocks in one
decomposition, on the same driver).

Host code here mirrors the ORCHESTRATION of BasePLS.run_pls
(pyls/base.py:341-399) and the subclass ``run_pls`` bodies; every
per-resample computation (gather/permute, z-score, cross-product, SVD,
Procrustes, accumulation) runs on the device through the C ABI of
include/plsx.h.  There is no CPU fallback.

Differences from the reference at this commit, on purpose:
  * ``permindices`` defaults to True, the documented default
    (pyls/structures.py:115-120); the shipped ``None`` makes
    BasePLS._single_perm treat index vectors as data.
  * ``n_proc`` counts GPUs, not CPU workers: the joblib pool of the reference
    (pyls/utils.py:252-279) is what the devices replace.  ``n_proc=8`` (or
    'max' / -1) on an 8-GPU node shards the resamples of THIS call over the
    GPUs from this one process -- one context and one host thread per device,
    ONE all-gather (pypyls_amd/team.py); ``device_ids=[...]`` names them
    explicitly.  On a one-GPU box both reduce to the ordinary call.
  * When torch.distributed is initialised (a script under torchrun: one
    process per GPU) the resamples are sharded across the RANKS instead and
    collected with one all-gather (pypyls_amd/parallel.py); ``n_proc`` /
    ``device_ids`` are then ignored.
"""
import warnings

import numpy as np

from . import hostmath, parallel, resampling
from .structures import PLSInputs, PLSResults

_METHOD_CODE = {'behavioral': 0, 'meancentered': 1, 'multiblock': 3}

# The B- and n_boot-sized result arrays (x_weights, bootstrap ratios / standard errors, the (T', L, n_boot)
# distributions: 440 MB at the headline shape) LAND in page-locked memory (57 GB/s instead of 8 - 10 pageable) that is
# mapped while the device resamples.  PLSResults holds ordinary numpy arrays, like the reference's: they are copied out
# of the page-locked landing zone by a few host threads (a memcpy releases the GIL; 440 MB in ~10 ms, one thread needs
# 55) and the landing zone is released with the call -- a caller that keeps many results (sweeps, per-subject loops)
# does not accumulate unswappable memory.  ``COPY_RESULTS_OUT_OF_PINNED = False`` hands out views of the
# page-locked memory instead (no second pass; that memory then stays locked for as long as the results live).
COPY_RESULTS_OUT_OF_PINNED = True
_COPY_THREADS = 8
_COPY_POOL = None


def _host_array(t):
    a = t.numpy()
    if not COPY_RESULTS_OUT_OF_PINNED:
        return a
    out = np.empty_like(a)
    n = a.size
    if n * a.itemsize < (8 << 20) or not a.flags.c_contiguous:
        np.copyto(out, a)
        return out
    global _COPY_POOL
    if _COPY_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _COPY_POOL = ThreadPoolExecutor(max_workers=_COPY_THREADS, thread_name_prefix='plsx-copy')
    src, dst = a.reshape(-1), out.reshape(-1)
    step = -(-n // _COPY_THREADS)
    list(_COPY_POOL.map(lambda lo: np.copyto(dst[lo:lo + step], src[lo:lo + step]), range(0, n, step)))
    return out


def _as_float_array(A, name):
    A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError('Expected 2D array for `{}`, got {}D array instead'.format(name, A.ndim))
    return A.astype(np.float64, copy=False)


def _check_finite(A, name):
    if not np.all(np.isfinite(A)):
        raise ValueError('Input `{}` contains NaN, infinity or a value too large'.format(name))


def _check_contrasts(contrasts, Tp, B, n_split):
    """Non-rotated PLS: the caller's contrasts (T', Lc) -> V = normalize(contrasts), checked on the host before any
    engine is created or looked up."""
    C = np.asarray(contrasts)
    if C.ndim != 2:
        raise ValueError('Expected 2D array for `contrasts`, got {}D array instead'.format(C.ndim))
    C = C.astype(np.float64)
    if C.shape[0] != Tp:
        raise ValueError('Provided `contrasts` must have one row per row of the cross-covariance matrix (groups x '
                         'conditions, x behaviours for behavioral PLS).\n    EXPECTED: {}\n    ACTUAL:   {}'
                         .format(Tp, C.shape[0]))
    if not 1 <= C.shape[1] <= min(Tp, B):
        raise ValueError('Provided `contrasts` must have between 1 and min(T\', B) = {} columns; got {}'
                         .format(min(Tp, B), C.shape[1]))
    if not np.all(np.isfinite(C)):
        raise ValueError('Input `contrasts` contains NaN, infinity or a value too large')
    norms = np.sqrt((C ** 2).sum(axis=0))
    if np.any(norms == 0):
        raise ValueError('Provided `contrasts` has a column of zeros (column {})'.format(int(np.argmin(norms != 0))))
    if n_split:
        raise ValueError('Split-half resampling (`n_split` > 0) is not available for non-rotated PLS (`contrasts`)')
    V = C / norms
    if np.abs(V.T @ V - np.eye(V.shape[1])).max() > 1e-8:
        warnings.warn('Provided `contrasts` are not orthogonal: the effects are not independent and `varexp` is not '
                      'a partition of the covariance.', stacklevel=4)
    return V


def _check_weights_ci(weights_ci, method, L, n_boot, bootsamples, contrasts):
    """What ``weights_ci`` does not cover, refused on the host before any engine is created or looked up -> the number
    of latent variables m (True: all L)."""
    if method == 'multiblock':
        raise ValueError('Percentile intervals of the x_weights (`weights_ci`) are not available for multiblock PLS')
    if contrasts:
        raise ValueError('Percentile intervals of the x_weights (`weights_ci`) are not available for non-rotated PLS '
                         '(`contrasts`)')
    n_boot = n_boot or 0
    if n_boot > 0 and bootsamples is not None and np.ndim(bootsamples) == 2:
        n_boot = np.shape(bootsamples)[1]
    if n_boot < 1:
        raise ValueError('`weights_ci` needs bootstraps (`n_boot` > 0)')
    if n_boot > 16384:
        raise ValueError('`weights_ci` takes at most 16384 bootstraps (the bound of the selection kernels); got '
                         '`n_boot` = {}'.format(n_boot))
    if weights_ci is True:
        return L
    if isinstance(weights_ci, (bool, np.bool_)) or not isinstance(weights_ci, (int, np.integer)) \
            or not 1 <= int(weights_ci) <= L:
        raise ValueError('`weights_ci` must be True or a number of latent variables in 1 .. {}; got {!r}'
                         .format(L, weights_ci))
    return int(weights_ci)


def _check_weights_perm(weights_perm, method, L, n_perm, permsamples, permindices):
    """What ``weights_perm`` does not cover, refused on the host before any engine is created or looked up -> the number
    of latent variables m (True: all L; with ``contrasts`` L is their number)."""
    if method == 'multiblock':
        raise ValueError('Permutation p-values of the x_weights (`weights_perm`) are not available for multiblock PLS')
    if not permindices:
        raise ValueError('`weights_perm` cannot be combined with `permindices=False`: the test rebuilds every permutation '
                         'from its index row, pre-permuted Y matrices have none')
    n_perm = n_perm or 0
    if n_perm > 0 and permsamples is not None and np.ndim(permsamples) == 2:
        n_perm = np.shape(permsamples)[1]
    if n_perm < 1:
        raise ValueError('`weights_perm` needs permutations (`n_perm` > 0)')
    if weights_perm is True:
        return L
    if isinstance(weights_perm, (bool, np.bool_)) or not isinstance(weights_perm, (int, np.integer)) \
            or not 1 <= int(weights_perm) <= L:
        raise ValueError('`weights_perm` must be True or a number of latent variables in 1 .. {}; got {!r}'
                         .format(L, weights_perm))
    return int(weights_perm)


def _weights_perm_pvals(obs, count, wmax):
    """The three arrays ``weights_perm`` adds to permres.  obs (B, m) = |Z| / s_f, the observed side of the family-wise
    comparison; count (B, m) = #{p : |Z_p| >= |Z|}; wmax (m, n_perm) = max_f |Z_p[f, l]| / s_f.  The maxT p-value counts,
    per latent variable, the maxima at or above the observed scaled magnitude: one sort and one searchsorted each."""
    n_perm = wmax.shape[1]
    fwe = np.empty(obs.shape)
    for l in range(obs.shape[1]):
        null = np.sort(wmax[l])
        fwe[:, l] = (n_perm - np.searchsorted(null, obs[:, l], side='left') + 1) / (n_perm + 1)
    return dict(x_weights_pvals=(count + 1) / (n_perm + 1), x_weights_max=wmax, x_weights_pvals_fwe=fwe)


def _check_confounds(confounds, X, permindices, cvsplits=None):
    """The checks of ``behavioral_pls(confounds=)``, on the host before any engine is created or looked up (wording of
    ``pls_regression``) -> dict(Z (S, q) float64, Zt = [1, Z - zbar] (S, q + 1), zmean (q,))."""
    S = len(X)
    Zc = np.asarray(confounds)
    if Zc.ndim == 1:
        Zc = Zc[:, None]
    if Zc.ndim != 2 or len(Zc) != S or Zc.shape[1] < 1 or not (np.issubdtype(Zc.dtype, np.number) or Zc.dtype == bool):
        raise ValueError('Provided `confounds` must be numeric with shape (S, q) or (S,), S = {}; got {}'
                         .format(S, np.shape(confounds)))
    if Zc.shape[1] > 15:
        raise ValueError('Provided `confounds` can have at most 15 columns; got {}'.format(Zc.shape[1]))
    Zc = np.ascontiguousarray(Zc, dtype=np.float64)
    if not np.isfinite(Zc).all():
        raise ValueError('Provided `confounds` must be finite; row {} is not'
                         .format(int(np.flatnonzero(~np.isfinite(Zc).all(axis=1))[0])))
    if not permindices:
        raise ValueError('`confounds` cannot be combined with `permindices=False`: pre-permuted Y matrices are not '
                         'residualised')
    zmean = Zc.mean(axis=0)
    Zt = np.c_[np.ones(S), Zc - zmean]
    if np.linalg.matrix_rank(Zt) < Zt.shape[1]:
        raise ValueError('Provided `confounds` are rank deficient together with the intercept on the {} rows'.format(S))
    cf = dict(Z=Zc, Zt=Zt, zmean=zmean)
    if cvsplits is not None and np.ndim(cvsplits) == 2 and np.shape(cvsplits)[0] == S:
        _check_cvrank(cf, np.asarray(cvsplits, dtype=bool))
    return cf


def _check_cvrank(cf, masks):
    """The confounds must have full column rank, together with the intercept, on the training rows of every split."""
    Zt = cf['Zt']
    for s in range(masks.shape[1]):
        tr = masks[:, s]
        if np.linalg.matrix_rank(Zt[tr]) < Zt.shape[1]:
            raise ValueError('Provided `confounds` are rank deficient together with the intercept on the {} training '
                             'rows of split {}'.format(int(tr.sum()), s))


def _refuse_confounds(kwargs, what):
    """``confounds`` belongs to behavioral_pls (and pls_regression): refused on the host, before any engine."""
    if kwargs.get('confounds') is not None:
        raise ValueError('`confounds` (the confound regression) is not available for {}: residualise the data before '
                         'the call, or use behavioral PLS'.format(what))
    kwargs.pop('confounds', None)


class _PLSCRun(object):
    """One analysis; the counterpart of BasePLS + subclass (pyls/base.py:232)."""

    def __init__(self, method, X, Y=None, groups=None, n_cond=1, **kwargs):
        self.method = method
        if groups is None:
            groups = [len(X) // n_cond]
        elif not isinstance(groups, (list, np.ndarray)):
            groups = [groups]
        groups = [int(g) for g in groups]
        # pyls/base.py:265-277
        n_samples = sum(g * n_cond for g in groups)
        if len(X) != n_samples:
            raise ValueError('Number of samples specified by `groups` and `n_cond` does not '
                             'match number of samples in input array(s).\n'
                             '    EXPECTED: {}\n    ACTUAL:   {} (groups: {} * n_cond: {})'
                             .format(len(X), n_samples, groups, n_cond))
        if Y is not None and len(X) != len(Y):
            raise ValueError('Provided `X` and `Y` matrices must have the same number of '
                             'samples. Provided matrices differed: X: {}, Y: {}'
                             .format(len(X), len(Y)))
        kwargs.setdefault('permindices', True)
        # non-rotated PLS: V = normalize(contrasts) (T', Lc), or None
        self.V = None
        if kwargs.get('contrasts') is not None:
            Xa, Ya = np.asarray(X), (None if Y is None else np.asarray(Y))
            if Xa.ndim != 2 or (Ya is not None and Ya.ndim != 2):
                raise ValueError('Expected 2D arrays for `X` and `Y`')
            Tp = len(groups) * n_cond * (Ya.shape[1] if Ya is not None else 1)
            self.V = _check_contrasts(kwargs['contrasts'], Tp, Xa.shape[1], kwargs.get('n_split'))
            kwargs['contrasts'] = np.asarray(kwargs['contrasts'], dtype=np.float64)
        else:
            kwargs.pop('contrasts', None)
        # weights_ci: LVs whose rotated bootstrap weights get percentile intervals (None: not asked for)
        self.weights_m = None
        if kwargs.get('weights_ci', False) is not False and kwargs.get('weights_ci') is not None:
            Xa = np.asarray(X)
            T = 1 if Y is None else (np.asarray(Y).shape[1] if np.asarray(Y).ndim == 2 else 0)
            if Xa.ndim != 2 or T < 1:
                raise ValueError('Expected 2D arrays for `X` and `Y`')
            self.weights_m = _check_weights_ci(kwargs['weights_ci'], method, min(len(groups) * n_cond * T, Xa.shape[1]),
                                               kwargs.get('n_boot'), kwargs.get('bootsamples'), self.V is not None)
        else:
            kwargs.pop('weights_ci', None)
        # weights_perm: LVs whose weights are tested against the permutations (None: not asked for)
        self.wperm_m = None
        if kwargs.get('weights_perm', False) is not False and kwargs.get('weights_perm') is not None:
            Xa = np.asarray(X)
            T = 1 if Y is None else (np.asarray(Y).shape[1] if np.asarray(Y).ndim == 2 else 0)
            if Xa.ndim != 2 or T < 1:
                raise ValueError('Expected 2D arrays for `X` and `Y`')
            L = self.V.shape[1] if self.V is not None else min(len(groups) * n_cond * T, Xa.shape[1])
            self.wperm_m = _check_weights_perm(kwargs['weights_perm'], method, L, kwargs.get('n_perm'),
                                               kwargs.get('permsamples'), kwargs.get('permindices'))
        else:
            kwargs.pop('weights_perm', None)
        # measurement hooks of bench.py --mode analysis (not inputs of the analysis): a dict that receives
        # per-phase wall times; (rank, world) of a world emulated on one GPU
        self.cvperm_given = kwargs.pop('_cvpermsamples', None)     # behavioral_pls(cv_perm=): validated (S, P) or None
        self.cv_lv_m = kwargs.pop('_cv_lv_m', None)                # behavioral_pls(cv_lv=): validated LV count or None
        self.cf = kwargs.pop('_confounds', None)                   # behavioral_pls(confounds=): validated dict or None
        self.phases = kwargs.pop('_phases', None)
        self.emulate = kwargs.pop('_emulate', None)
        self.device_ids = kwargs.pop('device_ids', None)
        self.transport = kwargs.pop('_transport', 'auto')
        if method == 'multiblock':
            kwargs['method'] = method                  # (the two reference front-ends record none)
        self.inputs = PLSInputs(X=X, Y=Y, groups=groups, n_cond=n_cond, **kwargs)
        # under torch.distributed every rank must draw the same index arrays
        self.rs = resampling.check_random_state(parallel.shared_seed(self.inputs.get('seed')))
        self.cells = resampling.cell_of_row(groups, n_cond)
        self.n_cells = len(groups) * n_cond
        self.engine = kwargs.get('_engine')

    # ------------------------------------------------------------------
    def _plan_draws(self, L):
        """Everything the analysis draws from ``self.rs``, in the reference's order
        (BasePLS.run_pls, base.py:362-397; crossval after the bootstrap,
        behavioral.py:219-221), as jobs of ONE host thread that starts before the
        data goes to the device: the SVD's seed matrix, the permutation arrays, the
        split masks of the original data, the bootstrap arrays, the cross-validation
        splits.  Only the ORDER of consumption is pinned by a seed; the device takes
        finished rows while later ones are still drawn (resampling.IndexStream)."""
        inp = self.inputs
        S = self.cells.size
        # the reference's randomized_svd consumes normal((L, L + 10)) from self.rs for the
        # original decomposition; draw it so that later index arrays match for a seed
        jobs = [lambda rs: rs.normal(size=(L, L + 10))]
        self.perm_stream = self.boot_stream = self.ystack = None
        self.orig_splits = self.cv_splits = None
        n_perm = inp.get('n_perm') or 0
        n_boot = inp.get('n_boot') or 0
        from .engine import check_index_array
        if n_perm > 0:
            # BasePLS.permutation, base.py:601-652
            permsamp = inp.get('permsamples')
            if permsamp is None:
                self.perm_stream = resampling.IndexStream('perm', inp.groups, inp.n_cond, n_perm)
                jobs.append(self.perm_stream.draw)
            elif not inp.get('permindices'):
                # pre-permuted Y matrices, (n_perm, S, T) (base.py:636-639)
                permsamp = np.asarray(permsamp)
                if self.method != 'behavioral' or permsamp.ndim != 3:
                    raise ValueError('permindices=False expects `permsamples` of shape '
                                     '(n_perm, S, T) and behavioral PLS')
                self.ystack = permsamp.astype(np.float64, copy=False)
            else:
                permsamp = np.asarray(permsamp)
                if permsamp.ndim != 2 or permsamp.shape[0] != S:
                    raise ValueError('resampling array must have shape (S, n) with S = {}; got {}'
                                     .format(S, permsamp.shape))
                self.perm_stream = resampling.IndexStream.of_array(check_index_array(permsamp, S))
                self.perm_given = permsamp
        n_split = inp.get('n_split')
        if (self.perm_stream is not None or self.ystack is not None) and n_split is not None:
            # the reference draws the split masks of the ORIGINAL data from self.rs after the
            # permutation arrays and before the bootstrap arrays (base.py:373-380); permutation
            # i uses a fresh RandomState(i) (base.py:705-708, 738-742)
            self.orig_splits = inp.get('_splitsamples')
            if self.orig_splits is None:
                jobs.append(lambda rs: setattr(self, 'orig_splits', resampling.gen_splits(
                    inp.groups, inp.n_cond, n_split, seed=rs, test_size=0.5)))
        if n_boot > 0:
            # BasePLS.bootstrap, base.py:439-528 (index arrays drawn AFTER the permutation
            # arrays, as in the reference's run_pls order)
            bootsamp = inp.get('bootsamples')
            if bootsamp is None:
                self.boot_stream = resampling.IndexStream('boot', inp.groups, inp.n_cond, n_boot)
                jobs.append(self.boot_stream.draw)
            else:
                bootsamp = np.asarray(bootsamp)
                if bootsamp.ndim != 2 or bootsamp.shape[0] != S:
                    raise ValueError('resampling array must have shape (S, n) with S = {}; got {}'
                                     .format(S, bootsamp.shape))
                self.boot_stream = resampling.IndexStream.of_array(check_index_array(bootsamp, S))
                self.boot_given = bootsamp
        if (self.method == 'behavioral' and inp.get('test_split') is not None
                and (inp.get('test_size') or 0) > 0 and self.V is None):
            # (non-rotated PLS: no fitted decomposition to predict from -- the masks came last, nothing else moves)
            # behavioral.py:219-221, 82-170
            self.cv_splits = inp.get('_cvsplits')
            if self.cv_splits is None:
                jobs.append(lambda rs: setattr(self, 'cv_splits', resampling.gen_splits(
                    inp.groups, inp.n_cond, inp.test_split, seed=rs, test_size=inp.test_size)))
        # cv_perm: the permutations of the cross-validation come after everything else a seeded call draws, the masks
        # included -- every other array of the call keeps its bits
        self.cvperm_stream = None
        if (inp.get('cv_perm') or 0) > 0:
            if self.cvperm_given is not None:
                self.cvperm_stream = resampling.IndexStream.of_array(self.cvperm_given)
            else:
                self.cvperm_stream = resampling.IndexStream('perm', inp.groups, inp.n_cond, int(inp.get('cv_perm')))
                jobs.append(self.cvperm_stream.draw)
        return resampling.DrawThread(self.rs, jobs)

    def run(self):
        import torch
        from .engine import Engine
        inp = self.inputs
        X = _as_float_array(inp.X, 'X')
        Y = None if self.method == 'meancentered' else _as_float_array(inp.Y, 'Y')
        Tp = self.n_cells * Y.shape[1] if Y is not None else self.n_cells
        if self.method == 'multiblock':
            Tp += self.n_cells                         # the task rows come first
        self.perm_given = self.boot_given = None
        from .engine import default_engine, touch_idle_release
        from . import team as _team
        touch_idle_release()                           # (a pending idle release is pushed back before the engine is looked up)
        devices = None
        if self.engine is None and self.emulate is None and parallel._dist() is None:
            # n_proc workers of the reference (pyls/utils.py:252-279) = GPUs of this node, driven from this process
            devices = _team.resolve_devices(inp.get('n_proc'), self.device_ids)
        self._mstreams = []
        self.team = None
        if devices is not None and len(devices) > 1:
            self.team = _team.team_for(devices, self.transport)
        elif devices is not None:
            self.engine = default_engine(devices[0])
        draws = self._plan_draws(min(Tp, X.shape[1])).start()
        try:
            unrefined = 0
            if self.team is not None:
                # one host thread per device; the draws above are shared (drawn ONCE for all ranks)
                res = self.team.run(lambda rank, world, eng: self._run_device(
                    X, Y, draws, eng, team=(rank, self.team)))
                unrefined = self.team.unrefined
            else:
                eng = self.engine or default_engine()
                ok = False
                with eng.lock:                         # one analysis at a time per context (shared default engine)
                    try:
                        res = self._run_device(X, Y, draws, eng)
                        ok = True
                    finally:
                        # state that must not leak into the next analysis on this context, whatever happened:
                        # the announced shard size and the refined / unrefined counters (a stale count would raise
                        # a spurious GradedSpectrumWarning -- and stale scratch sizing -- in an unrelated call)
                        if getattr(eng, 'ctx', None):
                            unrefined = eng.end_analysis(warn=ok) or 0
            # outside every finally: under -W error the warning must not replace a computed result half-way, and it
            # is attributed to the user's call (run <- behavioral_pls / meancentered_pls <- USER)
            Engine.warn_unrefined(unrefined, stacklevel=4)
            return res
        finally:
            draws.thread.join()                        # never leave the generators running on an error
            from .engine import touch_idle_release
            touch_idle_release()                       # (the cached engines are released after IDLE_RELEASE_S idle seconds)
            for ms in self._mstreams:
                ms.close()

    def _run_device(self, X, Y, draws, eng, team=None):
        """The analysis after the draws started (``team`` = (rank, Team): this thread is one rank of a
        single-process team, team.py -- every rank runs its shard and the collective, rank 0 alone finishes).  Everything B- or n_boot-sized stays on the device from the
        H2D copy of X to the finished statistics: the sign convention, the original's scores, the resampling,
        THE one collective, percentile intervals, bootstrap ratios and the (T', L, n_boot) layout of the
        distributions all run there; what PLSResults holds comes back once, into page-locked memory that is
        mapped while the device resamples.  (Round 3 crossed PCIe with the (B, L) weights five times and
        transposed the 200 MB distributions on the host: 0.26 - 0.30 s of fixed cost per call at c4.)"""
        import time
        import torch
        inp = self.inputs
        lead = team is None or team[0] == 0            # the rank that finishes the analysis and speaks for it
        phases = self.phases if lead else None         # dict: per-phase wall times (bench.py --mode analysis)

        t_last = [time.perf_counter()]

        def tick(name):
            if phases is None:
                return
            torch.cuda.synchronize(eng.device)
            now = time.perf_counter()
            phases[name] = phases.get(name, 0.0) + 1e3 * (now - t_last[0])
            t_last[0] = now

        cf = self.cf
        d_gx = d_gy = None
        if cf is not None:
            # confounds: this device's copies of X and Y are residualised on [1, Z - zbar] BEFORE they are bound, so
            # that everything the binding derives is built from the residuals; the host's Y becomes Y_r as well
            _check_finite(Y, 'Y')
            dX, dY, dZ = eng._dev(X, np.float64), eng._dev(Y, np.float64), eng._dev(cf['Z'], np.float64)
            d_gx, d_gy = eng.residualize(dX, dZ), eng.residualize(dY, dZ)
            eng.set_data(dX, dY, self.cells, len(inp.groups), inp.n_cond, _METHOD_CODE[self.method],
                         mean_centering=inp.get('mean_centering') or 0, covariance=bool(inp.get('covariance')))
            Y = dY.cpu().numpy()
            del dX
        else:
            eng.set_data(X, Y, self.cells, len(inp.groups), inp.n_cond, _METHOD_CODE[self.method],
                         mean_centering=inp.get('mean_centering') or 0,
                         covariance=bool(inp.get('covariance')))
        tick('h2d_and_bind')
        L = eng.L
        res = PLSResults(inputs=inp)
        # finite-input check (sklearn check_X_y in compute.xcorr, compute.py:78):
        # a NaN / inf anywhere in a column of X makes the device column mean
        # non-finite, which avoids a host pass over the (S, B) matrix
        d_xmean = eng.colmean_dev()
        if not bool(torch.isfinite(d_xmean).all().item()):
            raise ValueError('Input `X` contains NaN, infinity or a value too large')
        if Y is not None:
            _check_finite(Y, 'Y')

        # ---- original decomposition (BasePLS.svd, base.py:362-364), signs and scores on the device -------
        Lc = L                                         # columns of the results (non-rotated PLS: the contrasts')
        if self.V is not None:
            # non-rotated PLS: the contrasts stand where the SVD's y_weights stand; they fix the sign
            eng.set_contrasts(self.V)
            Lc = self.V.shape[1]
            d_xw, d_sv, d_yw = eng.decompose_dev()
        else:
            d_xw, d_sv, d_yw = eng.decompose_dev()
            eng.svd_flip(d_xw, d_yw)
        eng.set_original(d_xw, d_sv, d_yw)
        d_scores = eng.project_dev(d_xw)               # (X - mean) @ x_weights; the mean's share is added on the host
        sv = d_sv.cpu().numpy()
        yw = d_yw.cpu().numpy()
        if Lc != L:
            sv, yw = sv[:Lc].copy(), np.ascontiguousarray(yw[:, :Lc])
        tick('decompose')
        emulate = self.emulate                         # (rank, world) of an emulated run on one GPU (bench.py)
        if team is not None:
            rank, world = team[0], team[1].world
        else:
            rank, world = emulate if emulate is not None else parallel.rank_world()
        rotate = bool(inp.get('rotate', True))

        # ---- resampling: this rank's contiguous shard of the permutations and chunk-cyclic share
        # ---- of the bootstraps, launched chunk by chunk as the index rows arrive; results stay
        # ---- on the device through THE one collective (parallel.collect_device) ---------
        pstream, bstream, ystack = self.perm_stream, self.boot_stream, self.ystack
        n_perm_tot = pstream.n if pstream is not None else (ystack.shape[0] if ystack is not None else 0)
        n_boot_tot = bstream.n if bstream is not None else 0
        d_perm = d_dist = d_keep = usum = usq = None
        plo, phi = parallel.shard_bounds(n_perm_tot, rank, world)
        # Chunked shipping (IndexStream.chunks: 256 rows, then 4 x longer ranges) lets the device start while the
        # generator thread still draws.  It pays at both ends of the size range: c4's shard is device-seconds long
        # against 25 ms of drawing, and c2's 5000 + 5000 index rows take the host about as long to DRAW (4 - 9 ms)
        # as the device needs to process them -- shipping them as one range when the draw ends (tried: est. device
        # time < 50 ms -> one range) made the call slower, 9.9 -> 11.4 ms.  Caller-supplied arrays are one range.
        first = 256
        n_split = inp.get('n_split')
        mstream = None
        if n_split is not None and (pstream is not None or ystack is not None) and phi > plo:
            # split masks of this rank's permutations: produced block by block on their own host thread, from
            # now on, while the device runs the permutations and the bootstraps (permutation i uses
            # RandomState(i), base.py:705-708)
            mstream = resampling.MaskStream(inp.groups, inp.n_cond, n_split, plo, phi,
                                            given=inp.get('_perm_splitsamples'))
            self._mstreams.append(mstream)
        # the shard arrives in chunks: size the super-batch scratch once, for all of it
        eng.set_option('expect_resamples', max(phi - plo, sum(hi - lo for lo, hi in parallel.shard_chunks(
            n_boot_tot, rank, world)) if bstream is not None else 0))
        # verbose=True: the reference's tqdm bars (pyls/utils.py:128-152), counting resamples the DEVICE has finished;
        # they only appear when a leg is still running after 2 s (progress.py)
        from .progress import Bar
        show = lead and bool(inp.get('verbose')) and (emulate is None) and (parallel.rank_world()[0] == 0)
        bars = []
        if pstream is not None:
            d_perm = eng._zeros((phi - plo, L))
            bar = Bar('Running permutations', phi - plo, show, eng.device)
            bars.append(bar)
            for a, b in pstream.chunks(plo, phi, first=first):
                eng.perm_into(eng.rows_tensor(pstream.rows[a:b]), d_perm[a - plo:b - plo], rotate=rotate)
                bar.queued(b - a)
        elif ystack is not None:
            host = eng.perm_ystack(ystack[plo:phi], rotate=rotate) if phi > plo else np.zeros((L, 0))
            d_perm = torch.from_numpy(np.ascontiguousarray(host.T)).to(eng.device)
        tick('permutations')
        d_wcnt = d_wmax = d_wobs = None
        if self.wperm_m is not None:
            # weights_perm: this rank's share of the index rows once more, through the stateless test
            # (plsx_perm_weights_test): the null Z_p = R_p^T V0 is formed tile by tile, counted against the observed
            # x_weights @ diag(singvals) and reduced to its maxima over the features; counts and maxima ride in the
            # collective.  The rows of R are correlations in correlation-mode behavioral PLS; elsewhere the maxima are
            # taken over |Z_p| / s_f
            wm = self.wperm_m
            wstd = not (self.method == 'behavioral' and not inp.get('covariance'))
            d_wobs = eng.scale_columns(d_xw, d_sv)[:, :wm].contiguous()
            d_wcnt = torch.zeros((eng.B, wm), dtype=torch.int32, device=eng.device)
            d_wmax = eng._zeros((phi - plo, wm))
            if phi > plo:
                eng.perm_weights_test(eng.rows_tensor(pstream.rows[plo:phi]), d_yw[:, :wm].contiguous(), d_wobs, d_wcnt,
                                      d_wmax, standardise=wstd)
            if wstd:
                d_wobs = d_wobs.abs() * eng.perm_weights_scale()[:, None]      # (the observed side of the maxT comparison)
            else:
                d_wobs = d_wobs.abs()
            tick('weights_perm')
        if bstream is not None:
            # chunk-cyclic share (parallel.shard_chunks): no rank waits for the END of the draw
            # before its device has anything to do
            bchunks = parallel.shard_chunks(n_boot_tot, rank, world)
            usum, usq = eng._zeros((eng.B, L)), eng._zeros((eng.B, L))
            d_dist = eng._zeros((sum(hi - lo for lo, hi in bchunks), eng.Tp, L))
            off = 0
            # the series of this rank's bootstraps: where the weights are linear in the (unscaled) features the
            # library accumulates S x S moments per batch and passes the features once, in boot_finish
            eng.boot_begin(sum(hi - lo for lo, hi in bchunks))
            if self.weights_m is not None:
                # weights_ci: every bootstrap also leaves its rotation operand (m, T'); the stack rides in the collective
                d_keep = eng._zeros((d_dist.shape[0], self.weights_m, eng.Tp))
                if d_keep.shape[0] > 0:
                    eng.boot_keep(d_keep)
            bar = Bar('Running bootstraps', sum(hi - lo for lo, hi in bchunks), show, eng.device)
            bars.append(bar)
            for blo, bhi in bchunks:
                for a, b in bstream.chunks(blo, bhi, first=first):
                    eng.boot_into(eng.rows_tensor(bstream.rows[a:b]), usum, usq,
                                  d_dist[off + a - blo:off + b - blo])
                    for done in bars:
                        done.poll()
                    bar.queued(b - a)
                off += bhi - blo
            eng.boot_finish(usum, usq)
            if d_keep is not None:
                eng.boot_keep(None)
        # host work that needs no device result runs while the device is busy: page-locked landing zones of
        # the results (56 us per MB to map), the index arrays in the reference's layout and dtype ((S, n)
        # C-contiguous int64), the host-sized scores of the original data
        pin = {}
        permsamp = bootsamp = None
        if lead:
            pin = {'xw': eng.pinned_like(d_xw), 'scores': eng.pinned_like(d_scores)}
            if bstream is not None:
                pin['bsr'], pin['se'] = eng.pinned_like(d_xw), eng.pinned_like(d_xw)
                pin['dist'] = torch.empty((eng.Tp * L, n_boot_tot), dtype=torch.float64, pin_memory=True)
            if pstream is not None:
                permsamp = self.perm_given if self.perm_given is not None else pstream.samples
            if bstream is not None:
                bootsamp = self.boot_given if self.boot_given is not None else bstream.samples
        draws.join()
        for st in (pstream, bstream, self.cvperm_stream):
            if st is not None and lead:
                st.warn()
        for bar in bars:
            bar.watch()
        try:
            eng.sync()             # numerical status of the launches above is raised HERE, for the batch that set it
        finally:
            for bar in bars:
                bar.close()
        tick('bootstraps')
        orig_splits = self.orig_splits
        slices, totals = [], []
        if d_perm is not None:
            if orig_splits is not None:
                # split-half reliability of every permuted arrangement (base.py:705-708): block by block as the
                # masks arrive, the mean over splits (base.py:770) taken on the device; nothing visits the host
                d_uc, d_vc = eng._zeros((phi - plo, L)), eng._zeros((phi - plo, L))
                if mstream is not None:
                    sbar = Bar('Running split-half resampling of the permutations', phi - plo, show, eng.device)
                    try:
                        for a, b, masks in mstream:
                            dm = torch.from_numpy(masks).to(eng.device)
                            dp = eng.rows_tensor(pstream.rows[a:b]) if ystack is None else None
                            dy = eng._dev(ystack[a:b], np.float64) if ystack is not None else None
                            uc = eng._empty((b - a, masks.shape[1], L))
                            vc = eng._empty((b - a, masks.shape[1], L))
                            eng.split_half_into(dp, dm, uc, vc, ystack_dev=dy)
                            eng.mean_splits_into(uc, d_uc[a - plo:b - plo])
                            eng.mean_splits_into(vc, d_vc[a - plo:b - plo])
                            sbar.queued(b - a)
                        sbar.watch()
                        eng.sync()
                    finally:
                        sbar.close()
                        mstream.close()
                    if mstream.duplicates and lead:
                        warnings.warn('WARNING: Duplicate split halves used.')
                # ride along with the permutation block of the single collective
                d_perm = torch.cat([d_perm, d_uc, d_vc], dim=1)
                eng.sync()
                tick('split_half')
            if d_wmax is not None:
                # weights_perm: the maxima ride behind everything else in the permutation block
                d_perm = torch.cat([d_perm, d_wmax], dim=1)
            slices.append(d_perm)
            totals.append(n_perm_tot)
        cyclic = []
        if d_dist is not None:
            cyclic.append(len(slices))
            slices.append(d_dist)
            totals.append(n_boot_tot)
            if d_keep is not None:
                cyclic.append(len(slices))
                slices.append(d_keep)
                totals.append(n_boot_tot)
        cv_splits = self.cv_splits
        if cv_splits is not None and cf is not None:
            # the fold-wise confound regression: drawn masks are checked as soon as they exist, then Z~ is bound
            if inp.get('_cvsplits') is None:
                _check_cvrank(cf, np.asarray(cv_splits, dtype=bool))
            eng.set_confounds(dZ)
        if cv_splits is not None:
            # cross-validation (behavioral.py:219-221, 82-170): its shard rides in the same buffer
            clo, chi = parallel.shard_bounds(cv_splits.shape[1], rank, world)
            # cv_lv: the score correlations of the first lvm latent variables come out of the same pass
            # (plsx_crossval_lv_batch) and ride in the same slice, 2 T + lvm columns wide
            lvm = self.cv_lv_m or 0
            crossval = eng.crossval if cf is None else eng.crossval_confound
            d_pred = None
            if inp.get('cv_predict'):
                # the out-of-fold predictions of this rank's shard, a slot (T, S) per split, exported by the same pass
                # (plsx_crossval_pred_begin) -- with the fold-residualised Y beside them on the confound route
                Tn, Sn = Y.shape[1], len(X)
                nbytes = 8 * (chi - clo) * Tn * Sn * (2 if cf is not None else 1)
                free = torch.cuda.mem_get_info(eng.device)[0]
                if nbytes > free:
                    raise MemoryError('cv_predict: the stack of predictions of {} splits x T = {} x S = {} is {:.3f} GB{}; '
                                      '{:.3f} GB of device memory are free'
                                      .format(chi - clo, Tn, Sn, nbytes / 2 ** 30,
                                              ' with the fold-residualised Y beside it' if cf is not None else '',
                                              free / 2 ** 30))
                d_pred = [eng._empty((chi - clo, Tn, Sn)), eng._empty((chi - clo, Tn, Sn)) if cf is not None else None]
                if chi > clo:
                    eng.crossval_pred_begin(*d_pred)
            if chi > clo and lvm:
                r, r2, lvc = crossval(cv_splits[:, clo:chi], lv=True)
                local_cv = np.vstack([r, r2, lvc[:lvm]]).T                            # (m_loc, 2 T + lvm)
            elif chi > clo:
                r, r2 = crossval(cv_splits[:, clo:chi])
                local_cv = np.vstack([r, r2]).T                                       # (m_loc, 2 T)
            else:
                local_cv = np.zeros((0, 2 * Y.shape[1] + lvm))
            slices.append(torch.from_numpy(np.ascontiguousarray(local_cv)).to(eng.device))
            totals.append(cv_splits.shape[1])
            if d_pred is not None:
                if chi > clo:
                    eng.crossval_pred_end()
                for t in d_pred:                        # (the prediction rows ride in the same collective)
                    if t is not None:
                        slices.append(t)
                        totals.append(cv_splits.shape[1])
            tick('crossval')
        cvp = self.cvperm_stream if cv_splits is not None else None
        if cvp is not None:
            # cv_perm: the ranks shard the PERMUTATIONS, every rank under all the splits -- one S x S matrix per split
            # serves all of a rank's permutations, handed over in one call (plsx_crossval_perm_batch); the null rides
            # in the same collective
            qlo, qhi = parallel.shard_bounds(cvp.n, rank, world)
            d_null = eng._zeros((qhi - qlo, 2 * Y.shape[1] + lvm))
            if qhi > qlo:
                cvp.wait(qhi)
                dmk = torch.from_numpy(np.ascontiguousarray(cv_splits.T, dtype=np.uint8)).to(eng.device)
                nr, nr2 = eng._empty((qhi - qlo, Y.shape[1])), eng._empty((qhi - qlo, Y.shape[1]))
                crossval_perm_into = eng.crossval_perm_into if cf is None else eng.crossval_confound_perm_into
                if lvm:
                    # cv_lv: the split means of every permutation's score correlations (plsx_crossval_perm_lv_batch)
                    nlv = eng._empty((qhi - qlo, eng.L))
                    crossval_perm_into(dmk, eng.rows_tensor(cvp.rows[qlo:qhi]), nr, nr2, nlv)
                    d_null = torch.cat([nr, nr2, nlv[:, :lvm]], dim=1)
                else:
                    crossval_perm_into(dmk, eng.rows_tensor(cvp.rows[qlo:qhi]), nr, nr2)
                    d_null = torch.cat([nr, nr2], dim=1)
                eng.sync()
            slices.append(d_null)
            totals.append(cvp.n)
            tick('crossval_perm')
        sums = [usum, usq] if usum is not None else []
        if d_wcnt is not None:
            sums.append(d_wcnt.to(torch.float64))      # (integers far below 2^53: their sum over the ranks is exact)
        full, summed = parallel.collect_device(slices, totals, sums, cyclic=cyclic, emulate=emulate, team=team)
        if not lead:
            return None                                # rank 0 holds everything the ranks computed: it finishes
        if usum is not None:
            usum, usq = summed[:2]
        tick('collective')

        # ---- finish on the device; one trip home -----------------------------------------------------
        k = 0
        d_perm = distrib = None
        lo_hi = None
        if n_perm_tot > 0:
            blk = full[k].cpu().numpy().T                                             # (L or 3 L [+ m], n_perm)
            k += 1
            d_perm = np.ascontiguousarray(blk[:Lc])
            if orig_splits is not None:
                ucorrs, vcorrs = np.ascontiguousarray(blk[L:2 * L]), np.ascontiguousarray(blk[2 * L:3 * L])
            if d_wmax is not None:
                wmax = np.ascontiguousarray(blk[blk.shape[0] - self.wperm_m:])         # (m, n_perm)
                wcnt = np.rint(summed[-1].detach().cpu().numpy()).astype(np.int64)
        h_bsr = h_se = h_dist = None
        if bstream is not None:
            d_full = full[k]                                                           # (n_boot, T', L)
            k += 1
            d_series = eng.transpose_dev(d_full.reshape(n_boot_tot, eng.Tp * L))       # (T' L, n_boot) series
            if d_keep is not None:
                # weights_ci: the closing pass over the gathered stack (n_boot, m, T') and ALL index rows, on this rank
                tick('finish_and_d2h')
                d_wlo, d_whi = eng.boot_weights_ci(eng.rows_tensor(bstream.rows[:n_boot_tot]), full[k].contiguous(),
                                                   ci=inp.get('ci', 95))
                k += 1
                tick('weights_ci')
            lo_hi = eng.percentile_ci_dev(d_series, ci=inp.get('ci', 95))
            h_dist = eng.to_host_async(d_series, pin['dist'])
            d_bs = eng.scale_columns(d_xw, d_sv)                                       # x_weights @ singvals
            if self.method in ('behavioral', 'multiblock'):
                # add the original back, n_boot + 1 (behavioral.py:201-207)
                d_bsr, d_se = eng.boot_rel_dev(d_bs, usum, usq, n_boot_tot + 1, add_orig=True)
            else:
                # no add-back, n_boot (meancentered.py:162-164)
                d_bsr, d_se = eng.boot_rel_dev(d_bs, usum, usq, n_boot_tot, add_orig=False)
            h_bsr, h_se = eng.to_host_async(d_bsr, pin['bsr']), eng.to_host_async(d_se, pin['se'])
        h_xw = eng.to_host_async(d_xw, pin['xw'])
        h_scores = eng.to_host_async(d_scores, pin['scores'])
        xmean = d_xmean.cpu().numpy()
        if cv_splits is not None:
            Tn = Y.shape[1]
            cv = full[k].cpu().numpy().T
            res['cvres'].update(dict(pearson_r=np.ascontiguousarray(cv[:Tn]),
                                     r_squared=np.ascontiguousarray(cv[Tn:2 * Tn])))
            if lvm:
                res['cvres']['lv_corr'] = np.ascontiguousarray(cv[2 * Tn:])           # (lvm, test_split)
            if inp.get('cv_predict'):
                k += 1
                res['cvres']['y_pred'] = np.ascontiguousarray(full[k].cpu().numpy().transpose(2, 1, 0))   # (S, T, n)
                if cf is not None:
                    k += 1
                    res['cvres']['y_true'] = np.ascontiguousarray(full[k].cpu().numpy().transpose(2, 1, 0))
            if cvp is not None:
                k += 1
                null = full[k].cpu().numpy().T                                        # (2 T [+ lvm], P)
                null_r, null_r2 = np.ascontiguousarray(null[:Tn]), np.ascontiguousarray(null[Tn:2 * Tn])
                if lvm:
                    null_lv = np.ascontiguousarray(null[2 * Tn:])
                    res['cvres'].update(dict(perm_lv_corr=null_lv,
                                             lv_corr_pvals=_lv_corr_pvals(res['cvres']['lv_corr'], null_lv)))
                with np.errstate(invalid='ignore'):                                   # (a NaN null value compares false)
                    res['cvres'].update(dict(
                        perm_pearson_r=null_r, perm_r_squared=null_r2,
                        pearson_r_pvals=hostmath.perm_sig(res['cvres']['pearson_r'].mean(axis=-1), null_r),
                        r_squared_pvals=hostmath.perm_sig(res['cvres']['r_squared'].mean(axis=-1), null_r2),
                        cvpermsamples=(np.asarray(self.cvperm_given) if self.cvperm_given is not None
                                       else cvp.samples),
                        cvsamples=np.ascontiguousarray(cv_splits, dtype=bool)))
        eng.sync()
        tick('finish_and_d2h')
        xw = _host_array(h_xw)
        scores = h_scores.numpy()
        if Lc != L:
            xw, scores = np.ascontiguousarray(xw[:, :Lc]), scores[:, :Lc]
        res['x_weights'], res['y_weights'] = xw, yw
        res['x_scores'] = scores + (xmean @ xw)[None, :]
        if orig_splits is not None and d_perm is not None:
            uc, vc = eng.split_half(orig_splits)
            orig_uc, orig_vc = uc[0].mean(axis=-1), vc[0].mean(axis=-1)
            ci = inp.get('ci', 95)
            ull, uul = hostmath.boot_ci(ucorrs, ci=ci)
            vll, vul = hostmath.boot_ci(vcorrs, ci=ci)
            res['splitres'].update(dict(
                ucorr=orig_uc, vcorr=orig_vc,
                ucorr_pvals=hostmath.perm_sig(orig_uc, ucorrs),
                vcorr_pvals=hostmath.perm_sig(orig_vc, vcorrs),
                ucorr_lolim=ull, vcorr_lolim=vll, ucorr_uplim=uul, vcorr_uplim=vul))
            self.split_null = (ucorrs, vcorrs)
        if d_perm is not None:
            res['permres']['pvals'] = hostmath.perm_sig(sv, d_perm)
            res['permres']['permsamples'] = permsamp if ystack is None else \
                np.transpose(ystack, (1, 2, 0))                   # base.py:638-639 layout
            res['permres']['perm_singval'] = d_perm
            if d_wmax is not None:
                res['permres'].update(_weights_perm_pvals(d_wobs.cpu().numpy(), wcnt, wmax))

        # ---- scores / loadings (subclass run_pls) --------------------------
        if self.method in ('behavioral', 'multiblock'):
            y_scores = np.zeros((len(X), Lc))
            T = Y.shape[1]
            row0 = self.n_cells if self.method == 'multiblock' else 0      # (multiblock: the behaviour rows of y_weights)
            for c in range(self.n_cells):
                m = self.cells == c
                y_scores[m] = Y[m] @ yw[row0 + c * T:row0 + (c + 1) * T]
            res['y_scores'] = y_scores
            res['y_loadings'] = hostmath.cellwise_xcorr(res['x_scores'], Y, self.cells,
                                                        self.n_cells, bool(inp.get('covariance')))
            if self.method == 'multiblock':
                # the two gen_distrib outputs stacked, not row-normalised: cell means of the mean-centred scores first
                res['y_loadings'] = np.vstack([hostmath.cell_means_centered(
                    res['x_scores'], self.cells, len(inp.groups), inp.n_cond, inp.get('mean_centering') or 0),
                    res['y_loadings']])
        else:
            dummy = resampling.dummy_code(inp.groups, inp.n_cond)
            inp['Y'] = dummy
            res['y_scores'] = dummy @ yw
            # contrast = cell means of the mean-centred brain scores
            # (meancentered.py:151-155) = gen_covcorr(X) @ x_weights
            contrast = eng.crosscov(n=1)[0] @ xw

        # ---- bootstrap ratios / intervals ----------------------------------
        if bootsamp is not None:
            distrib = _host_array(h_dist).reshape(eng.Tp, L, n_boot_tot)                   # (T', L, n_boot)
            if lo_hi is not None:
                ci_arr = np.stack([lo_hi[0].cpu().numpy().reshape(eng.Tp, L),
                                   lo_hi[1].cpu().numpy().reshape(eng.Tp, L)], -1)
            else:                                       # more than 16384 bootstraps: numpy on the host copy
                ci_arr = np.stack(hostmath.boot_ci(distrib, ci=inp.get('ci', 95)), -1)
            bsr, se = _host_array(h_bsr), _host_array(h_se)
            if Lc != L:
                distrib, ci_arr = np.ascontiguousarray(distrib[:, :Lc]), np.ascontiguousarray(ci_arr[:, :Lc])
                bsr, se = np.ascontiguousarray(bsr[:, :Lc]), np.ascontiguousarray(se[:, :Lc])
            if self.method in ('behavioral', 'multiblock'):
                res['bootres'].update(dict(
                    x_weights_normed=bsr, x_weights_stderr=se,
                    y_loadings=res['y_loadings'].copy(), y_loadings_boot=distrib,
                    y_loadings_ci=ci_arr, bootsamples=bootsamp))
            else:
                res['bootres'].update(dict(
                    x_weights_normed=bsr, x_weights_stderr=se, bootsamples=bootsamp,
                    contrast=contrast, contrast_boot=distrib, contrast_ci=ci_arr))
            if d_keep is not None:
                res['bootres']['x_weights_ci'] = np.stack([d_wlo.cpu().numpy(), d_whi.cpu().numpy()], -1)   # (B, m, 2)

        res['varexp'] = hostmath.varexp(sv)
        res['singvals'] = sv
        if cf is not None:
            res['confound_mean'] = cf['zmean']
            res['confound_x'], res['confound_y'] = d_gx.cpu().numpy(), d_gy.cpu().numpy()
        tick('host_finish')
        self.engine_used = eng
        return res


def _check_cv_perm(cv_perm, cvpermsamples, X, test_split, test_size, contrasts):
    """The checks of ``behavioral_pls(cv_perm=, cvpermsamples=)``, on the host before any engine (wording and order of
    ``pls_regression``) -> False when not asked for, else the validated (S, P) array or None (to be drawn)."""
    if isinstance(cv_perm, (bool, np.bool_)) or not isinstance(cv_perm, (int, np.integer)) or cv_perm < 0:
        raise ValueError('Provided `cv_perm` must be a non-negative integer; got {!r}'.format(cv_perm))
    if int(cv_perm) == 0:
        return False
    if not (int(test_split or 0) > 0 and (test_size or 0) > 0):
        raise ValueError('`cv_perm` needs cross-validation: it permutes Y under the splits of `test_split` > 0 with '
                         '`test_size` > 0; got test_split = {!r}, test_size = {!r}'.format(test_split, test_size))
    if contrasts is not None:
        raise ValueError('`cv_perm` is not available with `contrasts`: non-rotated PLS has no fitted decomposition to '
                         'predict from, its cross-validation is not run')
    if cvpermsamples is None:
        return None
    from .engine import check_index_array
    S = len(X)
    cvperm = np.asarray(cvpermsamples)
    if cvperm.ndim != 2 or cvperm.shape != (S, int(cv_perm)):
        raise ValueError('Provided `cvpermsamples` must have shape (S, cv_perm) = ({}, {}); got {}'
                         .format(S, int(cv_perm), cvperm.shape))
    cvperm = check_index_array(cvperm, S)
    if not np.array_equal(np.sort(cvperm, axis=0), np.broadcast_to(np.arange(S)[:, None], cvperm.shape)):
        bad = int(np.flatnonzero((np.sort(cvperm, axis=0) != np.arange(S)[:, None]).any(axis=0))[0])
        raise ValueError('Provided `cvpermsamples` must hold one permutation of 0 .. {} per column; column {} '
                         'is not one'.format(S - 1, bad))
    return cvperm


def _check_cv_lv(cv_lv, X, Y, groups, n_cond, test_split, test_size, contrasts):
    """The checks of ``behavioral_pls(cv_lv=)``, on the host before any engine -> False when not asked for, else the
    number of latent variables m (True: all L = min(T', B))."""
    if cv_lv is False or cv_lv is None:
        return False
    if not (int(test_split or 0) > 0 and (test_size or 0) > 0):
        raise ValueError('`cv_lv` needs cross-validation: it correlates the scores of the test rows under the splits of '
                         '`test_split` > 0 with `test_size` > 0; got test_split = {!r}, test_size = {!r}'
                         .format(test_split, test_size))
    if contrasts is not None:
        raise ValueError('`cv_lv` is not available with `contrasts`: non-rotated PLS has no fitted decomposition to '
                         'project through, its cross-validation is not run')
    if X.ndim != 2 or Y.ndim != 2:
        raise ValueError('Expected 2D arrays for `X` and `Y`')
    n_groups = 1 if groups is None else (len(groups) if isinstance(groups, (list, np.ndarray)) else 1)
    L = min(n_groups * int(n_cond) * Y.shape[1], X.shape[1])
    if cv_lv is True:
        return L
    if isinstance(cv_lv, (bool, np.bool_)) or not isinstance(cv_lv, (int, np.integer)) or not 1 <= int(cv_lv) <= L:
        raise ValueError('`cv_lv` must be True or a number of latent variables in 1 .. {}; got {!r}'.format(L, cv_lv))
    return int(cv_lv)


def _check_cv_predict(cv_predict, test_split, test_size, contrasts):
    """The checks of ``behavioral_pls(cv_predict=)``, on the host before any engine -> True or False."""
    if cv_predict is None or (isinstance(cv_predict, (bool, np.bool_)) and not cv_predict):
        return False
    if not (isinstance(cv_predict, (bool, np.bool_)) and cv_predict):
        raise ValueError('`cv_predict` must be True or False for behavioral_pls (the prediction uses every live latent '
                         'variable); got {!r}'.format(cv_predict))
    if not (int(test_split or 0) > 0 and (test_size or 0) > 0):
        raise ValueError('`cv_predict` needs cross-validation: the predictions are those of the test rows of `test_split` '
                         '> 0 splits with `test_size` > 0; got test_split = {!r}, test_size = {!r}'
                         .format(test_split, test_size))
    if contrasts is not None:
        raise ValueError('`cv_predict` is not available with `contrasts`: non-rotated PLS has no fitted decomposition to '
                         'predict from, its cross-validation is not run')
    return True


def _refuse_cv_predict(kwargs, what):
    """``cv_predict`` belongs to behavioral_pls (and pls_regression / pls_da): refused on the host, before any engine."""
    if kwargs.get('cv_predict') not in (None, False):
        raise ValueError('`cv_predict` (the out-of-fold predictions) is not available for {}: only behavioral PLS is '
                         'cross-validated'.format(what))
    kwargs.pop('cv_predict', None)


def _refuse_cv_lv(kwargs, what):
    """``cv_lv`` belongs to behavioral_pls: refused on the host, before any engine."""
    if kwargs.get('cv_lv') not in (None, False):
        raise ValueError('`cv_lv` (the out-of-sample score correlation of the latent variables) is not available for '
                         '{}: only behavioral PLS is cross-validated'.format(what))
    kwargs.pop('cv_lv', None)


def _lv_corr_pvals(observed, null):
    """observed (m, n splits), null (m, P) split means -> (m,): (#{null > observed mean} + 1) / (P + 1); a NaN null value
    compares false, a NaN observed mean gives NaN."""
    mean = np.asarray(observed, dtype=np.float64).mean(axis=-1)
    with np.errstate(invalid='ignore'):
        p = hostmath.perm_sig(mean, null)
    return np.where(np.isnan(mean), np.nan, p)


def _refuse_cv_perm(kwargs, what):
    """``cv_perm`` / ``cvpermsamples`` belong to behavioral_pls: refused on the host, before any engine."""
    if kwargs.get('cv_perm') or kwargs.get('cvpermsamples') is not None:
        raise ValueError('`cv_perm` (the permutation test of the cross-validation) is not available for {}: only '
                         'behavioral PLS is cross-validated'.format(what))
    kwargs.pop('cv_perm', None)
    kwargs.pop('cvpermsamples', None)


def behavioral_pls(X, Y, *, groups=None, n_cond=1, n_perm=5000, n_boot=5000, n_split=0,
                   test_size=0.25, test_split=100, covariance=False, rotate=True, ci=95,
                   permsamples=None, bootsamples=None, seed=None, verbose=True, n_proc=None,
                   contrasts=None, weights_ci=False, cv_perm=0, cvpermsamples=None, cv_lv=False, confounds=None,
                   weights_perm=False, cv_predict=False, **kwargs):
    """Behavioral PLS of X (S, B) against Y (S, T); see pyls.behavioral_pls.  ``n_proc``: GPUs of this node to
    shard the resamples over (module docstring); ``device_ids=[...]`` names them.

    ``contrasts`` (T', Lc), T' = groups x conditions x behaviours in the row order of ``y_weights`` (group, then
    condition, then behaviour): non-rotated PLS.  The effects are the normalised columns of ``contrasts`` instead of
    the singular vectors of the cross-covariance matrix R: ``y_weights = V = normalize(contrasts)``, ``singvals[l] =
    ||R.T @ V[:, l]||``, ``x_weights`` the normalised ``R.T @ V``; permutations test each contrast (``rotate`` has no
    meaning), bootstraps give the reliability of each contrast's weights, and every result has Lc columns.  The
    cross-validation is not run (``cvres`` stays empty) and ``n_split`` > 0 raises.  A seeded call draws the same
    resampling arrays as the call without contrasts.

    ``weights_ci`` (True: all L latent variables; an int m: the first m, 1 <= m <= L): ``bootres.x_weights_ci`` (B, m, 2),
    the lower / upper ``ci`` percentile bound (numpy's linear interpolation) of the Procrustes-rotated, singular-value-
    scaled bootstrap weights U_b over the ``n_boot`` bootstraps.  The units are those of ``x_weights @ diag(singvals)``,
    the numerator of ``bootres.x_weights_normed``; the original fit is not part of the series (as for
    ``y_loadings_ci``).  The (B, m, n_boot) series is formed on the device one chunk of features at a time and never
    exists whole.  Needs 1 <= ``n_boot`` <= 16384; not available with ``contrasts`` (ValueError).  Every other array of
    the result keeps its bits and a seeded call draws the same resampling arrays.

    ``weights_perm`` (True: all L latent variables; an int m: the first m, 1 <= m <= L, with ``contrasts`` L = Lc; False,
    the default: nothing is added, nothing is drawn differently, every array keeps its bits): permutation p-values of
    the x_weights, feature by feature, for the permutations of ``permres.permsamples``.  With V0 = ``y_weights[:, :m]``
    and R_p the cross-covariance matrix of permutation p, the null is Z_p = R_p.T @ V0 (B, m) -- the permuted
    cross-covariance read along the observed behavioural pattern -- and the observed statistic Z = ``x_weights[:, :m] *
    singvals[:m]``, the units of ``weights_ci``.  Where the Procrustes rotation of the permutation test is exact (L = T',
    every latent variable live) Z_p is the rotated, singular-value-scaled permuted weights, whose column norms are the
    rotated ``perm_singval``; everywhere else R_p.T @ V0 is its definition, and ``rotate`` does not enter.  ``permres``
    gains ``x_weights_pvals`` (B, m) = (#{p : |Z_p[f, l]| >= |Z[f, l]|} + 1) / (n_perm + 1); ``x_weights_max`` (m,
    n_perm) = max_f |Z_p[f, l]| / s_f; ``x_weights_pvals_fwe`` (B, m) = (#{p : x_weights_max[l, p] >= |Z[f, l]| / s_f} +
    1) / (n_perm + 1), corrected over the features of a latent variable's map (single-step maxT).  s_f = 1 in
    correlation mode, where the rows of R are correlations already; with ``covariance=True`` s_f is the standard
    deviation (ddof = 1) of feature f over all rows, and a feature without variance has statistic 0 and both p-values
    1.  The (B, m, n_perm) series never exists: the device forms it tile by tile, counts and keeps the maxima
    (plsx_perm_weights_test).  GPUs shard the permutations.  Needs ``n_perm`` > 0 and index permutations
    (``permindices=False`` raises).  Every other array of the result keeps its bits.

    Permutation test of the cross-validation: ``cv_perm=P`` (needs ``test_split`` > 0 and ``test_size`` > 0; 0, the
    default: nothing is added, nothing changes) runs the whole cross-validation, under the same splits, for P
    permutations of the rows of Y -- drawn after everything else a seeded call draws, the split masks included, or
    given as ``cvpermsamples`` (S, P), one permutation of 0 .. S-1 per column.  ``cvres`` gains ``perm_pearson_r`` /
    ``perm_r_squared`` (T, P), the mean over the splits of every permutation's scores; ``pearson_r_pvals`` /
    ``r_squared_pvals`` (T,) = (#{null > mean over the splits of the observed score} + 1) / (P + 1), a NaN null value
    counting as not larger; ``cvpermsamples`` (S, P) and ``cvsamples`` (S, test_split), the training masks the null rests
    on.  The feature side of a fit does not see the permutation, so the device forms one S x S matrix per split and
    every (permutation, split) fit is S x S work.  GPUs shard the permutations.  Not available with ``contrasts``
    (ValueError); a cohort whose per-split matrix does not fit the device is refused.

    Out-of-sample score correlation of the latent variables: ``cv_lv`` (True: all L latent variables; an int m: the
    first m, 1 <= m <= L; needs ``test_split`` > 0 and ``test_size`` > 0; False, the default: nothing is added, nothing
    changes).  For every split the held-out rows are projected through the weights fitted on the others: the brain score
    is the z the prediction uses, the behaviour score is the test row of Y, centred (and, without ``covariance``, scaled)
    by the training moments of its cell, times the cell's rows of the training V.  ``cvres.lv_corr`` (m, test_split) is
    their Pearson correlation over all test rows of the split, per latent variable (LV l = the l-th largest singular
    value of the split's fit); NaN for a latent variable that is not live.  With ``cv_perm=P`` also ``perm_lv_corr``
    (m, P), the mean over the splits under every permutation, and ``lv_corr_pvals`` (m,) = (#{null > mean over the
    splits of the observed value} + 1) / (P + 1), NaN where that observed mean is NaN.  Every other array of the
    result keeps its bits and a seeded call draws the same resampling arrays.  A single latent variable, unlike the
    prediction, is only as stable as the gap around its singular value.  Not available with ``contrasts``
    (ValueError).

    Out-of-fold predictions: ``cv_predict=True`` (needs cross-validation; False, the default: nothing is added, nothing
    is drawn differently, every array keeps its bits) returns what ``cvres.pearson_r`` / ``r_squared`` are reductions
    of: ``cvres.y_pred`` (S, T, test_split), for a test row of split s ``z V_j^T + mean_train_j(Y)`` over the live
    latent variables of the training decomposition (the row's cell j), in the units of Y, NaN on the training rows.
    With ``confounds`` the prediction is that of the fold-residualised test Y, which exists on the device only and
    comes back as ``cvres.y_true`` (S, T, test_split), NaN off the test rows.  Under ``cv_perm`` only the observed fits
    are returned.  The stack is 8 S T test_split bytes on the device (twice that with ``confounds``) and rides in the
    call's one collective.  Not available with ``contrasts`` (ValueError).

    Confounds: ``confounds=Z`` (S, q) or (S,), 1 <= q <= 15 (None, the default: nothing is added, nothing is drawn
    differently, every array keeps its bits).  X and Y are residualised on ``[1, Z - zbar]`` -- one intercept and common
    slopes over the whole cohort, whatever the groups and conditions; the per-cell centring follows as always -- once,
    on the device, before the data set is bound (plsx_residualize).  The observed decomposition, ``n_perm``, ``n_boot``,
    ``n_split``, ``weights_ci`` and ``contrasts`` run on the residuals: permutations permute rows of the residualised
    Y, bootstraps resample residual rows -- the confound regression is NOT refitted per bootstrap, a limit of this
    version -- and a seeded call draws what the call without the keyword draws.  The result gains ``confound_mean``
    (q,) = zbar and ``confound_x`` (q, B) / ``confound_y`` (q, T), the slopes of X and Y on Z - zbar; every other array
    speaks of the residuals.  With ``test_split`` > 0 the confound regression is fitted on the TRAINING rows of every
    split and applied to all its rows (cross-validated confound regression: whole-cohort residuals leak the test rows
    into the training data): ``cvres.pearson_r`` / ``r_squared`` and ``cv_lv`` are scored on that fold's data
    (plsx_crossval_confound_batch: one fold copy of X per split, a group of splits at a time), and ``cv_perm`` permutes
    the residualised Y and residualises it again per fold (plsx_crossval_confound_perm_batch).  Refused (ValueError):
    Z of the wrong shape, q > 15, non-finite Z, Z rank deficient together with the intercept on all rows or on the
    training rows of a split, ``permindices=False`` (pre-permuted Y matrices are not residualised)."""
    if contrasts is not None:
        kwargs['contrasts'] = contrasts            # (recorded in `inputs` only when given)
    if weights_ci is not False:
        kwargs['weights_ci'] = weights_ci          # (recorded in `inputs` only when given)
    if weights_perm is not False:
        kwargs['weights_perm'] = weights_perm      # (recorded in `inputs` only when given)
    if confounds is not None:
        cf = _check_confounds(confounds, np.asarray(X), kwargs.get('permindices', True), kwargs.get('_cvsplits'))
        kwargs['confounds'] = cf['Z']              # (recorded in `inputs` only when given)
        kwargs['_confounds'] = cf
    cvperm = _check_cv_perm(cv_perm, cvpermsamples, np.asarray(X), test_split, test_size, contrasts)
    if cvperm is not False:
        kwargs['cv_perm'] = int(cv_perm)           # (recorded in `inputs` only when asked for)
        kwargs['_cvpermsamples'] = cvperm
    lvm = _check_cv_lv(cv_lv, np.asarray(X), np.asarray(Y), groups, n_cond, test_split, test_size, contrasts)
    if lvm is not False:
        kwargs['cv_lv'] = cv_lv                    # (recorded in `inputs` only when asked for)
        kwargs['_cv_lv_m'] = lvm
    if _check_cv_predict(cv_predict, test_split, test_size, contrasts):
        kwargs['cv_predict'] = True                # (recorded in `inputs` only when asked for)
    run = _PLSCRun('behavioral', np.asarray(X), np.asarray(Y), groups=groups, n_cond=n_cond,
                   n_perm=n_perm, n_boot=n_boot, n_split=n_split, test_size=test_size,
                   test_split=test_split, covariance=covariance, rotate=rotate, ci=ci,
                   permsamples=permsamples, bootsamples=bootsamples, seed=seed, verbose=verbose,
                   n_proc=n_proc, **kwargs)
    return run.run()


def _meancentered_design(X, groups, n_cond, mean_centering):
    """The argument checks of pyls/types/meancentered.py:16-38 -> (groups, mean_centering), with its resets and warnings."""
    if groups is None:
        if len(X) // n_cond != len(X) / n_cond:
            raise ValueError('Provided `X` matrix with {} samples is not evenly divisible into '
                             '{} conditions. Please confirm inputs are correct and try again. '
                             .format(len(X), n_cond))
        groups = [len(X) // n_cond]
    elif not isinstance(groups, (list, np.ndarray)):
        groups = [groups]
    if n_cond == 1 and len(groups) == 1:
        raise ValueError('Cannot perform PLS with only one group and one condition. Please '
                         'confirm inputs are correct.')
    if n_cond == 1 and mean_centering == 0:
        warnings.warn('Cannot set mean_centering to 0 when there is only one condition. '
                      'Resetting mean_centering to 1.')
        mean_centering = 1
    elif len(groups) == 1 and mean_centering == 1:
        warnings.warn('Cannot set mean_centering to 1 when there is only one group. '
                      'Resetting mean_centering to 0.')
        mean_centering = 0
    if mean_centering not in (0, 1, 2):
        raise ValueError('Mean centering type must be in [0, 1, 2].')
    return groups, mean_centering


def meancentered_pls(X, *, groups=None, n_cond=1, mean_centering=0, n_perm=5000, n_boot=5000,
                     n_split=0, rotate=True, ci=95, permsamples=None, bootsamples=None,
                     seed=None, verbose=True, n_proc=None, contrasts=None, weights_ci=False, weights_perm=False,
                     **kwargs):
    """Mean-centred PLS of X (S, B) sorted into groups x conditions; see
    pyls.meancentered_pls (argument checks of pyls/types/meancentered.py:16-38).

    ``contrasts`` (T', Lc), T' = groups x conditions (group-major rows): non-rotated PLS, as for
    :func:`behavioral_pls`; the bootstrap keeps the mean-centred conventions (no add-back of the original).

    ``weights_ci`` (True or an int m): ``bootres.x_weights_ci`` (B, m, 2), percentile intervals of the rotated bootstrap
    weights in the units of ``x_weights @ diag(singvals)``, as for :func:`behavioral_pls`.

    ``weights_perm`` (True or an int m): ``permres.x_weights_pvals`` / ``x_weights_max`` / ``x_weights_pvals_fwe``, the
    permutation p-values of the x_weights as for :func:`behavioral_pls`; the permutations move the rows of X across the
    cells, and s_f is the standard deviation of feature f over all rows."""
    if contrasts is not None:
        kwargs['contrasts'] = contrasts            # (recorded in `inputs` only when given)
    if weights_ci is not False:
        kwargs['weights_ci'] = weights_ci          # (recorded in `inputs` only when given)
    if weights_perm is not False:
        kwargs['weights_perm'] = weights_perm      # (recorded in `inputs` only when given)
    _refuse_cv_perm(kwargs, 'mean-centred PLS')
    _refuse_confounds(kwargs, 'mean-centred PLS')
    _refuse_cv_lv(kwargs, 'mean-centred PLS')
    _refuse_cv_predict(kwargs, 'mean-centred PLS')
    X = np.asarray(X)
    groups, mean_centering = _meancentered_design(X, groups, n_cond, mean_centering)
    run = _PLSCRun('meancentered', X, None, groups=groups, n_cond=n_cond,
                   mean_centering=mean_centering, n_perm=n_perm, n_boot=n_boot, n_split=n_split,
                   rotate=rotate, ci=ci, permsamples=permsamples, bootsamples=bootsamples,
                   seed=seed, verbose=verbose, n_proc=n_proc, **kwargs)
    return run.run()


def _check_multiblock(X, Y, groups, n_cond, kwargs):
    """What multiblock_pls does not cover, refused on the host before any engine is created or looked up."""
    if kwargs.get('n_split'):
        raise ValueError('Split-half resampling (`n_split` > 0) is not available for multiblock PLS')
    if kwargs.get('test_split'):
        raise ValueError('Cross-validation (`test_split` > 0) is not available for multiblock PLS')
    if kwargs.get('contrasts') is not None:
        raise ValueError('Non-rotated PLS (`contrasts`) is not available for multiblock PLS')
    if not kwargs.get('permindices', True):
        raise ValueError('multiblock PLS permutes the task block through index arrays: `permindices=False` '
                         '(pre-permuted Y matrices) is not available')
    bscan = kwargs.pop('bscan', None)
    if bscan is not None and sorted(int(c) for c in np.atleast_1d(bscan)) != list(range(n_cond)):
        raise ValueError('A behaviour block on a subset of the conditions (`bscan`) is not available: the behaviour '
                         'block of multiblock PLS covers every condition')
    for key in ('n_split', 'test_split', 'test_size', 'contrasts'):
        kwargs.pop(key, None)
    if X.ndim != 2 or Y.ndim != 2:
        raise ValueError('Expected 2D arrays for `X` and `Y`')
    if Y.shape[1] < 1:
        raise ValueError('multiblock PLS needs at least one behaviour (column of `Y`)')
    J = len(groups) * n_cond
    Tp = J + J * Y.shape[1]
    from .engine import max_tprime
    if Tp > max_tprime():
        raise ValueError('multiblock PLS: T\' = J + J T = {} rows (J = {} cells, T = {} behaviours) exceed the limit '
                         'of {}'.format(Tp, J, Y.shape[1], max_tprime()))
    if len(X) == len(Y):                                # (a mismatch is reported by the run object, as everywhere)
        _check_finite(np.asarray(X, dtype=np.float64), 'X')
        _check_finite(np.asarray(Y, dtype=np.float64), 'Y')


def multiblock_pls(X, Y, *, groups=None, n_cond=1, mean_centering=0, n_perm=5000, n_boot=5000,
                   covariance=False, rotate=True, ci=95, permsamples=None, bootsamples=None, seed=None,
                   verbose=True, n_proc=None, **kwargs):
    """Multiblock PLS of X (S, B) sorted into groups x conditions, with behaviours Y (S, T): the condition-means block
    of :func:`meancentered_pls` and the brain-behaviour block of :func:`behavioral_pls` in ONE decomposition (the Matlab
    PLS toolbox's method 4 in structure; pyls has no counterpart).  With J = groups x conditions cells,

        R = vstack([rownorm(R_task), rownorm(R_behav)])        # T' = J + J T rows

    where R_task (J, B) is the mean-centred cross-covariance (cell means minus the ``mean_centering`` reference mean),
    R_behav (J T, B) the per-cell cross-correlation (``covariance=True``: cross-covariance) and rownorm divides every
    row by its L2 norm over the features (a zero row stays zero), so that neither block's raw scale decides the
    decomposition.  ``y_weights`` (T', L): the J task rows first (group-major, then condition), then the behaviour rows
    (group, condition, behaviour).  ``y_scores`` comes from the behaviour rows, cell by cell; ``y_loadings`` (T', L)
    stacks the cell means of the mean-centred scores and the per-cell correlation of Y with the scores, neither
    normalised.  Permutations draw ONE index array per resample: the rows of X change cells in the task block and the
    rows of Y move against X in the behaviour block.  Bootstraps resample X and Y together; the bootstrap ratios follow
    the behavioural convention (the original is added back, n_boot + 1).  Result keys are those of
    :func:`behavioral_pls`; a seeded call draws its arrays in the same order.

    Not available (ValueError): ``n_split`` > 0, cross-validation (``test_split``), ``contrasts``, ``weights_perm``,
    ``permindices=False``, a behaviour block on a subset of the conditions; one group with one condition (the task
    block is identically zero).  ``mean_centering`` is reset with a warning as in :func:`meancentered_pls`."""
    _refuse_cv_perm(kwargs, 'multiblock PLS')
    _refuse_confounds(kwargs, 'multiblock PLS')
    _refuse_cv_lv(kwargs, 'multiblock PLS')
    _refuse_cv_predict(kwargs, 'multiblock PLS')
    X, Y = np.asarray(X), np.asarray(Y)
    groups, mean_centering = _meancentered_design(X, groups, n_cond, mean_centering)
    groups = [int(g) for g in groups]
    _check_multiblock(X, Y, groups, n_cond, kwargs)
    run = _PLSCRun('multiblock', X, Y, groups=groups, n_cond=n_cond, mean_centering=mean_centering,
                   n_perm=n_perm, n_boot=n_boot, covariance=covariance, rotate=rotate, ci=ci,
                   permsamples=permsamples, bootsamples=bootsamples, seed=seed, verbose=verbose,
                   n_proc=n_proc, **kwargs)
    return run.run()
