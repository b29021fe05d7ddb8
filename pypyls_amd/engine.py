"""
ctypes binding of libplsx.so (C ABI: include/plsx.h) and a thin device-side
engine object.  PyTorch-ROCm tensors are used only as device-memory handles
(`data_ptr()`) and for host<->device copies; all arithmetic on the resampling
path runs in the hand-written HIP kernels of csrc/.

There is NO CPU fallback: without the built library or without a GPU every
entry point raises.
"""
import ctypes
import threading
import os

import numpy as np

from . import _build

_LIB = None

PLSX_BEHAVIORAL = 0
PLSX_MEANCENTERED = 1
PLSX_REGRESSION = 2
PLSX_FLAG_COVARIANCE = 1


class PlsxError(RuntimeError):
    pass


def _load():
    global _LIB
    if _LIB is not None:
        return _LIB
    # PyTorch-ROCm ships its own HIP runtime; import it first so that the
    # library binds to the runtime torch already loaded (one runtime/process).
    import torch  # noqa: F401
    path = _build.lib_path()
    if not os.path.exists(path):
        raise PlsxError(
            'libplsx.so is not built ({}). Run `python -c "import __graft_entry__ as g; '
            'g.build()"` (needs hipcc). There is no CPU fallback.'.format(path))
    lib = ctypes.CDLL(path)
    vp, i32, c_d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    sig = {
        'plsx_version': ([], i32),
        'plsx_max_tprime': ([], i32),
        'plsx_ctx_create': ([i32, ctypes.POINTER(vp)], i32),
        'plsx_ctx_destroy': ([vp], i32),
        'plsx_last_error': ([vp], ctypes.c_char_p),
        'plsx_sync': ([vp], i32),
        'plsx_set_data': ([vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, ctypes.c_uint, vp], i32),
        'plsx_num_lv': ([vp], i32),
        'plsx_tprime': ([vp], i32),
        'plsx_crosscov_batch': ([vp, vp, vp, i32, vp, vp], i32),
        'plsx_decompose': ([vp, vp, vp, vp, vp], i32),
        'plsx_scratch_read': ([vp, i32, i32, i32, vp, vp], i32),
        'plsx_set_original': ([vp, vp, vp, vp, vp], i32),
        'plsx_set_contrasts': ([vp, vp, i32, vp], i32),
        'plsx_project': ([vp, vp, i32, vp, vp], i32),
        'plsx_colmean': ([vp, vp, vp], i32),
        'plsx_perm_batch': ([vp, vp, i32, i32, vp, vp], i32),
        'plsx_perm_batch_y': ([vp, vp, i32, i32, vp, vp], i32),
        'plsx_crossval_batch': ([vp, vp, i32, vp, vp, vp], i32),
        'plsx_crossval_perm_batch': ([vp, vp, i32, vp, i32, vp, vp, vp], i32),
        'plsx_crossval_lv_batch': ([vp, vp, i32, vp, vp, vp, vp], i32),
        'plsx_crossval_perm_lv_batch': ([vp, vp, i32, vp, i32, vp, vp, vp, vp, vp], i32),
        'plsx_residualize': ([vp, vp, i32, i32, i32, vp, i32, vp, i32, vp], i32),
        'plsx_set_confounds': ([vp, vp, i32, vp], i32),
        'plsx_crossval_confound_batch': ([vp, vp, i32, vp, vp, vp, vp], i32),
        'plsx_crossval_confound_perm_batch': ([vp, vp, i32, vp, i32, vp, vp, vp, vp, vp], i32),
        'plsx_crossval_confound_group': ([vp], i32),
        'plsx_boot_batch': ([vp, vp, i32, vp, vp, vp, vp], i32),
        'plsx_boot_begin': ([vp, ctypes.c_longlong, vp], i32),
        'plsx_boot_finish': ([vp, vp, vp, vp], i32),
        'plsx_boot_route': ([vp], i32),
        'plsx_boot_keep': ([vp, vp, ctypes.c_longlong, i32], i32),
        'plsx_boot_weights_ci': ([vp, vp, vp, i32, i32, i32, c_d, i32, c_d, vp, vp, vp], i32),
        'plsx_perm_weights_build': ([vp, vp, i32, vp, i32, vp, vp], i32),
        'plsx_perm_weights_test': ([vp, vp, i32, vp, i32, vp, i32, vp, vp, vp], i32),
        'plsx_perm_weights_scale': ([vp, vp, vp], i32),
        'plsx_split_route': ([vp], i32),
        'plsx_split_half_batch': ([vp, vp, i32, vp, i32, vp, vp, vp], i32),
        'plsx_split_half_batch_y': ([vp, vp, vp, i32, vp, i32, vp, vp, vp], i32),
        'plsx_boot_rel': ([vp, vp, vp, vp, i32, i32, ctypes.c_longlong, vp, vp, vp], i32),
        'plsx_last_timing': ([vp, ctypes.POINTER(c_d), i32], i32),
        'plsx_set_timing': ([vp, i32], i32),
        'plsx_kernel_timing': ([vp, i32, ctypes.POINTER(c_d), ctypes.POINTER(i32)], i32),
        'plsx_kernel_class_name': ([i32], ctypes.c_char_p),
        'plsx_set_perm_path': ([vp, i32], i32),
        'plsx_mean_splits': ([vp, vp, i32, i32, i32, vp, vp], i32),
        'plsx_svd_flip': ([vp, vp, vp, vp], i32),
        'plsx_scale_columns': ([vp, vp, ctypes.c_longlong, i32, vp, vp, vp], i32),
        'plsx_transpose': ([vp, vp, i32, i32, vp, vp], i32),
        'plsx_center_rows': ([vp, vp, i32, ctypes.c_longlong, vp, vp], i32),
        'plsx_set_option': ([vp, ctypes.c_char_p, i32], i32),
        'plsx_option_name': ([i32], ctypes.c_char_p),
        'plsx_numeric_report': ([vp, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)], i32),
        'plsx_set_scratch': ([vp, c_d, i32], i32),
        'plsx_mfma_f64_peak': ([vp, ctypes.POINTER(c_d)], i32),
        'plsx_percentile_ci': ([vp, vp, ctypes.c_longlong, i32, i32, c_d, i32, c_d, vp, vp, vp], i32),
        'plsx_simpls_decompose': ([vp, vp, vp, vp, vp, vp], i32),
        'plsx_simpls_set_original': ([vp, vp, vp], i32),
        'plsx_simpls_perm_batch': ([vp, vp, i32, vp, vp], i32),
        'plsx_simpls_boot_batch': ([vp, vp, vp, i32, vp, vp, vp, vp], i32),
        'plsx_simpls_set_row_masks': ([vp, vp, vp, vp], i32),
        'plsx_simpls_crossval_batch': ([vp, vp, i32, vp, vp, vp, vp], i32),
        'plsx_simpls_crossval_perm_batch': ([vp, vp, i32, vp, i32, vp, vp, vp, vp], i32),
        'plsx_simpls_crossval_nested_batch': ([vp, vp, i32, i32, vp, vp, vp, vp, vp, vp], i32),
        'plsx_simpls_crossval_nested_perm_batch': ([vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp], i32),
        'plsx_simpls_split_half_batch': ([vp, vp, i32, vp, i32, vp, vp, vp], i32),
        'plsx_simpls_set_confounds': ([vp, vp, i32, vp, vp, vp], i32),
        'plsx_simpls_crossval_confound_batch': ([vp, vp, i32, vp, vp, vp, vp], i32),
        'plsx_simpls_crossval_confound_perm_batch': ([vp, vp, i32, vp, i32, vp, vp, vp, vp], i32),
        'plsx_simpls_coef_begin': ([vp, i32, vp], i32),
        'plsx_simpls_coef_finish': ([vp, vp, vp, vp], i32),
        'plsx_simpls_coef_keep': ([vp, vp, ctypes.c_longlong], i32),
        'plsx_simpls_coef_ci': ([vp, vp, ctypes.c_longlong, i32, c_d, i32, c_d, vp, vp, vp], i32),
        'plsx_simpls_coef_perm_test': ([vp, vp, ctypes.c_longlong, vp, i32, vp, vp, vp], i32),
        'plsx_simpls_coef_perm_begin': ([vp, i32, vp, i32, vp, vp, ctypes.c_longlong], i32),
        'plsx_simpls_coef_perm_end': ([vp], i32),
        'plsx_simpls_set_classes': ([vp, vp, i32, vp], i32),
        'plsx_simpls_cv_class_begin': ([vp, vp, ctypes.c_longlong], i32),
        'plsx_simpls_cv_class_end': ([vp], i32),
        'plsx_simpls_cv_auc_begin': ([vp, vp, ctypes.c_longlong], i32),
        'plsx_simpls_cv_auc_end': ([vp], i32),
        'plsx_simpls_cv_pred_begin': ([vp, i32, vp, vp, vp, ctypes.c_longlong], i32),
        'plsx_simpls_cv_pred_end': ([vp], i32),
        'plsx_simpls_cvn_class_begin': ([vp, i32, vp, vp, vp, ctypes.c_longlong], i32),
        'plsx_simpls_cvn_class_end': ([vp], i32),
        'plsx_crossval_pred_begin': ([vp, vp, vp, ctypes.c_longlong], i32),
        'plsx_crossval_pred_end': ([vp], i32),
        'plsx_simpls_vip_keep': ([vp, i32, vp, ctypes.c_longlong], i32),
        'plsx_simpls_vip_ci': ([vp, vp, ctypes.c_longlong, i32, i32, c_d, i32, c_d, vp, vp, vp, vp], i32),
        'plsx_simpls_vip_perm_test': ([vp, vp, ctypes.c_longlong, i32, vp, vp, vp, vp], i32),
        'plsx_simpls_vip_perm_begin': ([vp, i32, vp, vp, vp, ctypes.c_longlong], i32),
        'plsx_simpls_vip_perm_end': ([vp], i32),
        'plsx_gen_permsamp': ([vp, i32, i32, i32, vp, ctypes.POINTER(i32), vp], i32),
        'plsx_gen_bootsamp': ([vp, i32, i32, i32, vp, ctypes.POINTER(i32), vp], i32),
        'plsx_gen_permsamp_stream': ([vp, i32, i32, i32, vp, ctypes.POINTER(i32), vp, ctypes.POINTER(i32)], i32),
        'plsx_gen_bootsamp_stream': ([vp, i32, i32, i32, vp, ctypes.POINTER(i32), vp, ctypes.POINTER(i32)], i32),
        'plsx_gen_splits': ([vp, i32, i32, i32, c_d, vp, ctypes.POINTER(i32), vp], i32),
        'plsx_gen_splits_seeded': ([vp, i32, i32, i32, c_d, vp, i32, vp], i32),
        'plsx_comm_load': ([vp, ctypes.c_char_p], i32),
        'plsx_comm_unique_id': ([vp, vp], i32),
        'plsx_comm_init': ([vp, vp, i32, i32], i32),
        'plsx_comm_rank': ([vp, ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
        'plsx_allgather': ([vp, vp, vp, ctypes.c_longlong, vp], i32),
        'plsx_comm_destroy': ([vp], i32),
        'plsx_comm_init_all': ([ctypes.POINTER(vp), i32, i32], i32),
        'plsx_comm_transport': ([vp], i32),
        'plsx_allgather_all': ([ctypes.POINTER(vp), i32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.c_longlong,
                                ctypes.POINTER(vp)], i32),
    }
    for name, (argtypes, restype) in sig.items():
        fn = getattr(lib, name)            # AttributeError if a symbol is missing
        fn.argtypes = argtypes
        fn.restype = restype
    _LIB = lib
    return lib


def exported_symbols():
    """Names declared in include/plsx.h that the loaded library exports."""
    lib = _load()
    names = ['plsx_version', 'plsx_max_tprime', 'plsx_ctx_create', 'plsx_ctx_destroy',
             'plsx_last_error', 'plsx_sync', 'plsx_set_data', 'plsx_num_lv', 'plsx_tprime',
             'plsx_crosscov_batch', 'plsx_scratch_read', 'plsx_decompose', 'plsx_set_original', 'plsx_set_contrasts', 'plsx_project',
             'plsx_colmean', 'plsx_perm_batch', 'plsx_perm_batch_y', 'plsx_crossval_batch', 'plsx_crossval_perm_batch', 'plsx_crossval_lv_batch', 'plsx_crossval_perm_lv_batch', 'plsx_residualize', 'plsx_set_confounds', 'plsx_crossval_confound_batch', 'plsx_crossval_confound_perm_batch', 'plsx_crossval_confound_group', 'plsx_boot_batch', 'plsx_boot_begin', 'plsx_boot_finish', 'plsx_boot_route', 'plsx_boot_keep', 'plsx_boot_weights_ci', 'plsx_perm_weights_build', 'plsx_perm_weights_test', 'plsx_perm_weights_scale', 'plsx_split_route', 'plsx_split_half_batch', 'plsx_split_half_batch_y',
             'plsx_boot_rel', 'plsx_last_timing', 'plsx_set_timing', 'plsx_kernel_timing',
             'plsx_kernel_class_name', 'plsx_set_perm_path', 'plsx_set_scratch', 'plsx_mfma_f64_peak',
             'plsx_percentile_ci', 'plsx_simpls_decompose', 'plsx_simpls_set_original', 'plsx_simpls_perm_batch',
             'plsx_simpls_boot_batch', 'plsx_simpls_set_row_masks', 'plsx_simpls_crossval_batch', 'plsx_simpls_crossval_perm_batch', 'plsx_simpls_crossval_nested_batch', 'plsx_simpls_crossval_nested_perm_batch', 'plsx_simpls_split_half_batch', 'plsx_simpls_set_confounds', 'plsx_simpls_crossval_confound_batch', 'plsx_simpls_crossval_confound_perm_batch', 'plsx_simpls_coef_begin', 'plsx_simpls_coef_finish', 'plsx_simpls_coef_keep', 'plsx_simpls_coef_ci', 'plsx_simpls_coef_perm_test', 'plsx_simpls_coef_perm_begin', 'plsx_simpls_coef_perm_end',
             'plsx_simpls_set_classes', 'plsx_simpls_cv_class_begin', 'plsx_simpls_cv_class_end',
             'plsx_simpls_cv_auc_begin', 'plsx_simpls_cv_auc_end', 'plsx_simpls_cv_pred_begin', 'plsx_simpls_cv_pred_end',
             'plsx_simpls_cvn_class_begin', 'plsx_simpls_cvn_class_end',
             'plsx_crossval_pred_begin', 'plsx_crossval_pred_end',
             'plsx_simpls_vip_keep', 'plsx_simpls_vip_ci', 'plsx_simpls_vip_perm_test', 'plsx_simpls_vip_perm_begin', 'plsx_simpls_vip_perm_end', 'plsx_gen_permsamp', 'plsx_gen_bootsamp',
             'plsx_gen_splits', 'plsx_gen_splits_seeded', 'plsx_gen_permsamp_stream',
             'plsx_gen_bootsamp_stream', 'plsx_set_option', 'plsx_option_name', 'plsx_numeric_report',
             'plsx_svd_flip', 'plsx_scale_columns', 'plsx_transpose', 'plsx_center_rows', 'plsx_mean_splits',
             'plsx_comm_load', 'plsx_comm_unique_id', 'plsx_comm_init', 'plsx_comm_rank', 'plsx_allgather',
             'plsx_comm_destroy', 'plsx_comm_init_all', 'plsx_comm_transport', 'plsx_allgather_all']
    return [n for n in names if hasattr(lib, n)]


def max_tprime():
    """Largest stacked dimension T' the library binds (plsx_max_tprime); no context, no device."""
    return int(_load().plsx_max_tprime())


def _torch():
    import torch
    return torch


def _virtual_indices(n, ci):
    """numpy's virtual indices (floor, fraction) of the two quantiles of a ``ci`` % interval over n values."""
    low = (100 - ci) / 2
    idx = []
    for q in (low, 100 - low):
        vi = (n - 1) * np.true_divide(q, 100)
        prev = np.floor(vi)
        idx.append((int(prev), float(vi - prev)))
    return idx


def option_names():
    """Keys of plsx_set_option (include/plsx.h)."""
    lib = _load()
    out, i = [], 0
    while True:
        name = lib.plsx_option_name(i)
        if not name:
            return out
        out.append(name.decode())
        i += 1


def options_from_env(environ=None):
    """``{'options': {...}, 'scratch_gb': ...}`` keyword arguments for :class:`Engine` from
    ``PLSX_<KEY>=<int>`` variables.  libplsx.so itself reads no environment variable and
    neither does the product path (``Engine()``, the front-ends): only bench.py, tools/ and
    the tests translate the environment -- so that one A/B command line or one monkeypatched
    test can select a kernel route -- through this helper."""
    environ = os.environ if environ is None else environ
    opts = {}
    for key in option_names():
        val = environ.get('PLSX_' + key.upper())
        if val is not None and val != '':
            try:
                opts[key] = int(val)
            except ValueError:
                opts[key] = 1
    kw = {'options': opts}
    if environ.get('PLSX_SCRATCH_GB'):
        kw['scratch_gb'] = float(environ['PLSX_SCRATCH_GB'])
    return kw


class GradedSpectrumWarning(UserWarning):
    """Resamples had live latent variables below 1e-5 of the largest singular value that the
    device could not refine on R (a dual-space route on data whose ORIGINAL spectrum was not graded;
    every feature-pass route refines, at every T'): their smallest LVs may miss the 1e-5 relative
    tolerance against an SVD of R (include/plsx.h, plsx_numeric_report)."""


def check_index_array(samples, S):
    """Row indices as the reference's fancy indexing ``X[inds]`` accepts them
    (pyls/base.py:569,599): integer dtype, negatives wrap like numpy's, anything
    outside [-S, S) raises IndexError.  The kernels index device memory with
    these values unchecked, so they are validated here."""
    samples = np.asarray(samples)
    if samples.dtype == bool or not np.issubdtype(samples.dtype, np.integer):
        raise IndexError('resampling arrays must hold integer row indices, got dtype {}'
                         .format(samples.dtype))
    if samples.size:
        lo, hi = int(samples.min()), int(samples.max())
        if lo < -S or hi >= S:
            raise IndexError('index {} is out of bounds for axis 0 with size {}'
                             .format(lo if lo < -S else hi, S))
        if lo < 0:
            samples = np.where(samples < 0, samples + S, samples)
    return samples


class Engine(object):
    """One device context.  All ndarray arguments / results are host numpy
    arrays unless a method says it returns a device tensor."""

    def __init__(self, device=None, scratch_gb=None, options=None):
        """``scratch_gb``: fixed super-batch scratch budget for a long-lived
        engine (steady-state throughput); None sizes the scratch per call
        (include/plsx.h, plsx_set_scratch).  ``options``: {key: int} route / layout
        switches for plsx_set_option (A/B measurements and tests; every route
        computes the same statistics)."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise PlsxError('no AMD GPU visible to PyTorch-ROCm: the PLS resampling engine has '
                            'no CPU fallback')
        self.lib = _load()
        if device is None:
            device = torch.cuda.current_device()
        self.device_index = int(device)
        self.device = torch.device('cuda', self.device_index)
        ctx = ctypes.c_void_p()
        rc = self.lib.plsx_ctx_create(self.device_index, ctypes.byref(ctx))
        if rc != 0:
            raise PlsxError('plsx_ctx_create failed with status {}'.format(rc))
        self.ctx = ctx
        # one analysis at a time per context: the context is not shared across host threads (include/plsx.h);
        # the front-ends hold this lock for the whole call, so two threads that call behavioral_pls /
        # pls_regression concurrently (they share the cached default engine) run one after the other
        self.lock = threading.RLock()
        self.S = self.B = self.L = self.Tp = 0
        self.refined = self.unrefined = 0
        if scratch_gb is not None:
            self._check(self.lib.plsx_set_scratch(self.ctx, float(scratch_gb), 1))
        for key, val in (options or {}).items():
            self.set_option(key, val)

    # -- plumbing ---------------------------------------------------------
    def close(self):
        if getattr(self, 'ctx', None):
            self.lib.plsx_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.plsx_last_error(self.ctx)
            raise PlsxError('libplsx status {}: {}'.format(rc, msg.decode() if msg else ''))

    def _stream(self):
        torch = _torch()
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, arr, dtype):
        torch = _torch()
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype))
        return t.to(self.device, non_blocking=False)

    def _empty(self, shape, dtype=None):
        torch = _torch()
        return torch.empty(shape, dtype=dtype or torch.float64, device=self.device)

    def _zeros(self, shape):
        torch = _torch()
        return torch.zeros(shape, dtype=torch.float64, device=self.device)

    def set_option(self, key, value=1):
        self._check(self.lib.plsx_set_option(self.ctx, str(key).encode(), int(value)))

    def sync(self):
        self._check(self.lib.plsx_sync(self.ctx))

    # -- the exported collective (include/plsx.h, "The collective") ---------
    def comm_load(self, path=None):
        """Bind the RCCL entry points.  Default: the librccl.so PyTorch-ROCm bundles (the copy this process
        already holds when a ``nccl`` process group exists), so that the process keeps ONE communication
        runtime."""
        if path is None:
            torch = _torch()
            cand = os.path.join(os.path.dirname(torch.__file__), 'lib', 'librccl.so')
            path = cand if os.path.exists(cand) else None
        self._check(self.lib.plsx_comm_load(self.ctx, path.encode() if path else None))

    def comm_unique_id(self):
        """128 bytes for :meth:`comm_init` (rank 0 draws them, every rank receives them through the launcher's
        own rendezvous)."""
        buf = ctypes.create_string_buffer(128)
        self._check(self.lib.plsx_comm_unique_id(self.ctx, buf))
        return bytes(buf.raw)

    def comm_init(self, uid, rank, world):
        """Collective over ``world`` ranks, one per GPU (ncclCommInitRank behind the C ABI)."""
        if len(uid) != 128:
            raise PlsxError('comm_init: the unique id is 128 bytes')
        self._check(self.lib.plsx_comm_init(self.ctx, ctypes.c_char_p(bytes(uid)), int(rank), int(world)))

    def comm_rank_world(self):
        r, w = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.plsx_comm_rank(self.ctx, ctypes.byref(r), ctypes.byref(w)))
        return r.value, w.value

    def comm_destroy(self):
        self._check(self.lib.plsx_comm_destroy(self.ctx))

    def allgather_into(self, send, recv):
        """recv (world, n) <- every rank's send (n,), on the current stream (plsx_allgather); contiguous device
        tensors of one dtype.  ``send`` may be ``recv[rank]``."""
        if not (send.is_contiguous() and recv.is_contiguous()) or send.dtype != recv.dtype:
            raise PlsxError('allgather_into: contiguous tensors of one dtype')
        nbytes = send.numel() * send.element_size()
        world = self.comm_rank_world()[1]
        if recv.numel() * recv.element_size() != nbytes * world:
            raise PlsxError('allgather_into: recv holds {} bytes, world {} x {} expected'.format(
                recv.numel() * recv.element_size(), world, nbytes))
        self._check(self.lib.plsx_allgather(self.ctx, send.data_ptr(), recv.data_ptr(), nbytes, self._stream()))
        return recv

    def numeric_report(self, warn=True, stacklevel=2):
        """(refined, unrefined) resample counts of graded spectra since the last call
        (plsx_numeric_report); warns when some could not be refined (``stacklevel``: whose line the warning
        is attributed to)."""
        a, b = ctypes.c_longlong(), ctypes.c_longlong()
        self._check(self.lib.plsx_numeric_report(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        self.refined += a.value
        self.unrefined += b.value
        if warn and b.value:
            import warnings
            warnings.warn('{} decomposition(s) had live latent variables below 1e-5 of the largest singular '
                          'value that could not be refined on the cross-covariance matrix (a dual-space route on '
                          'data whose original spectrum was not graded): singular values below ~6e-6 of the largest may differ from an '
                          'SVD of R by more than 1e-5 relative'.format(b.value), GradedSpectrumWarning,
                          stacklevel=stacklevel)
        return a.value, b.value

    def end_analysis(self, warn=True):
        """Close an analysis on this context, on the success AND on the error path of a front-end (it runs inside
        their ``finally``): forget the announced shard size (``expect_resamples``) and drain the refined / unrefined
        counters so that neither leaks into the next call.  It never warns itself -- a warning raised inside a
        ``finally`` would, under ``-W error``, replace the computed result: the count of unrefined
        decompositions is returned and the front-end warns AFTER its try block (:func:`warn_unrefined`), attributed to
        the user's call.  ``warn=False`` (an exception is already propagating): a failing device is not allowed to
        mask it."""
        try:
            self.set_option('expect_resamples', 0)
            return self.numeric_report(warn=False)[1]
        except PlsxError:
            if warn:
                raise
            return 0

    @staticmethod
    def warn_unrefined(n, stacklevel=3):
        """The GradedSpectrumWarning of an analysis that left ``n`` decompositions unrefined, attributed to the
        caller of the public front-end (stacklevel 3 from behavioral_pls / meancentered_pls / pls_regression's own
        frame: warn_unrefined <- run / pls_regression <- the public function <- USER)."""
        if n:
            import warnings
            warnings.warn('{} decomposition(s) had live latent variables below 1e-5 of the largest singular '
                          'value that could not be refined on the cross-covariance matrix (a dual-space route on '
                          'data whose original spectrum was not graded): singular values below ~6e-6 of the largest may differ from an '
                          'SVD of R by more than 1e-5 relative'.format(n), GradedSpectrumWarning, stacklevel=stacklevel)

    # -- data -------------------------------------------------------------
    def set_data(self, X, Y, cell_of_row, n_groups, n_cond, method, mean_centering=0,
                 covariance=False):
        """X (S, B), Y (S, T) or None: numpy arrays or device tensors."""
        torch = _torch()
        dX = X if isinstance(X, torch.Tensor) else self._dev(X, np.float64)
        dY = None
        if Y is not None:
            dY = Y if isinstance(Y, torch.Tensor) else self._dev(Y, np.float64)
        dC = self._dev(cell_of_row, np.int32)
        S, B = dX.shape
        T = 0 if dY is None else dY.shape[1]
        flags = PLSX_FLAG_COVARIANCE if covariance else 0
        self._check(self.lib.plsx_set_data(
            self.ctx, int(method), dX.data_ptr(), None if dY is None else dY.data_ptr(),
            dC.data_ptr(), S, B, T, int(n_groups), int(n_cond), int(mean_centering), flags,
            self._stream()))
        self.sync()
        self.S, self.B, self.T = S, B, T
        self.L = self.lib.plsx_num_lv(self.ctx)
        self.Tp = self.lib.plsx_tprime(self.ctx)

    def colmean(self):
        out = self._empty((self.B,))
        self._check(self.lib.plsx_colmean(self.ctx, out.data_ptr(), self._stream()))
        self.sync()
        return out.cpu().numpy()

    def _index_rows(self, samples):
        """(S, n) reference layout -> (n, S) int32 device tensor."""
        samples = np.asarray(samples)
        if samples.ndim != 2 or samples.shape[0] != self.S:
            raise ValueError('resampling array must have shape (S, n) with S = {}; got {}'
                             .format(self.S, samples.shape))
        return self._dev(check_index_array(samples, self.S).T, np.int32)

    # -- kernels ----------------------------------------------------------
    def crosscov(self, xsrc=None, ysrc=None, n=None):
        """gen_covcorr of n resamples; xsrc / ysrc (S, n) or None (identity)."""
        dx = None if xsrc is None else self._index_rows(xsrc)
        dy = None if ysrc is None else self._index_rows(ysrc)
        if n is None:
            n = (dx if dx is not None else dy).shape[0] if (dx is not None or dy is not None) else 1
        out = self._empty((n, self.Tp, self.B))
        self._check(self.lib.plsx_crosscov_batch(
            self.ctx, None if dx is None else dx.data_ptr(), None if dy is None else dy.data_ptr(),
            int(n), out.data_ptr(), self._stream()))
        self.sync()
        return out.cpu().numpy()

    def scratch_rows(self, slot, row0=0, nrows=None):
        """Rows of one resample's slot of the cross-product scratch as the last batch left them (plsx_scratch_read;
        tests): (nrows, Bpad) with the B features, the L score columns, zero padding; T' rounded up to 4 rows."""
        tpp, bpad = -(-self.Tp // 4) * 4, -(-(self.B + self.L) // 128) * 128
        nrows = tpp - row0 if nrows is None else nrows
        out = self._empty((nrows, bpad))
        self._check(self.lib.plsx_scratch_read(self.ctx, int(slot), int(row0), int(nrows), out.data_ptr(),
                                               self._stream()))
        self.sync()
        return out.cpu().numpy()

    def decompose(self):
        """-> x_weights (B, L), singvals (L,), y_weights (T', L), raw signs."""
        xw, sv, yw = self._empty((self.B, self.L)), self._empty((self.L,)), self._empty((self.Tp, self.L))
        self._check(self.lib.plsx_decompose(self.ctx, xw.data_ptr(), sv.data_ptr(), yw.data_ptr(),
                                            self._stream()))
        self.sync()
        return xw.cpu().numpy(), sv.cpu().numpy(), yw.cpu().numpy()

    def set_contrasts(self, V=None):
        """Non-rotated PLS (plsx_set_contrasts): V (T', Lc) with unit columns, after :meth:`set_data`; None returns
        the context to SVD mode.  decompose / set_original follow; results keep L columns, those >= Lc are zero."""
        if V is None:
            self._check(self.lib.plsx_set_contrasts(self.ctx, None, 0, self._stream()))
            return
        V = np.asarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != self.Tp or not 1 <= V.shape[1] <= self.L:
            raise ValueError('contrasts must have shape ({}, Lc) with 1 <= Lc <= {}; got {}'
                             .format(self.Tp, self.L, V.shape))
        d = self._dev(V, np.float64)
        self._check(self.lib.plsx_set_contrasts(self.ctx, d.data_ptr(), int(V.shape[1]), self._stream()))

    def _as_dev(self, a):
        """numpy array or device tensor -> contiguous fp64 device tensor."""
        torch = _torch()
        if isinstance(a, torch.Tensor):
            return a if (a.is_cuda and a.is_contiguous() and a.dtype == torch.float64) else \
                a.to(self.device, dtype=torch.float64).contiguous()
        return self._dev(a, np.float64)

    def set_original(self, x_weights, singvals, y_weights):
        """Arguments: numpy arrays or device tensors (the device-resident front-end passes what
        decompose_dev / svd_flip left on the device: no host round trip of the (B, L) weights)."""
        self._orig_xw = self._as_dev(x_weights)
        sv, yw = self._as_dev(singvals), self._as_dev(y_weights)
        self._check(self.lib.plsx_set_original(self.ctx, self._orig_xw.data_ptr(), sv.data_ptr(),
                                               yw.data_ptr(), self._stream()))
        self.sync()

    # -- device-resident pieces of the front-end (tensors in, tensors out; no host copies) ------
    def colmean_dev(self):
        out = self._empty((self.B,))
        self._check(self.lib.plsx_colmean(self.ctx, out.data_ptr(), self._stream()))
        return out

    def decompose_dev(self):
        """-> x_weights (B, L), singvals (L,), y_weights (T', L) device tensors, raw signs."""
        xw, sv, yw = self._empty((self.B, self.L)), self._empty((self.L,)), self._empty((self.Tp, self.L))
        self._check(self.lib.plsx_decompose(self.ctx, xw.data_ptr(), sv.data_ptr(), yw.data_ptr(),
                                            self._stream()))
        return xw, sv, yw

    def svd_flip(self, xw, yw):
        """sklearn's svd_flip as compute.svd applies it (pyls/compute.py:43-50), in place on device tensors."""
        self._check(self.lib.plsx_svd_flip(self.ctx, xw.data_ptr(), yw.data_ptr(), self._stream()))

    def project_dev(self, W):
        """(X - colmean) @ W for a device tensor W (B, L) -> device tensor (S, L)."""
        out = self._empty((self.S, W.shape[1]))
        self._check(self.lib.plsx_project(self.ctx, W.data_ptr(), W.shape[1], out.data_ptr(), self._stream()))
        return out

    def scale_columns(self, A, scale):
        """A (rows, cols) * scale (cols,) on the device -> new tensor."""
        out = self._empty(tuple(A.shape))
        self._check(self.lib.plsx_scale_columns(self.ctx, A.data_ptr(), A.shape[0], A.shape[1], scale.data_ptr(),
                                                out.data_ptr(), self._stream()))
        return out

    def transpose_dev(self, A):
        """(rows, cols) device tensor -> (cols, rows) device tensor."""
        out = self._empty((A.shape[1], A.shape[0]))
        self._check(self.lib.plsx_transpose(self.ctx, A.data_ptr(), A.shape[0], A.shape[1], out.data_ptr(),
                                            self._stream()))
        return out

    def boot_rel_dev(self, orig, usum, usq, n_boot, add_orig=False):
        """compute.boot_rel on device tensors -> (bsr, se) device tensors, no sync."""
        bsr, se = self._empty(tuple(usum.shape)), self._empty(tuple(usum.shape))
        self._check(self.lib.plsx_boot_rel(self.ctx, orig.data_ptr(), usum.data_ptr(), usq.data_ptr(),
                                           int(n_boot), 1 if add_orig else 0, usum.numel(),
                                           bsr.data_ptr(), se.data_ptr(), self._stream()))
        return bsr, se

    def percentile_ci_dev(self, series, ci=95):
        """compute.boot_ci of (nseries, n) contiguous device series -> (lo, hi) device tensors, or None when
        n exceeds the device sort (16384): the caller falls back to numpy on the host copy."""
        n = series.shape[-1]
        if n > 16384:
            return None
        low = (100 - ci) / 2
        idx = []
        for q in (low, 100 - low):                      # numpy's virtual index of the quantile
            vi = (n - 1) * np.true_divide(q, 100)
            prev = np.floor(vi)
            idx.append((int(prev), float(vi - prev)))
        lo, hi = self._empty((series.shape[0],)), self._empty((series.shape[0],))
        self._check(self.lib.plsx_percentile_ci(self.ctx, series.data_ptr(), series.shape[0], n, idx[0][0], idx[0][1],
                                                idx[1][0], idx[1][1], lo.data_ptr(), hi.data_ptr(), self._stream()))
        return lo, hi

    def pinned_like(self, t):
        """Page-locked host tensor of the shape of device tensor ``t`` (the destination of an asynchronous D2H
        copy; 56 us per MB to map -- call it while the device is busy)."""
        torch = _torch()
        return torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)

    def to_host_async(self, t, pinned=None):
        """Start the D2H copy of ``t`` into page-locked memory on the current stream; the numpy view of the
        returned tensor is valid after the next sync."""
        if pinned is None:
            pinned = self.pinned_like(t)
        pinned.copy_(t, non_blocking=True)
        return pinned

    def project(self, W):
        """(X - colmean) @ W for W (B, L) -> (S, L)."""
        dW = self._dev(W, np.float64)
        out = self._empty((self.S, dW.shape[1]))
        self._check(self.lib.plsx_project(self.ctx, dW.data_ptr(), dW.shape[1], out.data_ptr(),
                                          self._stream()))
        self.sync()
        return out.cpu().numpy()

    def perm(self, permsamples, rotate=True):
        """permsamples (S, P) -> permuted singular values (L, P)."""
        idx = self._index_rows(permsamples)
        n = idx.shape[0]
        out = self._empty((n, self.L))
        self._check(self.lib.plsx_perm_batch(self.ctx, idx.data_ptr(), n, 1 if rotate else 0,
                                             out.data_ptr(), self._stream()))
        self.sync()
        return out.cpu().numpy().T.copy()

    def perm_ystack(self, ystack, rotate=True):
        """ystack (n, S, T): pre-permuted Y matrices -> permuted singular values (L, n)."""
        ystack = np.asarray(ystack, dtype=np.float64)
        if ystack.ndim != 3 or ystack.shape[1] != self.S or ystack.shape[2] != self.T:
            raise ValueError('pre-permuted Y stack must have shape (n, {}, {}); got {}'
                             .format(self.S, self.T, ystack.shape))
        d = self._dev(ystack, np.float64)
        out = self._empty((ystack.shape[0], self.L))
        self._check(self.lib.plsx_perm_batch_y(self.ctx, d.data_ptr(), ystack.shape[0],
                                               1 if rotate else 0, out.data_ptr(), self._stream()))
        self.sync()
        return out.cpu().numpy().T.copy()

    def boot(self, bootsamples, usum=None, usq=None):
        """bootsamples (S, R) -> (usum, usq) device tensors (B, L), accumulated in
        place when given, and distrib (T', L, R) numpy."""
        idx = self._index_rows(bootsamples)
        n = idx.shape[0]
        if usum is None:
            usum, usq = self._zeros((self.B, self.L)), self._zeros((self.B, self.L))
        dist = self._empty((n, self.Tp, self.L))
        self.boot_begin(n)                       # a series of one call
        self._check(self.lib.plsx_boot_batch(self.ctx, idx.data_ptr(), n, usum.data_ptr(),
                                             usq.data_ptr(), dist.data_ptr(), self._stream()))
        self.boot_finish(usum, usq)
        self.sync()
        return usum, usq, np.ascontiguousarray(dist.cpu().numpy().transpose(1, 2, 0))

    def split_half(self, masks, perms=None, ystack=None, mask_rows=False):
        """Per-split correlations.  masks (np, S, ns) bool: one (S, ns) gen_splits
        array per arrangement; perms (S, np) index array, or ystack (np, S, T)
        pre-permuted behaviour matrices, or neither (original data).
        Returns ucorr, vcorr of shape (np, L, ns)."""
        torch = _torch()
        masks = np.asarray(masks)
        if masks.ndim == 2:
            masks = masks[None]
        if mask_rows:                                   # (np, ns, S) uint8 as the device consumes them
            n_arr, ns, S = masks.shape
        else:
            n_arr, S, ns = masks.shape
        if S != self.S:
            raise ValueError('split masks must have S = {} rows'.format(self.S))
        if mask_rows:
            dm = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.uint8)).to(self.device)
        else:
            dm = torch.from_numpy(np.ascontiguousarray(masks.transpose(0, 2, 1), dtype=np.uint8)).to(self.device)
        dp = None
        if perms is not None:
            dp = self._index_rows(perms)
            if dp.shape[0] != n_arr:
                raise ValueError('need one permutation per arrangement')
        dy = None
        if ystack is not None:
            dy = self._dev(ystack, np.float64)
            if tuple(dy.shape) != (n_arr, self.S, self.T) or dp is not None:
                raise ValueError('ystack must have shape ({}, {}, {}) and excludes perms'
                                 .format(n_arr, self.S, self.T))
        uc, vc = self._empty((n_arr, ns, self.L)), self._empty((n_arr, ns, self.L))
        self._check(self.lib.plsx_split_half_batch_y(
            self.ctx, None if dp is None else dp.data_ptr(), None if dy is None else dy.data_ptr(), n_arr,
            dm.data_ptr(), ns, uc.data_ptr(), vc.data_ptr(), self._stream()))
        self.sync()
        return (np.ascontiguousarray(uc.cpu().numpy().transpose(0, 2, 1)),
                np.ascontiguousarray(vc.cpu().numpy().transpose(0, 2, 1)))

    def split_route(self):
        """1 when the last split-half pass took the one-pass reader over raw first-half sums (plsx_split_route)."""
        return int(self.lib.plsx_split_route(self.ctx))

    def crossval(self, splits, lv=False):
        """splits (S, m) bool, True = training row -> pearson_r, r_squared (T, m); with ``lv`` also lv_corr (L, m), the
        out-of-sample score correlation of every latent variable from the same pass (plsx_crossval_lv_batch)."""
        torch = _torch()
        splits = np.asarray(splits)
        if splits.ndim != 2 or splits.shape[0] != self.S:
            raise ValueError('split masks must have shape (S, m) with S = {}'.format(self.S))
        dm = torch.from_numpy(np.ascontiguousarray(splits.T, dtype=np.uint8)).to(self.device)
        m = dm.shape[0]
        r, r2 = self._empty((m, self.T)), self._empty((m, self.T))
        if lv:
            c = self._empty((m, self.L))
            self._check(self.lib.plsx_crossval_lv_batch(self.ctx, dm.data_ptr(), m, r.data_ptr(), r2.data_ptr(),
                                                        c.data_ptr(), self._stream()))
            self.sync()
            return r.cpu().numpy().T.copy(), r2.cpu().numpy().T.copy(), c.cpu().numpy().T.copy()
        self._check(self.lib.plsx_crossval_batch(self.ctx, dm.data_ptr(), m, r.data_ptr(), r2.data_ptr(),
                                                 self._stream()))
        self.sync()
        return r.cpu().numpy().T.copy(), r2.cpu().numpy().T.copy()

    def crossval_pred_begin(self, pred_dev, true_dev=None):
        """Open a series of out-of-fold predictions: until :meth:`crossval_pred_end` every :meth:`crossval` /
        :meth:`crossval_confound` of m splits appends m slots (T, S) to ``pred_dev`` (capacity, T, S) float64 in
        submission order -- the prediction of the test rows of the split, NaN on its training rows -- and to
        ``true_dev``, where given, the observed rows at the same positions (plsx_crossval_pred_begin).  The tensors
        must stay alive until the series ends.  PlsxError: status -1 from the call that would pass the capacity, -2
        (context still usable) for a stack beyond the scratch budget."""
        torch = _torch()
        for t in (pred_dev, true_dev):
            if t is not None and (t.dim() != 3 or tuple(t.shape[1:]) != (self.T, self.S) or t.dtype != torch.float64
                                  or not t.is_contiguous() or t.shape[0] != pred_dev.shape[0]):
                raise ValueError('the stacks of predictions must be contiguous (capacity, {}, {}) float64 tensors'
                                 .format(self.T, self.S))
        self._check(self.lib.plsx_crossval_pred_begin(self.ctx, pred_dev.data_ptr(),
                                                      true_dev.data_ptr() if true_dev is not None else None,
                                                      int(pred_dev.shape[0])))

    def crossval_pred_end(self):
        """Close the series of out-of-fold predictions (plsx_crossval_pred_end)."""
        self._check(self.lib.plsx_crossval_pred_end(self.ctx))

    def crossval_perm_into(self, masks_dev, idx_dev, r_dev, r2_dev, lv_dev=None, lv_pairs_dev=None):
        """Device form of :meth:`crossval_perm`: masks (n, S) uint8, index rows (m, S) int32 -> r, r2 (m, T), the means
        over the n splits (plsx_crossval_perm_batch).  Pass all of the caller's permutations at once: every split's
        S x S matrix is formed once per call.  ``lv_dev`` (m, L): also the split means of the score correlations of
        the latent variables, ``lv_pairs_dev`` (m, n, L) their (permutation, split) values
        (plsx_crossval_perm_lv_batch)."""
        n, m = masks_dev.shape[0], idx_dev.shape[0]
        if lv_dev is None:
            self._check(self.lib.plsx_crossval_perm_batch(self.ctx, masks_dev.data_ptr(), n, idx_dev.data_ptr(), m,
                                                          r_dev.data_ptr(), r2_dev.data_ptr(), self._stream()))
            return
        self._check(self.lib.plsx_crossval_perm_lv_batch(
            self.ctx, masks_dev.data_ptr(), n, idx_dev.data_ptr(), m, r_dev.data_ptr(), r2_dev.data_ptr(),
            lv_dev.data_ptr(), None if lv_pairs_dev is None else lv_pairs_dev.data_ptr(), self._stream()))

    def crossval_perm_lv(self, splits, perms):
        """:meth:`crossval_perm` with the score correlations of the latent variables -> perm_pearson_r, perm_r_squared
        (T, m), perm_lv_corr (L, m) the split means, and the (permutation, split) values (L, m, n)."""
        torch = _torch()
        splits = np.asarray(splits)
        if splits.ndim != 2 or splits.shape[0] != self.S:
            raise ValueError('split masks must have shape (S, n) with S = {}'.format(self.S))
        idx = check_index_array(np.asarray(perms), self.S)
        dm = torch.from_numpy(np.ascontiguousarray(splits.T, dtype=np.uint8)).to(self.device)
        di = torch.from_numpy(np.ascontiguousarray(idx.T, dtype=np.int32)).to(self.device)
        m, n = di.shape[0], dm.shape[0]
        r, r2 = self._empty((m, self.T)), self._empty((m, self.T))
        c, pairs = self._empty((m, self.L)), self._empty((m, n, self.L))
        self.crossval_perm_into(dm, di, r, r2, c, pairs)
        self.sync()
        return (r.cpu().numpy().T.copy(), r2.cpu().numpy().T.copy(), c.cpu().numpy().T.copy(),
                np.ascontiguousarray(pairs.cpu().numpy().transpose(2, 0, 1)))

    def crossval_perm(self, splits, perms):
        """Permutation null of the cross-validation: splits (S, n) bool, True = training row; perms (S, m), one
        permutation of 0 .. S-1 per column -> perm_pearson_r, perm_r_squared (T, m): for every permutation of the rows
        of Y the scores of :meth:`crossval` under the same splits, averaged over the splits."""
        torch = _torch()
        splits = np.asarray(splits)
        if splits.ndim != 2 or splits.shape[0] != self.S:
            raise ValueError('split masks must have shape (S, n) with S = {}'.format(self.S))
        idx = check_index_array(np.asarray(perms), self.S)
        dm = torch.from_numpy(np.ascontiguousarray(splits.T, dtype=np.uint8)).to(self.device)
        di = torch.from_numpy(np.ascontiguousarray(idx.T, dtype=np.int32)).to(self.device)
        m = di.shape[0]
        r, r2 = self._empty((m, self.T)), self._empty((m, self.T))
        self.crossval_perm_into(dm, di, r, r2)
        self.sync()
        return r.cpu().numpy().T.copy(), r2.cpu().numpy().T.copy()

    # -- confound regression of behavioural PLS -------------------------------
    def residualize(self, A, Z, slopes=True):
        """A (S, n) device tensor (contiguous) <- its residuals on [1, Z - zbar], Z (S, q) numpy or device tensor, in
        place (plsx_residualize: stateless, before :meth:`set_data`) -> the slopes on Z - zbar (q, n) as a device
        tensor, or None.  PlsxError (status -1) for rank deficient confounds: nothing is written."""
        torch = _torch()
        dZ = Z if isinstance(Z, torch.Tensor) else self._dev(np.ascontiguousarray(Z, dtype=np.float64), np.float64)
        if A.dim() != 2 or not A.is_contiguous() or dZ.dim() != 2 or dZ.shape[0] != A.shape[0]:
            raise ValueError('residualize takes a contiguous (S, n) tensor and confounds (S, q)')
        S, n = A.shape
        g = self._empty((dZ.shape[1], n)) if slopes else None
        self._check(self.lib.plsx_residualize(self.ctx, A.data_ptr(), n, n, S, dZ.data_ptr(), int(dZ.shape[1]),
                                              None if g is None else g.data_ptr(), n, self._stream()))
        return g

    def set_confounds(self, Z):
        """Binds Z (S, q) for :meth:`crossval_confound` / :meth:`crossval_confound_perm_into` (plsx_set_confounds; a
        behavioural binding, after :meth:`set_data`, which clears it)."""
        torch = _torch()
        dZ = Z if isinstance(Z, torch.Tensor) else self._dev(np.ascontiguousarray(Z, dtype=np.float64), np.float64)
        if dZ.dim() != 2 or dZ.shape[0] != self.S:
            raise ValueError('confounds must have shape ({}, q); got {}'.format(self.S, tuple(dZ.shape)))
        self._check(self.lib.plsx_set_confounds(self.ctx, dZ.data_ptr(), int(dZ.shape[1]), self._stream()))

    def crossval_confound(self, splits, lv=False):
        """:meth:`crossval` with the confound regression fitted on the training rows of every split and applied to
        all its rows (plsx_crossval_confound_batch; after :meth:`set_confounds`)."""
        torch = _torch()
        splits = np.asarray(splits)
        if splits.ndim != 2 or splits.shape[0] != self.S:
            raise ValueError('split masks must have shape (S, m) with S = {}'.format(self.S))
        dm = torch.from_numpy(np.ascontiguousarray(splits.T, dtype=np.uint8)).to(self.device)
        m = dm.shape[0]
        r, r2 = self._empty((m, self.T)), self._empty((m, self.T))
        c = self._empty((m, self.L)) if lv else None
        self._check(self.lib.plsx_crossval_confound_batch(self.ctx, dm.data_ptr(), m, r.data_ptr(), r2.data_ptr(),
                                                          None if c is None else c.data_ptr(), self._stream()))
        self.sync()
        out = (r.cpu().numpy().T.copy(), r2.cpu().numpy().T.copy())
        return out + (c.cpu().numpy().T.copy(),) if lv else out

    def crossval_confound_perm_into(self, masks_dev, idx_dev, r_dev, r2_dev, lv_dev=None, lv_pairs_dev=None):
        """:meth:`crossval_perm_into` under the fold-wise confound regression: the residualised Y is permuted and
        residualised again per fold (plsx_crossval_confound_perm_batch)."""
        n, m = masks_dev.shape[0], idx_dev.shape[0]
        self._check(self.lib.plsx_crossval_confound_perm_batch(
            self.ctx, masks_dev.data_ptr(), n, idx_dev.data_ptr(), m, r_dev.data_ptr(), r2_dev.data_ptr(),
            None if lv_dev is None else lv_dev.data_ptr(), None if lv_pairs_dev is None else lv_pairs_dev.data_ptr(),
            self._stream()))

    def crossval_confound_perm(self, splits, perms, lv=False):
        """:meth:`crossval_perm` (``lv``: :meth:`crossval_perm_lv` without the pairs) under the fold-wise confound
        regression."""
        torch = _torch()
        splits = np.asarray(splits)
        if splits.ndim != 2 or splits.shape[0] != self.S:
            raise ValueError('split masks must have shape (S, n) with S = {}'.format(self.S))
        idx = check_index_array(np.asarray(perms), self.S)
        dm = torch.from_numpy(np.ascontiguousarray(splits.T, dtype=np.uint8)).to(self.device)
        di = torch.from_numpy(np.ascontiguousarray(idx.T, dtype=np.int32)).to(self.device)
        m = di.shape[0]
        r, r2 = self._empty((m, self.T)), self._empty((m, self.T))
        c = self._empty((m, self.L)) if lv else None
        self.crossval_confound_perm_into(dm, di, r, r2, c)
        self.sync()
        out = (r.cpu().numpy().T.copy(), r2.cpu().numpy().T.copy())
        return out + (c.cpu().numpy().T.copy(),) if lv else out

    def crossval_confound_group(self):
        """Splits per group of fold copies of the last fold-wise call (plsx_crossval_confound_group)."""
        return int(self.lib.plsx_crossval_confound_group(self.ctx))

    # -- SIMPLS regression ---------------------------------------------------
    def set_data_regression(self, Xc, Yc, n_components):
        """Xc (S, B), Yc (S, T): globally column-centred data."""
        self.set_data(Xc, Yc, np.zeros(len(Xc), np.int32), 1, int(n_components), PLSX_REGRESSION)
        self.k = int(n_components)

    def simpls_decompose(self):
        """-> x_weights (B, k), pctvar_y (k,), cvec (T, k), y_loadings (T, k)."""
        xwT, pct = self._empty((self.k, self.B)), self._empty((self.k,))
        cv, yl = self._empty((self.T, self.k)), self._empty((self.T, self.k))
        self._check(self.lib.plsx_simpls_decompose(self.ctx, xwT.data_ptr(), pct.data_ptr(), cv.data_ptr(),
                                                   yl.data_ptr(), self._stream()))
        self.sync()
        return (np.ascontiguousarray(xwT.cpu().numpy().T), pct.cpu().numpy(), cv.cpu().numpy(),
                yl.cpu().numpy())

    def simpls_decompose_dev(self):
        """The original SIMPLS fit with everything B-sized left on the device and the sign rule of compute.svd applied
        there (plsx_svd_flip): -> x_weights (B, k) DEVICE tensor, pctvar_y (k,) numpy, y_loadings (T, k) numpy."""
        xwT, pct = self._empty((self.k, self.B)), self._empty((self.k,))
        cv, yl = self._empty((self.T, self.k)), self._empty((self.T, self.k))
        self._check(self.lib.plsx_simpls_decompose(self.ctx, xwT.data_ptr(), pct.data_ptr(), cv.data_ptr(),
                                                   yl.data_ptr(), self._stream()))
        W = self.transpose_dev(xwT)
        self.svd_flip(W, cv)
        return W, pct.cpu().numpy(), yl.cpu().numpy()

    def simpls_set_original_dev(self, W):
        """simpls_set_original for a device tensor W (B, k): transposed and column-centred on the device."""
        wT = self.transpose_dev(W)
        self._check(self.lib.plsx_center_rows(self.ctx, wT.data_ptr(), wT.shape[0], wT.shape[1], wT.data_ptr(),
                                              self._stream()))
        self._check(self.lib.plsx_simpls_set_original(self.ctx, wT.data_ptr(), self._stream()))
        self.sync()                                   # (wT is released on return)

    def simpls_set_original(self, x_weights):
        w0c = np.asarray(x_weights) - np.asarray(x_weights).mean(axis=0, keepdims=True)
        d = self._dev(w0c.T, np.float64)
        self._check(self.lib.plsx_simpls_set_original(self.ctx, d.data_ptr(), self._stream()))
        self.sync()

    def simpls_perm(self, permsamples):
        """permsamples (S, P) -> pctvar of Y per permutation (k, P)."""
        idx = self._index_rows(permsamples)
        out = self._empty((idx.shape[0], self.k))
        self._check(self.lib.plsx_simpls_perm_batch(self.ctx, idx.data_ptr(), idx.shape[0], out.data_ptr(),
                                                    self._stream()))
        self.sync()
        return out.cpu().numpy().T.copy()

    def simpls_set_row_masks(self, okx=None, oky=None):
        """okx / oky (S,) bool: usable rows of X / Y (all-NaN rows are False)."""
        torch = _torch()
        dx = None if okx is None else torch.from_numpy(np.ascontiguousarray(okx, dtype=np.uint8)).to(self.device)
        dy = None if oky is None else torch.from_numpy(np.ascontiguousarray(oky, dtype=np.uint8)).to(self.device)
        self._check(self.lib.plsx_simpls_set_row_masks(
            self.ctx, None if dx is None else dx.data_ptr(), None if dy is None else dy.data_ptr(),
            self._stream()))
        self.sync()

    def simpls_boot(self, bootsamples, usum=None, usq=None, ystack=None):
        """-> usum, usq device tensors (B, k) (accumulated in place when given)
        and y_loadings_boot (T, k, R).  ystack (R, S, T): one Y per bootstrap."""
        idx = self._index_rows(bootsamples)
        n = idx.shape[0]
        if usum is None:
            usum, usq = self._zeros((self.B, self.k)), self._zeros((self.B, self.k))
        dys = None
        if ystack is not None:
            dys = self._dev(ystack, np.float64)
            if tuple(dys.shape) != (n, self.S, self.T):
                raise ValueError('ystack must have shape ({}, {}, {})'.format(n, self.S, self.T))
        yl = self._empty((n, self.T, self.k))
        self.boot_begin(n)                       # a series of one call
        self._check(self.lib.plsx_simpls_boot_batch(
            self.ctx, idx.data_ptr(), None if dys is None else dys.data_ptr(), n, usum.data_ptr(),
            usq.data_ptr(), yl.data_ptr(), self._stream()))
        self.boot_finish(usum, usq)
        self.sync()
        return usum, usq, np.ascontiguousarray(yl.cpu().numpy().transpose(1, 2, 0))

    # -- device-resident variants (no host copies, no sync): bench / pipelines --
    def index_tensor(self, samples):
        """(S, n) host index array -> (n, S) int32 device tensor."""
        return self._index_rows(samples)

    def rows_tensor(self, rows):
        """(n, S) int32 host rows (one resample per row, already validated) -> device tensor."""
        torch = _torch()
        return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)

    def perm_into(self, idx_dev, out_dev, rotate=True):
        """idx_dev (n, S) int32 device tensor, out_dev (n, L) fp64 device tensor."""
        self._check(self.lib.plsx_perm_batch(self.ctx, idx_dev.data_ptr(), idx_dev.shape[0],
                                             1 if rotate else 0, out_dev.data_ptr(), self._stream()))

    def boot_begin(self, n_total):
        """Announce a series of n_total bootstraps accumulating into one (usum, usq) (include/plsx.h,
        plsx_boot_begin).  Returns 1 when the library moved the pass over the features out of the loop (the
        quadratic-form route: the batches then leave usum / usq alone until boot_finish), 0 otherwise."""
        self._check(self.lib.plsx_boot_begin(self.ctx, int(n_total), self._stream()))
        return int(self.lib.plsx_boot_route(self.ctx))

    def boot_finish(self, usum, usq):
        """Close the series: adds what it still owes usum / usq (a no-op on the in-place route)."""
        self._check(self.lib.plsx_boot_finish(self.ctx, usum.data_ptr(), usq.data_ptr(), self._stream()))

    def boot_into(self, idx_dev, usum, usq, dist_dev):
        """idx_dev (n, S) int32; usum / usq (B, L) accumulated in place; dist_dev
        (n, T', L)."""
        self._check(self.lib.plsx_boot_batch(self.ctx, idx_dev.data_ptr(), idx_dev.shape[0],
                                             usum.data_ptr(), usq.data_ptr(), dist_dev.data_ptr(),
                                             self._stream()))

    def boot_keep(self, stack=None):
        """Have every :meth:`boot_into` that follows also keep the bootstrap's rotation operand: ``stack`` (capacity, m,
        T'), a contiguous float64 tensor on this device, receives the first m columns of M_b, transposed, in submission
        order (plsx_boot_keep).  ``None`` ends the keeping.  PlsxError: status -4 without bound PLS-C data and a set
        original, -2 with contrasts or multiblock data, -1 from the batch that would overflow the stack."""
        if stack is None:
            self._check(self.lib.plsx_boot_keep(self.ctx, None, 0, 0))
            return
        torch = _torch()
        if stack.dim() != 3 or stack.shape[2] != self.Tp or stack.dtype != torch.float64 or not stack.is_contiguous():
            raise ValueError('the kept stack must be a contiguous (capacity, m, {}) float64 tensor'.format(self.Tp))
        self._check(self.lib.plsx_boot_keep(self.ctx, stack.data_ptr(), int(stack.shape[0]), int(stack.shape[1])))

    def boot_weights_ci(self, idx_dev, stack, ci=95):
        """Percentile interval of the rotated bootstrap weights: ``idx_dev`` (n, S) int32 index rows and ``stack`` (n, m,
        T') -- a kept stack, the gathered stacks of several ranks, or any contiguous float64 device tensor of that shape
        -> (lo, hi) device tensors (B, m), ``np.percentile(U_boot[:, :m], [(100 - ci) / 2, 100 - (100 - ci) / 2],
        axis=-1)`` of the (B, L, n) series of ``single_boot(...)[1]``, in the units of ``x_weights @ diag(singvals)``,
        without that array ever existing (plsx_boot_weights_ci).  No sync.  PlsxError status -2 (context still usable)
        for n > 16384 or a stack that does not fit the scratch budget."""
        torch = _torch()
        if stack.dim() != 3 or stack.shape[2] != self.Tp or stack.dtype != torch.float64 or not stack.is_contiguous():
            raise ValueError('the stack must be a contiguous (n, m, {}) float64 tensor'.format(self.Tp))
        n, m = int(stack.shape[0]), int(stack.shape[1])
        if tuple(idx_dev.shape) != (n, self.S) or idx_dev.dtype != torch.int32 or not idx_dev.is_contiguous():
            raise ValueError('the index rows must be a contiguous ({}, {}) int32 tensor'.format(n, self.S))
        idx = _virtual_indices(max(n, 1), ci)
        lo, hi = self._empty((self.B, max(m, 1))), self._empty((self.B, max(m, 1)))
        self._check(self.lib.plsx_boot_weights_ci(self.ctx, idx_dev.data_ptr(), stack.data_ptr(), n, m, idx[0][0],
                                                  idx[0][1], idx[1][0], idx[1][1], lo.data_ptr(), hi.data_ptr(),
                                                  self._stream()))
        return lo, hi

    def _check_perm_weights(self, idx_dev, V):
        """The operands both permutation entries of the x_weights share -> (n, m)."""
        torch = _torch()
        if V.dim() != 2 or V.shape[0] != self.Tp or V.dtype != torch.float64 or not V.is_contiguous():
            raise ValueError('the pattern V must be a contiguous ({}, m) float64 tensor'.format(self.Tp))
        if idx_dev.dim() != 2 or idx_dev.shape[1] != self.S or idx_dev.dtype != torch.int32 \
                or not idx_dev.is_contiguous():
            raise ValueError('the index rows must be a contiguous (n, {}) int32 tensor'.format(self.S))
        # (the builders index device memory with these values unchecked)
        if idx_dev.numel() and not (int(idx_dev.min()) >= 0 and int(idx_dev.max()) < self.S):
            raise IndexError('the index rows must hold row indices in 0 .. {}'.format(self.S - 1))
        return int(idx_dev.shape[0]), int(V.shape[1])

    def perm_weights_build(self, idx_dev, V):
        """The subject-space operands of the permutation null of the x_weights: ``idx_dev`` (n, S) int32 index rows,
        ``V`` (T', m) the observed pattern -> W (n, m, S) device tensor with ``W[p] @ Xf == (R_p.T @ V).T``, R_p the
        cross-covariance matrix of permutation p and Xf the resample-independent feature matrix of the binding: the
        per-cell scaled X in correlation mode, else the centred X (plsx_perm_weights_build).  No sync.  PlsxError status
        -4 without bound PLS-C data, -2 for multiblock data, -1 for m outside 1 .. T'."""
        n, m = self._check_perm_weights(idx_dev, V)
        W = self._empty((max(n, 1), max(m, 1), self.S))
        self._check(self.lib.plsx_perm_weights_build(self.ctx, idx_dev.data_ptr(), n, V.data_ptr(), m, W.data_ptr(),
                                                     self._stream()))
        return W

    def perm_weights_test(self, idx_dev, V, obs, count, dmax, standardise=False):
        """The permutation statistics of the x_weights along ``V`` (T', m) for the index rows ``idx_dev`` (n, S) int32
        against the observed ``obs`` (B, m) = ``x_weights[:, :m] * singvals[:m]``: ``count`` (B, m) int32 += the number of
        p with ``q_f |(R_p.T @ V)[f, l]| >= q_f |obs[f, l]|``, ``dmax`` (n, m) = the maximum over the features of the left
        side; q_f = 1 / s_f (0 for a feature without variance) with s_f the standard deviation of feature f over all rows
        when ``standardise``, else 1 (plsx_perm_weights_test).  Stateless: counts of disjoint sets of index rows add, their
        maxima concatenate.  No sync.  PlsxError status -2 (context still usable) when not even 64 permutations fit the
        scratch budget and for multiblock data, -4 without bound PLS-C data, -1 for m outside 1 .. T'."""
        torch = _torch()
        n, m = self._check_perm_weights(idx_dev, V)
        if tuple(obs.shape) != (self.B, m) or obs.dtype != torch.float64 or not obs.is_contiguous():
            raise ValueError('the observed statistic must be a contiguous ({}, {}) float64 tensor'.format(self.B, m))
        if tuple(count.shape) != (self.B, m) or count.dtype != torch.int32 or not count.is_contiguous():
            raise ValueError('the counts must be a contiguous ({}, {}) int32 tensor'.format(self.B, m))
        if tuple(dmax.shape) != (n, m) or dmax.dtype != torch.float64 or not dmax.is_contiguous():
            raise ValueError('the maxima must be a contiguous ({}, {}) float64 tensor'.format(n, m))
        self._check(self.lib.plsx_perm_weights_test(self.ctx, idx_dev.data_ptr(), n, V.data_ptr(), m, obs.data_ptr(),
                                                    1 if standardise else 0, count.data_ptr(), dmax.data_ptr(),
                                                    self._stream()))

    def perm_weights_scale(self):
        """(B,) device tensor: q_f = 1 / s_f, what ``perm_weights_test(standardise=True)`` scales feature f by -- s_f the
        standard deviation (ddof = 1) of the bound feature over all rows, q_f = 0 for a feature without variance
        (plsx_perm_weights_scale).  No sync."""
        q = self._empty((self.B,))
        self._check(self.lib.plsx_perm_weights_scale(self.ctx, q.data_ptr(), self._stream()))
        return q

    def simpls_perm_into(self, idx_dev, out_dev):
        """idx_dev (n, S) int32, out_dev (n, k): pctvar of the permuted Y."""
        self._check(self.lib.plsx_simpls_perm_batch(self.ctx, idx_dev.data_ptr(), idx_dev.shape[0],
                                                    out_dev.data_ptr(), self._stream()))

    def simpls_crossval_into(self, masks_dev, r_dev, r2_dev, sse_dev):
        """masks_dev (m, S) uint8, 1 = training row; r_dev / r2_dev (m, k, T): Pearson r and R^2 of the test rows under
        the first c = 1 .. k components; sse_dev (m, k + 1, T): squared error summed over the test rows, row 0 the
        intercept-only model (plsx_simpls_crossval_batch)."""
        m = masks_dev.shape[0]
        if tuple(masks_dev.shape) != (m, self.S) or masks_dev.dtype != _torch().uint8 or not masks_dev.is_contiguous():
            raise ValueError('split masks must be a contiguous (m, {}) uint8 tensor'.format(self.S))
        for t, rows in ((r_dev, self.k), (r2_dev, self.k), (sse_dev, self.k + 1)):
            if tuple(t.shape) != (m, rows, self.T) or not t.is_contiguous():
                raise ValueError('cross-validation outputs must be contiguous (m, k, T), (m, k, T) and (m, k + 1, T)')
        self._check(self.lib.plsx_simpls_crossval_batch(self.ctx, masks_dev.data_ptr(), m, r_dev.data_ptr(),
                                                        r2_dev.data_ptr(), sse_dev.data_ptr(), self._stream()))

    def simpls_crossval_perm_into(self, masks_dev, idx_dev, r_dev, r2_dev, mse_dev):
        """masks_dev (n, S) uint8, 1 = training row: the observed splits; idx_dev (m, S) int32, one permutation of the
        rows of Y per row.  r_dev / r2_dev (m, k, T): per permutation the mean over the n splits of the test-row Pearson
        r and R^2 of the first c = 1 .. k components; mse_dev (m, k + 1): the mean over the splits of the squared error
        per usable test row, row 0 the intercept-only model (plsx_simpls_crossval_perm_batch)."""
        torch = _torch()
        n, m = masks_dev.shape[0], idx_dev.shape[0]
        if tuple(masks_dev.shape) != (n, self.S) or masks_dev.dtype != torch.uint8 or not masks_dev.is_contiguous():
            raise ValueError('split masks must be a contiguous (n, {}) uint8 tensor'.format(self.S))
        if tuple(idx_dev.shape) != (m, self.S) or idx_dev.dtype != torch.int32 or not idx_dev.is_contiguous():
            raise ValueError('permutations must be a contiguous (m, {}) int32 tensor'.format(self.S))
        for t, shape in ((r_dev, (m, self.k, self.T)), (r2_dev, (m, self.k, self.T)), (mse_dev, (m, self.k + 1))):
            if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError('permuted cross-validation outputs must be contiguous float64 (m, k, T), (m, k, T) and '
                                 '(m, k + 1)')
        self._check(self.lib.plsx_simpls_crossval_perm_batch(self.ctx, masks_dev.data_ptr(), n, idx_dev.data_ptr(), m,
                                                             r_dev.data_ptr(), r2_dev.data_ptr(), mse_dev.data_ptr(),
                                                             self._stream()))

    def _check_nested_codes(self, codes_dev):
        torch = _torch()
        if codes_dev.dim() != 3 or codes_dev.shape[1] < 2 or codes_dev.shape[2] != self.S \
                or codes_dev.dtype != torch.uint8 or not codes_dev.is_contiguous():
            raise ValueError('nested split codes must be a contiguous (n, 1 + ni, {}) uint8 tensor with ni >= 1'
                             .format(self.S))
        return int(codes_dev.shape[0]), int(codes_dev.shape[1]) - 1

    def simpls_crossval_nested_into(self, codes_dev, r_dev, r2_dev, mse_dev, ncomp_dev, inner_dev):
        """Nested cross-validation of the component count.  codes_dev (n, 1 + ni, S) uint8: 1 = training row, 0 = test
        row, 2 = on neither side; row 0 of group s is outer split s, rows 1 .. ni its inner folds.  r_dev / r2_dev (n, T):
        the outer test rows' Pearson r and R^2 at the component count the inner folds chose; mse_dev (n,); ncomp_dev (n,)
        int32, 0 = undefined; inner_dev (n, k + 1): the mean inner-fold mse of c = 0 .. k components
        (plsx_simpls_crossval_nested_batch)."""
        torch = _torch()
        n, ni = self._check_nested_codes(codes_dev)
        for t, shape in ((r_dev, (n, self.T)), (r2_dev, (n, self.T)), (mse_dev, (n,)), (inner_dev, (n, self.k + 1))):
            if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError('nested cross-validation outputs must be contiguous float64 (n, T), (n, T), (n,) and '
                                 '(n, k + 1)')
        if tuple(ncomp_dev.shape) != (n,) or ncomp_dev.dtype != torch.int32 or not ncomp_dev.is_contiguous():
            raise ValueError('the selected component counts must be a contiguous (n,) int32 tensor')
        self._check(self.lib.plsx_simpls_crossval_nested_batch(
            self.ctx, codes_dev.data_ptr(), n, ni, r_dev.data_ptr(), r2_dev.data_ptr(), mse_dev.data_ptr(),
            ncomp_dev.data_ptr(), inner_dev.data_ptr(), self._stream()))

    def simpls_crossval_nested_perm_into(self, codes_dev, idx_dev, r_dev, r2_dev, mse_dev, count_dev):
        """The null of :meth:`simpls_crossval_nested_into` under permuted Y, selection included: idx_dev (m, S) int32,
        one permutation of the rows of Y per row.  r_dev / r2_dev (m, T), mse_dev (m,): per permutation the mean over
        the n outer splits of the nested scores, each split at the component count selected inside that permutation;
        count_dev (m, k) int32: how many outer splits chose c (plsx_simpls_crossval_nested_perm_batch)."""
        torch = _torch()
        n, ni = self._check_nested_codes(codes_dev)
        m = idx_dev.shape[0]
        if tuple(idx_dev.shape) != (m, self.S) or idx_dev.dtype != torch.int32 or not idx_dev.is_contiguous():
            raise ValueError('permutations must be a contiguous (m, {}) int32 tensor'.format(self.S))
        for t, shape in ((r_dev, (m, self.T)), (r2_dev, (m, self.T)), (mse_dev, (m,))):
            if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError('permuted nested cross-validation outputs must be contiguous float64 (m, T), (m, T) and '
                                 '(m,)')
        if tuple(count_dev.shape) != (m, self.k) or count_dev.dtype != torch.int32 or not count_dev.is_contiguous():
            raise ValueError('the selection counts must be a contiguous (m, k) int32 tensor')
        self._check(self.lib.plsx_simpls_crossval_nested_perm_batch(
            self.ctx, codes_dev.data_ptr(), n, ni, idx_dev.data_ptr(), m, r_dev.data_ptr(), r2_dev.data_ptr(),
            mse_dev.data_ptr(), count_dev.data_ptr(), self._stream()))

    def _nested_codes_dev(self, codes):
        codes = np.asarray(codes)
        if codes.ndim != 3 or codes.shape[0] != self.S:
            raise ValueError('nested split codes must have shape (S, n, 1 + ni) with S = {}'.format(self.S))
        return _torch().from_numpy(np.ascontiguousarray(codes.transpose(1, 2, 0), dtype=np.uint8)).to(self.device)

    def simpls_crossval_nested(self, codes):
        """codes (S, n, 1 + ni) of {0, 1, 2}, ``[:, s, 0]`` outer split s and ``[:, s, 1:]`` its inner folds -> dict of
        nested_pearson_r, nested_r_squared (T, n), nested_mse (n,), nested_ncomp (n,) int, inner_mse (k + 1, n)."""
        torch = _torch()
        dc = self._nested_codes_dev(codes)
        n = dc.shape[0]
        r, r2, mse, inner = self._empty((n, self.T)), self._empty((n, self.T)), self._empty((n,)), self._empty((n, self.k + 1))
        nc = torch.zeros((n,), dtype=torch.int32, device=self.device)
        self.simpls_crossval_nested_into(dc, r, r2, mse, nc, inner)
        self.sync()
        return dict(nested_pearson_r=r.cpu().numpy().T.copy(), nested_r_squared=r2.cpu().numpy().T.copy(),
                    nested_mse=mse.cpu().numpy(), nested_ncomp=nc.cpu().numpy().astype(np.int64),
                    inner_mse=inner.cpu().numpy().T.copy())

    def simpls_crossval_nested_perm(self, codes, perms):
        """codes as :meth:`simpls_crossval_nested`; perms (S, m), one permutation of 0 .. S-1 per column -> dict of
        perm_nested_pearson_r, perm_nested_r_squared (T, m), perm_nested_mse (m,), perm_nested_ncomp (k, m) int."""
        torch = _torch()
        dc = self._nested_codes_dev(codes)
        idx = check_index_array(np.asarray(perms), self.S)
        di = torch.from_numpy(np.ascontiguousarray(idx.T, dtype=np.int32)).to(self.device)
        m = di.shape[0]
        r, r2, mse = self._empty((m, self.T)), self._empty((m, self.T)), self._empty((m,))
        cnt = torch.zeros((m, self.k), dtype=torch.int32, device=self.device)
        self.simpls_crossval_nested_perm_into(dc, di, r, r2, mse, cnt)
        self.sync()
        return dict(perm_nested_pearson_r=r.cpu().numpy().T.copy(), perm_nested_r_squared=r2.cpu().numpy().T.copy(),
                    perm_nested_mse=mse.cpu().numpy(), perm_nested_ncomp=cnt.cpu().numpy().T.astype(np.int64))

    def simpls_set_confounds(self, Z):
        """Z (S, q) host array, 1 <= q <= 15, finite on the usable rows: residualises the bound X and Y on [1, Z] over
        the usable rows, in place, forms K again and keeps Z for the fold entries (plsx_simpls_set_confounds; after
        :meth:`set_data_regression` and :meth:`simpls_set_row_masks`).  -> the slopes of X (q, B) and of Y (q, T) on
        Z - zbar, device tensors.  PlsxError status -4 without bound regression data, -1 for q outside 1 .. 15 or rank
        deficient confounds."""
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[0] != self.S:
            raise ValueError('confounds must have shape ({}, q); got {}'.format(self.S, Z.shape))
        d = self._dev(Z, np.float64)
        gx, gy = self._empty((max(Z.shape[1], 1), self.B)), self._empty((max(Z.shape[1], 1), self.T))
        self._check(self.lib.plsx_simpls_set_confounds(self.ctx, d.data_ptr(), int(Z.shape[1]), gx.data_ptr(),
                                                       gy.data_ptr(), self._stream()))
        return gx, gy

    def simpls_crossval_confound_into(self, masks_dev, r_dev, r2_dev, sse_dev):
        """:meth:`simpls_crossval_into` with the confound regression fitted on the training rows of every split and
        applied to all its rows (plsx_simpls_crossval_confound_batch; after :meth:`simpls_set_confounds`).  PlsxError
        status -2, the context still usable, on the global route of the solver or when one K_s and one fit do not fit
        half the scratch budget."""
        m = masks_dev.shape[0]
        if tuple(masks_dev.shape) != (m, self.S) or masks_dev.dtype != _torch().uint8 or not masks_dev.is_contiguous():
            raise ValueError('split masks must be a contiguous (m, {}) uint8 tensor'.format(self.S))
        for t, rows in ((r_dev, self.k), (r2_dev, self.k), (sse_dev, self.k + 1)):
            if tuple(t.shape) != (m, rows, self.T) or not t.is_contiguous():
                raise ValueError('cross-validation outputs must be contiguous (m, k, T), (m, k, T) and (m, k + 1, T)')
        self._check(self.lib.plsx_simpls_crossval_confound_batch(self.ctx, masks_dev.data_ptr(), m, r_dev.data_ptr(),
                                                                 r2_dev.data_ptr(), sse_dev.data_ptr(), self._stream()))

    def simpls_crossval_confound_perm_into(self, masks_dev, idx_dev, r_dev, r2_dev, mse_dev):
        """:meth:`simpls_crossval_perm_into` under the fold-wise confound regression: the residualised Y is permuted and
        residualised again per fold (plsx_simpls_crossval_confound_perm_batch).  No row masks."""
        torch = _torch()
        n, m = masks_dev.shape[0], idx_dev.shape[0]
        if tuple(masks_dev.shape) != (n, self.S) or masks_dev.dtype != torch.uint8 or not masks_dev.is_contiguous():
            raise ValueError('split masks must be a contiguous (n, {}) uint8 tensor'.format(self.S))
        if tuple(idx_dev.shape) != (m, self.S) or idx_dev.dtype != torch.int32 or not idx_dev.is_contiguous():
            raise ValueError('permutations must be a contiguous (m, {}) int32 tensor'.format(self.S))
        for t, shape in ((r_dev, (m, self.k, self.T)), (r2_dev, (m, self.k, self.T)), (mse_dev, (m, self.k + 1))):
            if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError('permuted cross-validation outputs must be contiguous float64 (m, k, T), (m, k, T) and '
                                 '(m, k + 1)')
        self._check(self.lib.plsx_simpls_crossval_confound_perm_batch(
            self.ctx, masks_dev.data_ptr(), n, idx_dev.data_ptr(), m, r_dev.data_ptr(), r2_dev.data_ptr(),
            mse_dev.data_ptr(), self._stream()))

    def simpls_split_half_into(self, perm_dev, masks_dev, uc_dev, vc_dev):
        """Split-half reliability of the SIMPLS components.  perm_dev (n, S) int32, one permutation of the rows of Y per
        arrangement, or None: the observed arrangement (n = masks_dev.shape[0]); masks_dev (n, ns, S) uint8, 1 = first
        half, the arrangement's own splits.  uc_dev / vc_dev (n, ns, k): per split the correlation between the halves of
        the projections D_h^T q_c over the features and D_h w_c over the behaviours (plsx_simpls_split_half_batch);
        :meth:`mean_splits_into` averages them."""
        torch = _torch()
        if masks_dev.dim() != 3:
            raise ValueError('split masks must be a contiguous (n, ns, {}) uint8 tensor'.format(self.S))
        n, ns = masks_dev.shape[0], masks_dev.shape[1]
        if tuple(masks_dev.shape) != (n, ns, self.S) or masks_dev.dtype != torch.uint8 or not masks_dev.is_contiguous() \
                or n < 1 or ns < 1:
            raise ValueError('split masks must be a contiguous (n, ns, {}) uint8 tensor'.format(self.S))
        if perm_dev is not None and (tuple(perm_dev.shape) != (n, self.S) or perm_dev.dtype != torch.int32
                                     or not perm_dev.is_contiguous()):
            raise ValueError('permutations must be a contiguous (n, {}) int32 tensor, one per arrangement'.format(self.S))
        for t in (uc_dev, vc_dev):
            if tuple(t.shape) != (n, ns, self.k) or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError('split-half outputs must be contiguous float64 (n, ns, k)')
        self._check(self.lib.plsx_simpls_split_half_batch(
            self.ctx, None if perm_dev is None else perm_dev.data_ptr(), n, masks_dev.data_ptr(), ns,
            uc_dev.data_ptr(), vc_dev.data_ptr(), self._stream()))

    def simpls_coef_begin(self, c):
        """Open a coefficient series for the model of the first ``c`` components: until :meth:`simpls_coef_finish`
        every :meth:`simpls_boot_into` also accumulates the bootstrap's coefficients in dual space
        (plsx_simpls_coef_begin).  PlsxError (status -2, context still usable) when the T x S x S accumulator does
        not fit."""
        self._check(self.lib.plsx_simpls_coef_begin(self.ctx, int(c), self._stream()))

    def simpls_coef_finish(self, bsum, bsq):
        """Close the series: bsum / bsq (B, T) += sum over the bootstraps of coefs / coefs^2, one pass over the
        features (plsx_simpls_coef_finish)."""
        for t in (bsum, bsq):
            if tuple(t.shape) != (self.B, self.T) or not t.is_contiguous():
                raise ValueError('coefficient sums must be contiguous ({}, {}) tensors'.format(self.B, self.T))
        self._check(self.lib.plsx_simpls_coef_finish(self.ctx, bsum.data_ptr(), bsq.data_ptr(), self._stream()))

    def simpls_coef_keep(self, stack):
        """Have the open coefficient series keep every bootstrap's A_b: ``stack`` (capacity, T, S), a contiguous
        float64 tensor on this device, is filled in submission order by the :meth:`simpls_boot_into` calls that
        follow (plsx_simpls_coef_keep).  PlsxError: status -4 without an open series, -1 from the batch that would
        overflow the stack."""
        torch = _torch()
        if stack.dim() != 3 or tuple(stack.shape[1:]) != (self.T, self.S) or stack.dtype != torch.float64 \
                or not stack.is_contiguous():
            raise ValueError('the kept stack must be a contiguous (capacity, {}, {}) float64 tensor'.format(self.T, self.S))
        self._check(self.lib.plsx_simpls_coef_keep(self.ctx, stack.data_ptr(), int(stack.shape[0])))

    def simpls_coef_ci(self, stack, ci=95):
        """Percentile interval of the coefficients over the bootstraps of ``stack`` (n, T, S) -- a kept stack, the
        gathered stacks of several ranks, or any contiguous float64 device tensor of that shape: (lo, hi) device
        tensors (B, T), ``np.percentile(coefs_boot, [(100 - ci) / 2, 100 - (100 - ci) / 2], axis=-1)`` of
        ``coefs_boot[f, t, b] = (Xc.T @ stack[b].T)[f, t]`` without that array ever existing (plsx_simpls_coef_ci).  No
        sync.  PlsxError status -2 (context still usable) for n > 16384 or a stack that does not fit the scratch
        budget."""
        torch = _torch()
        if stack.dim() != 3 or tuple(stack.shape[1:]) != (self.T, self.S) or stack.dtype != torch.float64 \
                or not stack.is_contiguous():
            raise ValueError('the stack must be a contiguous (n, {}, {}) float64 tensor'.format(self.T, self.S))
        n = int(stack.shape[0])
        idx = _virtual_indices(max(n, 1), ci)
        lo, hi = self._empty((self.B, self.T)), self._empty((self.B, self.T))
        self._check(self.lib.plsx_simpls_coef_ci(self.ctx, stack.data_ptr(), n, idx[0][0], idx[0][1], idx[1][0],
                                                 idx[1][1], lo.data_ptr(), hi.data_ptr(), self._stream()))
        return lo, hi

    def simpls_coef_perm_test(self, stack, obs, count, dmax, standardise=True):
        """The permutation statistics of ``stack`` (n, T, S) -- any contiguous float64 device tensor -- against the
        observed coefficients ``obs`` (B, T): ``count`` (B, T) int32 += the number of b with
        ``s_f |(Xc.T @ stack[b].T)[f, t]| >= s_f |obs[f, t]|``, ``dmax`` (n, T) = the maximum over the features of the
        left side; s_f the standard deviation of feature f when ``standardise``, else 1
        (plsx_simpls_coef_perm_test).  No sync."""
        torch = _torch()
        if stack.dim() != 3 or tuple(stack.shape[1:]) != (self.T, self.S) or stack.dtype != torch.float64 \
                or not stack.is_contiguous():
            raise ValueError('the stack must be a contiguous (n, {}, {}) float64 tensor'.format(self.T, self.S))
        n = int(stack.shape[0])
        self._check_coef_perm(obs, count, dmax, n)
        self._check(self.lib.plsx_simpls_coef_perm_test(self.ctx, stack.data_ptr(), n, obs.data_ptr(),
                                                        1 if standardise else 0, count.data_ptr(), dmax.data_ptr(),
                                                        self._stream()))

    def _check_coef_perm(self, obs, count, dmax, n):
        torch = _torch()
        if tuple(obs.shape) != (self.B, self.T) or obs.dtype != torch.float64 or not obs.is_contiguous():
            raise ValueError('the observed coefficients must be a contiguous ({}, {}) float64 tensor'.format(self.B, self.T))
        if tuple(count.shape) != (self.B, self.T) or count.dtype != torch.int32 or not count.is_contiguous():
            raise ValueError('the counts must be a contiguous ({}, {}) int32 tensor'.format(self.B, self.T))
        if tuple(dmax.shape) != (n, self.T) or dmax.dtype != torch.float64 or not dmax.is_contiguous():
            raise ValueError('the maxima must be a contiguous ({}, {}) float64 tensor'.format(n, self.T))

    def simpls_coef_perm_begin(self, c, obs, count, dmax, standardise=True):
        """Open a permutation series of the coefficients of the ``c``-component model: until
        :meth:`simpls_coef_perm_end` every :meth:`simpls_perm_into` also forms its permutations' coefficients tile by
        tile, adds their exceedances of ``obs`` (B, T) to ``count`` (B, T) int32 and appends their maxima over the
        features to ``dmax`` (capacity, T) in submission order (plsx_simpls_coef_perm_begin).  The three tensors must
        stay alive until the series ends.  PlsxError: status -1 for c outside 1 .. k and from the batch that would
        pass the capacity, -4 before the original fit is set."""
        self._check_coef_perm(obs, count, dmax, int(dmax.shape[0]))
        self._check(self.lib.plsx_simpls_coef_perm_begin(self.ctx, int(c), obs.data_ptr(), 1 if standardise else 0,
                                                         count.data_ptr(), dmax.data_ptr(), int(dmax.shape[0])))

    def simpls_coef_perm_end(self):
        """Close the permutation series of the coefficients (plsx_simpls_coef_perm_end)."""
        self._check(self.lib.plsx_simpls_coef_perm_end(self.ctx))

    def simpls_set_classes(self, codes):
        """Bind one class code 0 .. T - 1 per row of the bound regression data, whose Y is the centred indicator matrix
        of those T classes (plsx_simpls_set_classes); ``None`` clears the binding.  PlsxError: status -1 for a code
        outside the range, -2 (context still usable) for more than 32 classes."""
        if codes is None:
            self._check(self.lib.plsx_simpls_set_classes(self.ctx, None, 0, self._stream()))
            return
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if codes.shape != (self.S,):
            raise ValueError('class codes must have shape ({},); got {}'.format(self.S, codes.shape))
        dev = _torch().from_numpy(codes).to(self.device)
        self._check(self.lib.plsx_simpls_set_classes(self.ctx, dev.data_ptr(), self.T, self._stream()))

    def simpls_cv_class_begin(self, conf_dev):
        """Open a series of confusion counts: until :meth:`simpls_cv_class_end` every :meth:`simpls_crossval_into` of m
        splits appends m blocks (k, T, T) -- [c - 1, true class, predicted class] over the usable test rows -- to
        ``conf_dev`` (capacity, k, T, T) int32 in submission order, and every :meth:`simpls_crossval_perm_into` of m
        permutations m blocks, each summed over that call's splits (plsx_simpls_cv_class_begin).  The tensor must stay
        alive until the series ends.  PlsxError: status -4 before :meth:`simpls_set_classes`, -1 from the call that
        would pass the capacity."""
        torch = _torch()
        if conf_dev.dim() != 4 or tuple(conf_dev.shape[1:]) != (self.k, self.T, self.T) or conf_dev.dtype != torch.int32 \
                or not conf_dev.is_contiguous():
            raise ValueError('the confusion counts must be a contiguous (capacity, {}, {}, {}) int32 tensor'
                             .format(self.k, self.T, self.T))
        self._check(self.lib.plsx_simpls_cv_class_begin(self.ctx, conf_dev.data_ptr(), int(conf_dev.shape[0])))

    def simpls_cv_class_end(self):
        """Close the series of confusion counts (plsx_simpls_cv_class_end)."""
        self._check(self.lib.plsx_simpls_cv_class_end(self.ctx))

    def simpls_cv_auc_begin(self, auc_dev):
        """Open a series of AUC counts, independent of the confusion series: until :meth:`simpls_cv_auc_end` every
        :meth:`simpls_crossval_into` of m splits appends m blocks (k, T, 2) -- [c - 1, class, (u2, pairs)]: twice the
        Mann-Whitney U of the predicted indicator of the class between the usable test rows of the class and the other
        usable test rows, ties counted once, and the number of such pairs -- to ``auc_dev`` (capacity, k, T, 2) int64 in
        submission order, and every :meth:`simpls_crossval_perm_into` of m permutations m blocks, each summed over that
        call's splits (plsx_simpls_cv_auc_begin).  The tensor must stay alive until the series ends.  PlsxError: status
        -4 before :meth:`simpls_set_classes`, -1 from the call that would pass the capacity."""
        torch = _torch()
        if auc_dev.dim() != 4 or tuple(auc_dev.shape[1:]) != (self.k, self.T, 2) or auc_dev.dtype != torch.int64 \
                or not auc_dev.is_contiguous():
            raise ValueError('the AUC counts must be a contiguous (capacity, {}, {}, 2) int64 tensor'
                             .format(self.k, self.T))
        self._check(self.lib.plsx_simpls_cv_auc_begin(self.ctx, auc_dev.data_ptr(), int(auc_dev.shape[0])))

    def simpls_cv_auc_end(self):
        """Close the series of AUC counts (plsx_simpls_cv_auc_end)."""
        self._check(self.lib.plsx_simpls_cv_auc_end(self.ctx))

    CVN_RULES = {'mse': 0, 'accuracy': 1, 'balanced_accuracy': 2}

    def simpls_cvn_class_begin(self, rule, conf_dev, auc_dev=None, inner_dev=None):
        """Open the series of nested counts (PLS-DA; after :meth:`simpls_set_classes`): until
        :meth:`simpls_cvn_class_end` the nested entries classify every fit, select the component count of a group by
        ``rule`` -- 'balanced_accuracy' or 'accuracy' of the confusion counts pooled over the inner folds (first maximum),
        or 'mse' (the rule they have without the series) -- and append the OUTER fit's counts at the selected count:
        :meth:`simpls_crossval_nested_into` of n outer splits n blocks to ``conf_dev`` (capacity, T, T) int32,
        ``auc_dev`` (capacity, T, 2) int64 (or None: no AUC counts) and the pooled inner counts to ``inner_dev``
        (capacity, k, T, T) int32 (or None); :meth:`simpls_crossval_nested_perm_into` of m permutations m blocks, each
        the sum over the outer splits (plsx_simpls_cvn_class_begin).  The tensors must stay alive until the series ends.
        PlsxError: status -4 before :meth:`simpls_set_classes`, -1 from the call that would pass the capacity."""
        torch = _torch()
        if rule not in self.CVN_RULES:
            raise ValueError('the selection rule must be one of {}; got {!r}'.format(sorted(self.CVN_RULES), rule))
        cap = int(conf_dev.shape[0]) if conf_dev.dim() == 3 else -1
        for t, shape, dt in ((conf_dev, (cap, self.T, self.T), torch.int32), (auc_dev, (cap, self.T, 2), torch.int64),
                             (inner_dev, (cap, self.k, self.T, self.T), torch.int32)):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous()):
                raise ValueError('the nested counts must be contiguous (capacity, {0}, {0}) int32, (capacity, {0}, 2) int64 '
                                 'and (capacity, {1}, {0}, {0}) int32 tensors of one capacity'.format(self.T, self.k))
        self._check(self.lib.plsx_simpls_cvn_class_begin(
            self.ctx, self.CVN_RULES[rule], conf_dev.data_ptr(), auc_dev.data_ptr() if auc_dev is not None else None,
            inner_dev.data_ptr() if inner_dev is not None else None, cap))

    def simpls_cvn_class_end(self):
        """Close the series of nested counts (plsx_simpls_cvn_class_end)."""
        self._check(self.lib.plsx_simpls_cvn_class_end(self.ctx))

    def simpls_cv_pred_begin(self, c, pred_dev, ncomp_dev=None, true_dev=None):
        """Open a series of out-of-fold predictions: until :meth:`simpls_cv_pred_end` every :meth:`simpls_crossval_into`
        / :meth:`simpls_crossval_confound_into` of m splits appends m slots (T, S) to ``pred_dev`` (capacity, T, S)
        float64 in submission order -- the prediction of the ``c``-component model on the usable test rows of the split,
        NaN elsewhere -- and every :meth:`simpls_crossval_nested_into` the slots of its outer fits; ``c = 0``: with the
        component count its selection chose (plsx_simpls_cv_pred_begin).  ``ncomp_dev`` (capacity,) int32 takes the
        count used per slot, ``true_dev`` (capacity, T, S) the observed values at the same positions.  The tensors must
        stay alive until the series ends.  PlsxError: status -1 for c outside 0 .. k and from the call that would pass
        the capacity, -2 (context still usable) for a stack beyond the scratch budget."""
        torch = _torch()
        for t in (pred_dev, true_dev):
            if t is not None and (t.dim() != 3 or tuple(t.shape[1:]) != (self.T, self.S) or t.dtype != torch.float64
                                  or not t.is_contiguous() or t.shape[0] != pred_dev.shape[0]):
                raise ValueError('the stacks of predictions must be contiguous (capacity, {}, {}) float64 tensors'
                                 .format(self.T, self.S))
        if ncomp_dev is not None and (tuple(ncomp_dev.shape) != (int(pred_dev.shape[0]),) or ncomp_dev.dtype != torch.int32
                                      or not ncomp_dev.is_contiguous()):
            raise ValueError('the component counts must be a contiguous (capacity,) int32 tensor')
        self._check(self.lib.plsx_simpls_cv_pred_begin(
            self.ctx, int(c), ncomp_dev.data_ptr() if ncomp_dev is not None else None, pred_dev.data_ptr(),
            true_dev.data_ptr() if true_dev is not None else None, int(pred_dev.shape[0])))

    def simpls_cv_pred_end(self):
        """Close the series of out-of-fold predictions (plsx_simpls_cv_pred_end)."""
        self._check(self.lib.plsx_simpls_cv_pred_end(self.ctx))

    def simpls_vip_keep(self, stack):
        """Keep the VIP stack of every bootstrap the :meth:`simpls_boot_into` calls that follow solve: ``stack``
        (capacity, c, S), a contiguous float64 tensor on this device, is filled in submission order with the scaled dual
        weights of the first c components (plsx_simpls_vip_keep); ``VIP_b[f]**2 = B * ((Xc.T @ stack[b].T)**2).sum(-1)[f]``.
        Independent of a coefficient series.  PlsxError: status -4 before the original fit is set, -1 for c outside
        1 .. k and from the batch that would overflow the stack."""
        torch = _torch()
        if stack.dim() != 3 or stack.shape[2] != self.S or stack.dtype != torch.float64 or not stack.is_contiguous():
            raise ValueError('the kept VIP stack must be a contiguous (capacity, c, {}) float64 tensor'.format(self.S))
        self._check(self.lib.plsx_simpls_vip_keep(self.ctx, int(stack.shape[1]), stack.data_ptr(), int(stack.shape[0])))

    def simpls_vip_ci(self, stack, ci=95):
        """Standard deviation (ddof = 1) and percentile interval of the VIP scores over the bootstraps of ``stack``
        (n, c, S) -- a kept stack, the gathered stacks of several ranks, or any contiguous float64 device tensor of that
        shape: (sd, lo, hi) device tensors (B,), ``np.std(vip_boot, ddof=1, axis=-1)`` and ``np.percentile(vip_boot,
        [(100 - ci) / 2, 100 - (100 - ci) / 2], axis=-1)`` of ``vip_boot[f, b] = sqrt(B * ((Xc.T @ stack[b].T)**2).sum(-1))[f]``
        without that array ever existing (plsx_simpls_vip_ci).  No sync.  PlsxError status -2 (context still usable) for
        n > 16384 or a stack that does not fit the scratch budget."""
        torch = _torch()
        if stack.dim() != 3 or stack.shape[2] != self.S or stack.dtype != torch.float64 or not stack.is_contiguous():
            raise ValueError('the stack must be a contiguous (n, c, {}) float64 tensor'.format(self.S))
        n, c = int(stack.shape[0]), int(stack.shape[1])
        idx = _virtual_indices(max(n, 1), ci)
        sd, lo, hi = self._empty((self.B,)), self._empty((self.B,)), self._empty((self.B,))
        self._check(self.lib.plsx_simpls_vip_ci(self.ctx, stack.data_ptr(), n, c, idx[0][0], idx[0][1], idx[1][0],
                                                idx[1][1], sd.data_ptr(), lo.data_ptr(), hi.data_ptr(), self._stream()))
        return sd, lo, hi

    def simpls_vip_perm_test(self, stack, obs, count, dmax):
        """The permutation statistics of ``stack`` (n, c, S) -- any contiguous float64 device tensor in the layout of
        :meth:`simpls_vip_keep` -- against the observed VIP scores ``obs`` (B,): ``count`` (B,) int32 += the number of b
        with ``sqrt(B * ((Xc.T @ stack[b].T)**2).sum(-1))[f] >= obs[f]``, ``dmax`` (n,) = the maximum over the features
        of the left side, 0 for a permutation whose scores are NaN (plsx_simpls_vip_perm_test).  No sync."""
        torch = _torch()
        if stack.dim() != 3 or stack.shape[2] != self.S or stack.dtype != torch.float64 or not stack.is_contiguous():
            raise ValueError('the stack must be a contiguous (n, c, {}) float64 tensor'.format(self.S))
        n, c = int(stack.shape[0]), int(stack.shape[1])
        self._check_vip_perm(obs, count, dmax, n)
        self._check(self.lib.plsx_simpls_vip_perm_test(self.ctx, stack.data_ptr(), n, c, obs.data_ptr(),
                                                       count.data_ptr(), dmax.data_ptr(), self._stream()))

    def _check_vip_perm(self, obs, count, dmax, n):
        torch = _torch()
        if tuple(obs.shape) != (self.B,) or obs.dtype != torch.float64 or not obs.is_contiguous():
            raise ValueError('the observed VIP scores must be a contiguous ({},) float64 tensor'.format(self.B))
        if tuple(count.shape) != (self.B,) or count.dtype != torch.int32 or not count.is_contiguous():
            raise ValueError('the counts must be a contiguous ({},) int32 tensor'.format(self.B))
        if tuple(dmax.shape) != (n,) or dmax.dtype != torch.float64 or not dmax.is_contiguous():
            raise ValueError('the maxima must be a contiguous ({},) float64 tensor'.format(n))

    def simpls_vip_perm_begin(self, c, obs, count, dmax):
        """Open a permutation series of the VIP scores of the ``c``-component model: until
        :meth:`simpls_vip_perm_end` every :meth:`simpls_perm_into` also forms its permutations' scores tile by tile,
        adds their exceedances of ``obs`` (B,) to ``count`` (B,) int32 and appends their maxima over the features to
        ``dmax`` (capacity,) in submission order (plsx_simpls_vip_perm_begin).  Independent of a coefficient series:
        both may be open.  The three tensors must stay alive until the series ends.  PlsxError: status -1 for c
        outside 1 .. k and from the batch that would pass the capacity, -4 before the original fit is set."""
        self._check_vip_perm(obs, count, dmax, int(dmax.shape[0]))
        self._check(self.lib.plsx_simpls_vip_perm_begin(self.ctx, int(c), obs.data_ptr(), count.data_ptr(),
                                                        dmax.data_ptr(), int(dmax.shape[0])))

    def simpls_vip_perm_end(self):
        """Close the permutation series of the VIP scores (plsx_simpls_vip_perm_end)."""
        self._check(self.lib.plsx_simpls_vip_perm_end(self.ctx))

    def simpls_boot_into(self, idx_dev, usum, usq, yl_dev, ystack=None):
        """idx_dev (n, S) int32; usum / usq (B, k) accumulated in place; yl_dev (n, T, k);
        ystack (n, S, T) device tensor: one Y per bootstrap (3-D Y), or None."""
        if ystack is not None and tuple(ystack.shape) != (idx_dev.shape[0], self.S, self.T):
            raise ValueError('ystack must have shape ({}, {}, {})'.format(idx_dev.shape[0], self.S, self.T))
        self._check(self.lib.plsx_simpls_boot_batch(self.ctx, idx_dev.data_ptr(),
                                                    None if ystack is None else ystack.data_ptr(),
                                                    idx_dev.shape[0], usum.data_ptr(), usq.data_ptr(),
                                                    yl_dev.data_ptr(), self._stream()))

    def split_half_into(self, perm_dev, masks_dev, uc_dev, vc_dev, ystack_dev=None):
        """perm_dev (np, S) int32 or None, masks_dev (np, ns, S) uint8, outputs (np, ns, L);
        ystack_dev (np, S, T): pre-permuted behaviour matrices instead of index rows."""
        n_arr, ns = masks_dev.shape[0], masks_dev.shape[1]
        self._check(self.lib.plsx_split_half_batch_y(
            self.ctx, None if perm_dev is None else perm_dev.data_ptr(),
            None if ystack_dev is None else ystack_dev.data_ptr(), n_arr, masks_dev.data_ptr(), ns,
            uc_dev.data_ptr(), vc_dev.data_ptr(), self._stream()))

    def mean_splits_into(self, corr_dev, out_dev):
        """corr_dev (np, ns, L) -> out_dev (np, L): the mean over splits of BasePLS.split_half (base.py:770)."""
        n_arr, ns, L = corr_dev.shape
        self._check(self.lib.plsx_mean_splits(self.ctx, corr_dev.data_ptr(), n_arr, ns, L, out_dev.data_ptr(),
                                              self._stream()))

    def boot_rel(self, orig, usum, usq, n_boot, add_orig=False):
        """compute.boot_rel on the device; orig numpy or tensor (B, L).  With
        add_orig the original is added back first and ``n_boot`` must already
        be R + 1 (behavioral.py:201-207)."""
        torch = _torch()
        d_orig = orig if isinstance(orig, torch.Tensor) else self._dev(orig, np.float64)
        bsr, se = self._empty(tuple(usum.shape)), self._empty(tuple(usum.shape))
        self._check(self.lib.plsx_boot_rel(self.ctx, d_orig.data_ptr(), usum.data_ptr(), usq.data_ptr(),
                                           int(n_boot), 1 if add_orig else 0, usum.numel(),
                                           bsr.data_ptr(), se.data_ptr(),
                                           self._stream()))
        self.sync()
        return bsr.cpu().numpy(), se.cpu().numpy()

    def percentile_ci(self, boot, ci=95):
        """compute.boot_ci on the device: boot (..., n) -> lower, upper (...)."""
        boot = np.ascontiguousarray(boot, dtype=np.float64)
        n = boot.shape[-1]
        if n > 16384:                                   # longer series: numpy on the host
            low = (100 - ci) / 2
            lo, hi = np.percentile(boot, [low, 100 - low], axis=-1)
            return lo, hi
        low = (100 - ci) / 2
        idx = []
        for q in (low, 100 - low):                      # numpy's virtual index of the quantile
            vi = (n - 1) * np.true_divide(q, 100)
            prev = np.floor(vi)
            idx.append((int(prev), float(vi - prev)))
        d = self._dev(boot.reshape(-1, n), np.float64)
        lo, hi = self._empty((d.shape[0],)), self._empty((d.shape[0],))
        self._check(self.lib.plsx_percentile_ci(self.ctx, d.data_ptr(), d.shape[0], n, idx[0][0], idx[0][1],
                                                idx[1][0], idx[1][1], lo.data_ptr(), hi.data_ptr(),
                                                self._stream()))
        self.sync()
        shp = boot.shape[:-1]
        return lo.cpu().numpy().reshape(shp), hi.cpu().numpy().reshape(shp)

    # -- measurement --------------------------------------------------------
    def mfma_f64_peak(self):
        """Measured fp64 MFMA TFLOP/s of this GPU (microbenchmark)."""
        v = ctypes.c_double()
        self._check(self.lib.plsx_mfma_f64_peak(self.ctx, ctypes.byref(v)))
        return v.value

    def set_timing(self, enable=True):
        self._check(self.lib.plsx_set_timing(self.ctx, 1 if enable else 0))

    def kernel_timing(self):
        """{kernel class: (summed ms, launches)} since set_timing(True)."""
        out = {}
        k = 0
        while True:
            name = self.lib.plsx_kernel_class_name(k)
            if not name:
                break
            ms, n = ctypes.c_double(), ctypes.c_int()
            self._check(self.lib.plsx_kernel_timing(self.ctx, k, ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                out[name.decode()] = (ms.value, n.value)
            k += 1
        return out

    def set_perm_path(self, dual):
        """Permutations through the S x S dual path (True) or the feature pass; None keeps
        the route and only drops the cached S x S kernel (a new analysis forms its own)."""
        rc = self.lib.plsx_set_perm_path(self.ctx, -1 if dual is None else (1 if dual else 0))
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def last_timing(self):
        """include/plsx.h, plsx_last_timing.  ``urot_waves`` .. ``gram_kernel`` say how the last rotation (k_urot) and Gram pass
        were launched, ``split_blocks`` / ``split_reader`` how the last split-half pass ran; they are recorded whether or
        not timing is on.  ``moment_rows``: 1 when the compact bootstrap blocks of the last launch formed the first
        moments of the features in their padding rows (option ``no_moment_rows`` forces 0).  ``perm_projected``: 1 when
        the last permutation call took the projected route -- singular values from the row norms of (V0^T A_p) X, no R,
        no Gram pass, no small solver (option ``no_perm_project`` forces 0).  ``compact_col_tiles``: column tiles per wave
        of the compact bootstrap blocks of the last launch -- 4 (blocks of 256 columns) or 2 (128; option
        ``no_compact_wide`` forces it, ``compact_wide_always`` forces 4 up to T' = 64), 0 without such a launch."""
        buf = (ctypes.c_double * 24)()
        n = self.lib.plsx_last_timing(self.ctx, buf, 24)
        keys = ['xprod_ms', 'xprod_launches', 'resamples_per_group', 'm_tiles', 'superbatch',
                'xprod_resamples', 'dual_perm', 'compact_row_fraction', 'nt_flops', 'quad_series', 'quad_m_tiles',
                'quad_blocks_per_lv', 'urot_waves', 'urot_splits', 'urot_res_per_split', 'urot_variant',
                'gram_chunks', 'urot_variant_last', 'gram_kernel', 'split_blocks', 'split_reader',
                'moment_rows', 'perm_projected', 'compact_col_tiles']
        return {k: buf[i] for i, k in enumerate(keys[:max(n, 0)])}


# ---------------------------------------------------------------------------
# the front-ends' default engine
# ---------------------------------------------------------------------------
_DEFAULT = {}
_DEFAULT_LOCK = threading.Lock()


def default_engine(device=None, replica=0):
    """The engine the public calls use when none is passed: ONE per (process, device), created on first use and
    kept -- its context, the resident copy of the last X and the super-batch scratch stay mapped between calls.
    (``replica`` > 0: a further context on the same device, for a team that lists a device twice, team.py.)

    Why not a fresh engine per call (rounds 1-3): mapping device memory is not free on a shared MI355X.  The
    driver clears recycled VRAM lazily, so a call that maps the tens of GB its predecessor just released waits
    for the clear (25 ms per GB: 1 - 5 s measured for the c4 shape, ten times the analysis' own fixed cost),
    while a context that is re-bound (plsx_set_data) reuses what it holds.  ``release_default_engine()`` gives
    the memory back.

    **What stays mapped after a call returns**: the resident copy of X (0.8 GB at 500 x 200 000) and the
    super-batch scratch the call sized for itself (up to 48 GB) -- on purpose, see above, but it IS device memory
    that later work on the same GPU (torch or otherwise) cannot use until ``pypyls_amd.release_default_engine()``
    is called.  Thread safety: creation is guarded here, use is serialised by ``Engine.lock`` in the front-ends."""
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    key = (int(device), int(replica))
    with _DEFAULT_LOCK:
        eng = _DEFAULT.get(key)
        if eng is None or not getattr(eng, 'ctx', None):
            if not _DEFAULT:
                import atexit
                atexit.register(release_default_engine)     # free the device memory before the runtime goes away
            eng = _DEFAULT[key] = Engine(device=key[0])
    return eng


# The cached engines keep the resident X and the super-batch scratch (up to tens of GB) mapped so that the NEXT call
# does not pay for mapping them again (25 ms per GB of recycled VRAM).  A process that has stopped calling should not
# sit on that memory for ever (a surprise-OOM for other work sharing the GPU): IDLE_RELEASE_S
# seconds after the last front-end call finished, the cached engines (and teams) nobody is using are released -- the
# next call simply builds new ones.  0 / None disables; release_default_engine() does it at once.
IDLE_RELEASE_S = 300.0
_IDLE = {'timer': None}


def touch_idle_release():
    """(Re)start the idle clock; the front-ends call this when a call ends."""
    if not IDLE_RELEASE_S:
        return
    with _DEFAULT_LOCK:
        old = _IDLE['timer']
        if old is not None:
            old.cancel()
        t = threading.Timer(float(IDLE_RELEASE_S), _idle_fire)
        t.daemon = True
        _IDLE['timer'] = t
        t.start()


def _idle_fire():
    try:
        with _DEFAULT_LOCK:
            engines = list(_DEFAULT.values())
        held = []
        for eng in engines:
            if eng.lock.acquire(blocking=False):
                held.append(eng)
        try:
            if len(held) == len(engines):               # nobody is in a call: give the memory back
                release_default_engine()
            else:
                touch_idle_release()                    # a call is running: look again later
        finally:
            for eng in held:
                eng.lock.release()
    except Exception:                                   # noqa: BLE001 -- a timer thread must never raise (interpreter exit)
        pass


def release_default_engine(device=None):
    """Destroy the cached default engine(s) and free their device memory."""
    from . import team as _team
    _team.release_teams()                                   # their communicators go before the contexts
    with _DEFAULT_LOCK:
        keys = [k for k in _DEFAULT if device is None or k[0] == int(device)]
        engines = [_DEFAULT.pop(key, None) for key in keys]
    for eng in engines:
        if eng is not None:
            with eng.lock:                                  # (a call in flight on another thread finishes first)
                eng.close()
