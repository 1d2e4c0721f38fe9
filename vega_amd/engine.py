"""ctypes binding of libvegamx.so and the lowering of a :class:`vega_amd.setup.Problem` to it.

This is the reference-side binding INTEGRATION.md describes: plain ``ctypes`` against the C ABI of
``include/vegamx.h``.  There is no CPU fallback: if the library (or a GPU) is missing the engine
fails loudly.
"""
import contextlib
import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import fftlog_op, static_terms

_LIB_PATH = Path(__file__).resolve().parent / 'libvegamx.so'
_lib = None

VMX_MAX_ELL = 4
VMX_MAX_SMOOTH = 3
VMX_N_KERNELS = 13
HCD = {'none': 0, 'Rogers': 1, 'sinc': 2, 'fvoigt': 3}
NL = {'none': 0, 'arinyo': 1, 'mcdonald': 2}
VD = {None: 0, 'gauss': 1, 'lorentz': 2}
SCALE_UNIT, SCALE_AP_AT, SCALE_AISO_EPS, SCALE_PHI_ALPHA = 0, 1, 2, 3
PKLIN = {'peak': 0, 'smooth': 1, 'full': 2}
MAT_DISTORTION, MAT_INVCOV, MAT_METAL = 0, 1, 2
BB_POS = {('pre', 'mul'): 0, ('pre', 'add'): 1, ('post', 'mul'): 2, ('post', 'add'): 3}
BB_POLY, BB_SKY = 0, 1
DEFAULT_GROWTH_RATE = 0.970386   # reference vega/utils.py:60

STATUS_BOUNDS, STATUS_ARINYO, STATUS_NONFINITE, STATUS_NOT_CONSTANT = 1, 2, 4, 8


class EngineError(RuntimeError):
    pass


class Tracer(C.Structure):
    _fields_ = [('bias_slot', C.c_int32), ('bias_eta_slot', C.c_int32), ('beta_slot', C.c_int32),
                ('is_lya', C.c_int32), ('discrete', C.c_int32), ('vd_sigma_slot', C.c_int32),
                ('evol_kind', C.c_int32), ('alpha_slot', C.c_int32)]


class PipeDesc(C.Structure):
    _fields_ = [
        ('tracer', Tracer * 2), ('same_tracer', C.c_int32), ('growth_rate_slot', C.c_int32),
        ('growth_rate_default', C.c_double), ('fast_metals', C.c_int32), ('pk_lin_kind', C.c_int32),
        ('is_peak', C.c_int32),
        ('uvb', C.c_int32), ('heii', C.c_int32),
        ('bias_gamma_slot', C.c_int32), ('bias_prim_slot', C.c_int32), ('lambda_uv_slot', C.c_int32),
        ('bias_gamma_e_slot', C.c_int32), ('lambda_heii_slot', C.c_int32),
        ('hcd_model', C.c_int32), ('bias_hcd_slot', C.c_int32), ('beta_hcd_slot', C.c_int32),
        ('l0_hcd_slot', C.c_int32), ('l0_default', C.c_double),
        ('nl_model', C.c_int32), ('arinyo_slot', C.c_int32 * 6), ('arinyo_power', C.c_double),
        ('gk_table', C.c_int32), ('mock_los_slot', C.c_int32), ('mock_los_size', C.c_double),
        ('peak_nl', C.c_int32), ('sigma_nl_par_slot', C.c_int32), ('sigma_nl_per_slot', C.c_int32),
        ('n_smooth', C.c_int32), ('smooth_par_slot', C.c_int32 * VMX_MAX_SMOOTH),
        ('smooth_per_slot', C.c_int32 * VMX_MAX_SMOOTH), ('smooth_weight', C.c_double * VMX_MAX_SMOOTH),
        ('exp_par_slot', C.c_int32), ('exp_per_slot', C.c_int32),
        ('vd_kind', C.c_int32), ('damping_scale', C.c_double), ('damping_power', C.c_int32),
        ('n_ell', C.c_int32), ('scale_mode', C.c_int32), ('scale_slot', C.c_int32 * 2),
        ('drp_slot', C.c_int32), ('croom_slot', C.c_int32 * 2), ('radiation', C.c_int32),
        ('rad_slot', C.c_int32 * 4), ('uv_shotnoise', C.c_int32), ('uvsn_slot', C.c_int32 * 3),
        ('single_ell', C.c_int32), ('z_eff', C.c_double)]


class MetalDesc(C.Structure):
    _fields_ = [('pipeline', C.c_int32), ('tracer', Tracer * 2), ('same_tracer', C.c_int32),
                ('growth_rate_slot', C.c_int32), ('growth_rate_default', C.c_double),
                ('extra_bias_slot', C.c_int32), ('apply_bias', C.c_int32), ('multiplicity', C.c_double),
                ('amplitude_slot', C.c_int32), ('in_direct', C.c_int32)]


class ItemDesc(C.Structure):
    _fields_ = [('n_model', C.c_int32), ('n_dist', C.c_int32), ('pipe_peak', C.c_int32),
                ('pipe_smooth', C.c_int32), ('bao_amp_slot', C.c_int32)]


VMX_FIT_MAXN, VMX_FIT_MAX_STAGES = 32, 2


class FitStage(C.Structure):
    _fields_ = [('n', C.c_int32), ('col', C.c_int32 * VMX_FIT_MAXN), ('has_lo', C.c_int32 * VMX_FIT_MAXN),
                ('has_hi', C.c_int32 * VMX_FIT_MAXN), ('lo', C.c_double * VMX_FIT_MAXN), ('hi', C.c_double * VMX_FIT_MAXN),
                ('err', C.c_double * VMX_FIT_MAXN)]


class FitSpec(C.Structure):
    _fields_ = [('n_stages', C.c_int32), ('n_params', C.c_int32), ('iterate', C.c_int32), ('maxfcn', C.c_int32),
                ('up', C.c_double), ('tol', C.c_double), ('stage', FitStage * VMX_FIT_MAX_STAGES)]


class MockStream(C.Structure):
    _fields_ = [('n_mocks', C.c_int32), ('wave', C.c_int32), ('draws', C.POINTER(C.c_double)), ('stride', C.c_int64),
                ('n_drawn', C.POINTER(C.c_int32)), ('timeout_seconds', C.c_double)]


class FitOptions(C.Structure):
    _fields_ = [('const_hint', C.c_int32), ('chunk', C.c_int32), ('lanes', C.c_int32), ('reserved', C.c_int32),
                ('mocks', C.POINTER(MockStream))]


class FitResultArrays(C.Structure):
    _fields_ = [('x', C.POINTER(C.c_double)), ('ext', C.POINTER(C.c_double)), ('V', C.POINTER(C.c_double)),
                ('fval', C.POINTER(C.c_double)), ('edm', C.POINTER(C.c_double)), ('flags', C.POINTER(C.c_int32)),
                ('nfcn', C.POINTER(C.c_int64)), ('n_iter', C.POINTER(C.c_int32))]


class FitStats(C.Structure):
    _fields_ = [('rounds', C.c_int64), ('evaluations', C.c_int64), ('engine_calls', C.c_int64), ('fits_unfinished', C.c_int64),
                ('calls_by_batch', C.c_int64 * 8), ('evaluations_by_batch', C.c_int64 * 8),
                ('seconds', C.c_double), ('seconds_setup', C.c_double), ('seconds_rounds', C.c_double),
                ('seconds_host_waiting', C.c_double), ('gpu_idle_seconds_between_rounds', C.c_double),
                ('seconds_waiting_for_draws', C.c_double), ('seconds_enqueuing_waves', C.c_double),
                ('seconds_enqueuing_rounds', C.c_double), ('seconds_enqueuing_calls', C.c_double)]


VMX_ENS_MAXN = 64


class EnsembleSpec(C.Structure):
    _fields_ = [('n_params', C.c_int32), ('n', C.c_int32), ('col', C.POINTER(C.c_int32)), ('lo', C.POINTER(C.c_double)),
                ('hi', C.POINTER(C.c_double)), ('a', C.c_double), ('log_norm', C.c_double), ('seed', C.c_uint64),
                ('stream', C.c_uint64), ('theta_fixed', C.POINTER(C.c_double))]


class EnsembleOptions(C.Structure):
    _fields_ = [('const_hint', C.c_int32), ('chunk', C.c_int32), ('lanes', C.c_int32), ('reserved', C.c_int32)]


class EnsembleStats(C.Structure):
    _fields_ = [('steps', C.c_int64), ('proposals', C.c_int64), ('accepted', C.c_int64), ('rejected_outside_box', C.c_int64),
                ('rejected_failed_model', C.c_int64), ('engine_calls', C.c_int64), ('seconds', C.c_double),
                ('seconds_enqueuing', C.c_double), ('host_synchronisations', C.c_int64), ('const_hint', C.c_int32),
                ('lanes', C.c_int32)]


class EnsembleMoves(C.Structure):
    _fields_ = [('weights', C.c_double * 3), ('gamma0', C.c_double), ('sigma', C.c_double), ('gamma_s', C.c_double),
                ('flags', C.c_uint32), ('reserved', C.c_uint32)]


class EnsembleCov(C.Structure):
    _fields_ = [('weight', C.c_double), ('scale', C.c_double), ('flags', C.c_uint32), ('reserved', C.c_uint32)]


class EnsembleAdapt(C.Structure):
    _fields_ = [('lag', C.c_double), ('time', C.c_double), ('adapt_until', C.c_int64), ('flags', C.c_uint32), ('reserved', C.c_uint32)]


VMX_SLICE_COUNTS = 8
SLICE_COUNT_NAMES = ('updates', 'moved', 'rows', 'expansions', 'contractions', 'box', 'failed', 'capped')


class EnsembleSlice(C.Structure):
    _fields_ = [('mu0', C.c_double), ('tune_steps', C.c_int32), ('max_expansions', C.c_int32), ('max_contractions', C.c_int32),
                ('flags', C.c_int32)]


VMX_NS_MAXN = 32
VMX_NS_MAX_LIVE = 4096
NESTED_STOP = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double))


class NestedSpec(C.Structure):
    _fields_ = [('n_params', C.c_int32), ('n', C.c_int32), ('col', C.POINTER(C.c_int32)), ('lo', C.POINTER(C.c_double)),
                ('hi', C.POINTER(C.c_double)), ('nlive', C.c_int32), ('K', C.c_int32), ('num_repeats', C.c_int32),
                ('reserved', C.c_int32), ('log_norm', C.c_double), ('seed', C.c_uint64), ('stream', C.c_uint64),
                ('theta_fixed', C.POINTER(C.c_double))]


class NestedOptions(C.Structure):
    _fields_ = [('const_hint', C.c_int32), ('chunk', C.c_int32), ('lanes', C.c_int32), ('draw_live', C.c_int32),
                ('stop', NESTED_STOP), ('user', C.c_void_p)]


class NestedStats(C.Structure):
    _fields_ = [('iterations', C.c_int64), ('rounds', C.c_int64), ('rows', C.c_int64), ('rows_own_position', C.c_int64),
                ('engine_calls', C.c_int64), ('host_waits', C.c_int64), ('seconds', C.c_double), ('seconds_enqueuing', C.c_double),
                ('const_hint', C.c_int32), ('lanes', C.c_int32)]


NESTED_SET_STOP = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double))


class NestedSetOptions(C.Structure):
    _fields_ = [('const_hint', C.c_int32), ('chunk', C.c_int32), ('lanes', C.c_int32), ('draw_live', C.c_int32),
                ('stop', NESTED_SET_STOP), ('user', C.c_void_p)]


VMX_NS_KNN = 8
VMX_NS_MAX_CLUSTERS = 8
VMX_NS_CLUSTER = 1


class NestedClusters(C.Structure):
    _fields_ = [('live_cluster', C.POINTER(C.c_int32)), ('next_id', C.POINTER(C.c_int32)), ('dead_cluster', C.POINTER(C.c_int32)),
                ('flags', C.c_uint32), ('reserved', C.c_uint32)]


class NestedPhantoms(C.Structure):
    _fields_ = [('fraction', C.c_double), ('capacity', C.c_int64), ('u', C.POINTER(C.c_double)), ('lnl', C.POINTER(C.c_double)),
                ('birth', C.POINTER(C.c_double)), ('iteration', C.POINTER(C.c_int64)), ('thread', C.POINTER(C.c_int32)),
                ('repeat', C.POINTER(C.c_int32)), ('cluster', C.POINTER(C.c_int32)), ('count', C.c_int64),
                ('flags', C.c_uint32), ('reserved', C.c_uint32)]


class NestedSetPhantoms(C.Structure):
    _fields_ = [('fraction', C.c_double), ('capacity', C.c_int64), ('u', C.POINTER(C.c_double)), ('lnl', C.POINTER(C.c_double)),
                ('birth', C.POINTER(C.c_double)), ('iteration', C.POINTER(C.c_int64)), ('thread', C.POINTER(C.c_int32)),
                ('repeat', C.POINTER(C.c_int32)), ('count', C.POINTER(C.c_int64)), ('flags', C.c_uint32), ('reserved', C.c_uint32)]


class PhantomArrays:
    """The phantom record of one call of :meth:`Engine.nested_run_many` (include/vegamx.h: vmx_nested_set_phantoms): the kept
    ``fraction``, ``capacity`` rows per run and the host arrays ``u`` [E, capacity, n], ``lnl``, ``birth``, ``iteration`` (int64),
    ``thread``, ``repeat`` [E, capacity] and ``count`` int64 [E] (out: the rows every run wrote); ``flags``: 0."""

    def __init__(self, runs, capacity, n, fraction, flags=0):
        self.E, self.capacity, self.n, self.fraction, self.flags = int(runs), int(capacity), int(n), float(fraction), int(flags)
        rows = max(self.capacity, 0)
        self.u, self.lnl, self.birth = np.empty((self.E, rows, self.n)), np.empty((self.E, rows)), np.empty((self.E, rows))
        self.iteration = np.empty((self.E, rows), dtype=np.int64)
        self.thread, self.repeat = np.empty((self.E, rows), dtype=np.int32), np.empty((self.E, rows), dtype=np.int32)
        self.count = np.zeros(self.E, dtype=np.int64)

    def struct(self):
        return NestedSetPhantoms(self.fraction, self.capacity, _dp(self.u), _dp(self.lnl), _dp(self.birth),
                                 self.iteration.ctypes.data_as(C.POINTER(C.c_int64)), _ip(self.thread), _ip(self.repeat),
                                 self.count.ctypes.data_as(C.POINTER(C.c_int64)), self.flags, 0)

    def run(self, e):
        """Run ``e``'s rows in the order they were written: (u [N, n], lnl [N], birth [N], tag [N, 3] int64)."""
        c = int(self.count[e])
        return (self.u[e, :c].copy(), self.lnl[e, :c].copy(), self.birth[e, :c].copy(),
                np.stack([self.iteration[e, :c], self.thread[e, :c].astype(np.int64), self.repeat[e, :c].astype(np.int64)], axis=1))


VMX_SMC_MAX_PARTICLES = 4096
VMX_SMC_REC = 8


class SmcSpec(C.Structure):
    _fields_ = [('n_params', C.c_int32), ('n', C.c_int32), ('col', C.POINTER(C.c_int32)), ('lo', C.POINTER(C.c_double)),
                ('hi', C.POINTER(C.c_double)), ('N', C.c_int32), ('sweeps', C.c_int32), ('ess', C.c_double),
                ('log_norm', C.c_double), ('seed', C.c_uint64), ('stream', C.c_uint64), ('theta_fixed', C.POINTER(C.c_double))]


class SmcOptions(C.Structure):
    _fields_ = [('const_hint', C.c_int32), ('chunk', C.c_int32), ('lanes', C.c_int32), ('draw', C.c_int32)]


class SmcKeep(C.Structure):
    _fields_ = [('rec_u', C.POINTER(C.c_double)), ('topups_left', C.POINTER(C.c_int32)), ('flags', C.c_int32)]


class SmcStats(C.Structure):
    _fields_ = [('stages', C.c_int64), ('sweeps', C.c_int64), ('rows', C.c_int64), ('rows_own_position', C.c_int64),
                ('accepted', C.c_int64), ('rejected_failed_model', C.c_int64), ('engine_calls', C.c_int64),
                ('host_waits', C.c_int64), ('seconds', C.c_double), ('seconds_enqueuing', C.c_double), ('const_hint', C.c_int32),
                ('lanes', C.c_int32)]


FIT_BATCH_BINS = ('1', '2..4', '5..16', '17..64', '65..256', '257..1024', '1025..4096', '4097..')


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _in_place(dtype, **arrays):
    """The named arrays are what the library can update in place: C-contiguous NumPy arrays of ``dtype``."""
    for name, arr in arrays.items():
        if not (isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.flags.c_contiguous):
            raise ValueError(f'{name}: a C-contiguous {np.dtype(dtype).name} array (updated in place)')


def _ensemble_moves(moves):
    """The mapping ``moves`` of the ensemble entries as the library reads it (None: none)."""
    if moves is None:
        return None
    return EnsembleMoves((C.c_double * 3)(*(float(w) for w in moves['weights'][:3])), float(moves['gamma0']), float(moves['sigma']),
                         float(moves['gamma_s']), int(moves.get('flags', 0)), 0)


def _ensemble_cov(moves):
    """The covariance move of the mapping ``moves`` - a fourth weight and ``cov_scale`` - as vmx_ensemble_run_many_cov reads it
    (None: the mapping has three weights)."""
    if moves is None or len(moves['weights']) < 4:
        return None
    return EnsembleCov(float(moves['weights'][3]), float(moves['cov_scale']), int(moves.get('cov_flags', 0)), 0)


def _stats_dict(stats):
    return {name: getattr(stats, name) for name, _ in stats._fields_}


def load_library():
    """Load libvegamx.so (built in-tree by ``__graft_entry__.build()``); no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get('VEGAMX_LIBRARY', _LIB_PATH))
    if not path.is_file():
        raise EngineError(f'{path} not found: build it with `python -c "import __graft_entry__ as g; '
                          'g.build()"`. The vegamx engine has no CPU fallback.')
    lib = C.CDLL(str(path))
    lib.vmx_last_error.restype = C.c_char_p
    lib.vmx_kernel_name.restype = C.c_char_p
    lib.vmx_kernel_name.argtypes = [C.c_int32]
    lib.vmx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.vmx_destroy.argtypes = [C.c_void_p]
    lib.vmx_destroy.restype = None
    dptr, iptr = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.vmx_set_template.argtypes = [C.c_void_p, C.c_int32, dptr, dptr, dptr, dptr, dptr, C.c_int32]
    lib.vmx_set_fftlog.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32, C.c_double, C.c_double, C.c_int32]
    lib.vmx_add_gk_table.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.vmx_add_gk_table_mock.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.vmx_set_spline_extrapolation.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_set_fftlog_padding.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.vmx_set_fvoigt_table.argtypes = [C.c_void_p, dptr, dptr, C.c_int32]
    lib.vmx_add_pipeline.argtypes = [C.c_void_p, C.POINTER(PipeDesc), C.c_int32, dptr, dptr, dptr, dptr, dptr]
    lib.vmx_add_item.argtypes = [C.c_void_p, C.POINTER(ItemDesc)]
    lib.vmx_set_shotnoise_table.argtypes = [C.c_void_p, dptr, C.c_int32, C.c_double, C.c_double]
    lib.vmx_item_set_additive_template.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32, C.c_int32, C.c_double]
    lib.vmx_pipeline_set_odd_terms.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32, C.c_double, C.c_double,
                                               C.c_int32, C.c_int32, iptr]
    lib.vmx_pipeline_set_odd_operator.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32, C.c_int32]
    lib.vmx_item_add_metal.argtypes = [C.c_void_p, C.c_int32, C.POINTER(MetalDesc)]
    lib.vmx_item_add_broadband.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, iptr, dptr,
                                           C.c_int32]
    lib.vmx_item_set_matrix.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dptr]
    lib.vmx_item_set_matrix_csr.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), iptr, dptr]
    lib.vmx_item_set_mask.argtypes = [C.c_void_p, C.c_int32, iptr, C.c_int32]
    lib.vmx_item_set_data.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32]
    lib.vmx_set_global_invcov.argtypes = [C.c_void_p, dptr, C.c_int32]
    lib.vmx_item_set_mock_pool.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32, C.c_int32]
    lib.vmx_set_mock_index.argtypes = [C.c_void_p, iptr, C.c_int32]
    lib.vmx_item_set_mock_factor.argtypes = [C.c_void_p, C.c_int32, dptr, dptr, C.c_int32]
    lib.vmx_item_get_mock_pool.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32, C.c_int32]
    lib.vmx_host_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int64]
    lib.vmx_host_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.vmx_add_prior.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double]
    lib.vmx_finalize.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.vmx_model_size.argtypes = [C.c_void_p]
    lib.vmx_pipeline_column.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_eval.argtypes = [C.c_void_p, dptr, C.c_int32, dptr, dptr, iptr]
    lib.vmx_eval_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vmx_sync.argtypes = [C.c_void_p]
    lib.vmx_eval_device_mocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vmx_fit_migrad.argtypes = [C.c_void_p, C.POINTER(FitSpec), C.c_int32, dptr, iptr, C.POINTER(FitOptions),
                                   C.POINTER(FitResultArrays), C.POINTER(FitStats)]
    lib.vmx_ensemble_run.argtypes = [C.c_void_p, C.POINTER(EnsembleSpec), C.c_int32, dptr, dptr, C.POINTER(C.c_int64), C.c_int64,
                                     C.c_int32, C.c_int32, dptr, dptr, C.POINTER(EnsembleOptions), C.POINTER(EnsembleStats)]
    lib.vmx_ensemble_run_many.argtypes = [C.c_void_p, C.POINTER(EnsembleSpec), C.c_int32, C.c_int32, C.POINTER(C.c_uint64), iptr, dptr,
                                          dptr, C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.c_int32, dptr, dptr,
                                          C.POINTER(EnsembleOptions), C.POINTER(EnsembleStats), C.POINTER(C.c_int64)]
    lib.vmx_ensemble_run_many_moves.argtypes = lib.vmx_ensemble_run_many.argtypes + [C.POINTER(EnsembleMoves)]
    lib.vmx_ensemble_run_many_cov.argtypes = lib.vmx_ensemble_run_many_moves.argtypes + [C.POINTER(EnsembleCov), C.POINTER(C.c_int64)]
    lib.vmx_ensemble_cov_factor.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, dptr, dptr, dptr, iptr]
    lib.vmx_ensemble_run_pt.argtypes = [C.c_void_p, C.POINTER(EnsembleSpec), C.c_int32, C.c_int32, C.c_int32, dptr, C.POINTER(C.c_uint64),
                                        iptr, dptr, dptr, C.POINTER(C.c_int64), C.c_int64, C.c_int32, C.c_int32, C.c_int32, dptr, dptr,
                                        C.POINTER(EnsembleOptions), C.POINTER(EnsembleStats), C.POINTER(C.c_int64),
                                        C.POINTER(EnsembleMoves), C.POINTER(C.c_int64)]
    lib.vmx_ensemble_run_pt_adapt.argtypes = lib.vmx_ensemble_run_pt.argtypes + [C.POINTER(EnsembleAdapt), dptr, C.POINTER(C.c_int64)]
    lib.vmx_ensemble_run_slice.argtypes = lib.vmx_ensemble_run_many.argtypes[:-1] + [C.POINTER(EnsembleSlice), dptr, C.POINTER(C.c_int64)]
    i64p = C.POINTER(C.c_int64)
    lib.vmx_chain_store_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]
    lib.vmx_chain_store_destroy.argtypes = [C.c_void_p]
    lib.vmx_chain_store_reserve.argtypes = [C.c_void_p, C.c_int64]
    lib.vmx_chain_store_rows.argtypes = [C.c_void_p, i64p]
    lib.vmx_chain_store_append.argtypes = [C.c_void_p, C.c_int64, dptr, dptr]
    lib.vmx_chain_store_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, dptr, dptr]
    lib.vmx_chain_store_summary.argtypes = [C.c_void_p, C.c_int64, C.c_double, i64p, dptr, dptr, dptr, i64p]
    lib.vmx_chain_store_order_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int32, i64p, dptr]
    lib.vmx_chain_store_best.argtypes = [C.c_void_p, C.c_int64, dptr, i64p, C.POINTER(C.c_int32), dptr]
    lib.vmx_ensemble_set_chain_store.argtypes = [C.c_void_p, C.c_void_p]
    u64p = C.POINTER(C.c_uint64)
    lib.vmx_sample_store_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]
    lib.vmx_sample_store_destroy.argtypes = [C.c_void_p]
    lib.vmx_sample_store_put.argtypes = [C.c_void_p, C.c_int32, C.c_int64, dptr, dptr, dptr]
    lib.vmx_sample_store_counts.argtypes = [C.c_void_p, i64p]
    lib.vmx_sample_store_fetch.argtypes = [C.c_void_p, C.c_int32, dptr, dptr, dptr]
    lib.vmx_sample_store_summary.argtypes = [C.c_void_p, dptr, dptr, dptr, dptr, u64p, dptr]
    lib.vmx_sample_store_order_stats.argtypes = [C.c_void_p, C.c_int32, u64p, dptr]
    lib.vmx_sample_store_best.argtypes = [C.c_void_p, dptr, i64p, dptr]
    lib.vmx_nested_run.argtypes = [C.c_void_p, C.POINTER(NestedSpec), dptr, dptr, C.POINTER(C.c_int64), C.c_int32, dptr, dptr, iptr,
                                   C.POINTER(NestedOptions), C.POINTER(NestedStats)]
    lib.vmx_nested_run_clustered.argtypes = lib.vmx_nested_run.argtypes + [C.POINTER(NestedClusters)]
    lib.vmx_nested_run_phantoms.argtypes = lib.vmx_nested_run_clustered.argtypes + [C.POINTER(NestedPhantoms)]
    lib.vmx_nested_cluster_points.argtypes = [C.c_int32, dptr, C.c_int32, C.c_int32, iptr, iptr, iptr, iptr, iptr, dptr, dptr]
    lib.vmx_nested_run_many.argtypes = [C.c_void_p, C.POINTER(NestedSpec), C.c_int32, C.POINTER(C.c_uint64), iptr, dptr, dptr,
                                        C.POINTER(C.c_int64), iptr, C.c_int32, dptr, dptr, iptr, iptr, C.POINTER(NestedSetOptions),
                                        C.POINTER(NestedStats), C.POINTER(C.c_int64)]
    lib.vmx_nested_run_many_phantoms.argtypes = lib.vmx_nested_run_many.argtypes + [C.POINTER(NestedSetPhantoms)]
    lib.vmx_smc_run.argtypes = [C.c_void_p, C.POINTER(SmcSpec), dptr, dptr, C.POINTER(C.c_int64), dptr, dptr, C.c_int32, dptr, dptr,
                                iptr, C.POINTER(SmcOptions), C.POINTER(SmcStats)]
    lib.vmx_smc_run_many.argtypes = [C.c_void_p, C.POINTER(SmcSpec), C.c_int32, C.POINTER(C.c_uint64), iptr, dptr, dptr,
                                     C.POINTER(C.c_int64), dptr, dptr, iptr, C.c_int32, dptr, dptr, iptr, iptr, C.POINTER(SmcOptions),
                                     C.POINTER(SmcStats), C.POINTER(C.c_int64)]
    lib.vmx_smc_run_kept.argtypes = lib.vmx_smc_run.argtypes[:11] + [C.POINTER(SmcKeep)] + lib.vmx_smc_run.argtypes[11:]
    lib.vmx_smc_run_many_kept.argtypes = lib.vmx_smc_run_many.argtypes[:16] + [C.POINTER(SmcKeep)] + lib.vmx_smc_run_many.argtypes[16:]
    lib.vmx_derived_const_hint.argtypes = [C.c_void_p, iptr]
    lib.vmx_set_constant_nl_hint.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_set_direct_pk.argtypes = [C.c_void_p, dptr, C.c_int32, C.c_int32]
    lib.vmx_set_linear_spectra.argtypes = [C.c_void_p, dptr, dptr, dptr, C.c_int32]
    lib.vmx_item_set_marg_matrix.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32, C.c_int32]
    lib.vmx_marg_coeff.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int32]
    lib.vmx_marg_coeff_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.vmx_marg_layout.argtypes = [C.c_void_p, C.c_int32, iptr, iptr]
    lib.vmx_set_quadratic_form.argtypes = [C.c_void_p, dptr]
    lib.vmx_set_quadratic_form_kind.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_set_static_poly.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_set_mu_quadrature.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_get_mu_nodes.argtypes = [C.c_void_p, dptr, dptr, C.c_int32]
    lib.vmx_set_mu_rule_box.argtypes = [C.c_void_p, C.c_int32, iptr, dptr, dptr]
    lib.vmx_stream.argtypes = [C.c_void_p]
    lib.vmx_stream.restype = C.c_void_p
    lib.vmx_last_stream.argtypes = [C.c_void_p]
    lib.vmx_last_stream.restype = C.c_void_p
    lib.vmx_set_lanes.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_debug_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, dptr, C.c_int64]
    lib.vmx_debug_read.restype = C.c_int64
    lib.vmx_debug_math.argtypes = [C.c_void_p, C.c_int32, dptr, C.c_int64, dptr]
    lib.vmx_debug_poison_scratch.argtypes = [C.c_int]
    lib.vmx_debug_poison_scratch.restype = C.c_int
    lib.vmx_matvec_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_void_p]
    lib.vmx_item_set_metal_static.argtypes = [C.c_void_p, C.c_int32, C.c_int32, dptr, C.c_int32]
    lib.vmx_item_set_metal_basis.argtypes = [C.c_void_p, C.c_int32, C.c_int32, dptr, C.c_int32]
    lib.vmx_item_set_metal_kron.argtypes = [C.c_void_p, C.c_int32, C.c_int32, dptr, C.c_int32, dptr, C.c_int32]
    lib.vmx_set_metal_beta_override.argtypes = [C.c_void_p, C.c_int32, C.c_double]
    lib.vmx_set_parameter_transform.argtypes = [C.c_void_p, dptr, dptr]
    lib.vmx_matmul_host.argtypes = [C.c_void_p, dptr, C.c_int32, C.c_int32, dptr, C.c_int32, dptr]
    lib.vmx_pipeline_set_tracer_evolution.argtypes = [C.c_void_p, C.c_int32, dptr, dptr, C.c_int32]
    lib.vmx_set_profiling.argtypes = [C.c_void_p, C.c_int32]
    lib.vmx_set_profiling_mask.argtypes = [C.c_void_p, C.c_uint32]
    lib.vmx_get_timings.argtypes = [C.c_void_p, dptr, C.POINTER(C.c_int64), C.c_int32]
    lib.vmx_struct_size.argtypes = [C.c_int32]
    for which, struct in enumerate((Tracer, PipeDesc, MetalDesc, ItemDesc, FitSpec, FitOptions, FitResultArrays, FitStats,
                                    EnsembleSpec, EnsembleOptions, EnsembleStats, NestedSpec, NestedOptions, NestedStats,
                                    SmcSpec, SmcOptions, SmcStats, NestedClusters, NestedSetOptions, NestedPhantoms,
                                    NestedSetPhantoms, SmcKeep, None, EnsembleMoves, EnsembleAdapt, EnsembleSlice)):
        if struct is None:          # (an index that names no struct)
            continue
        if lib.vmx_struct_size(which) != C.sizeof(struct):
            raise EngineError(f'ABI mismatch: {struct.__name__} is {C.sizeof(struct)} bytes here, '
                              f'{lib.vmx_struct_size(which)} in libvegamx.so')
    _lib = lib
    return lib


@contextlib.contextmanager
def poison_scratch(on=True):
    """While the block runs, device scratch of plain doubles that a call takes without clearing it reads as NaN (include/vegamx.h:
    vmx_debug_poison_scratch; process-wide, for tests).  The switch is put back on the way out."""
    lib = load_library()
    before = lib.vmx_debug_poison_scratch(1 if on else 0)
    try:
        yield
    finally:
        lib.vmx_debug_poison_scratch(before)


def cluster_points(u, prev_id, next_id, device=0):
    """The clustering of one nested-sampling iteration on the device (include/vegamx.h: vmx_nested_cluster_points): ``u`` [m, n],
    ``prev_id`` [m].  dict(ids [m], k, n_clusters, next_id, mean [n_clusters, n], C [n_clusters, n, n]) - the entries of the same
    names of :func:`vega_amd.nested.cluster_points`."""
    lib = load_library()
    u = np.ascontiguousarray(u, dtype=np.float64)
    prev_id = np.ascontiguousarray(prev_id, dtype=np.int32)
    if u.ndim != 2 or prev_id.shape != (u.shape[0],):
        raise ValueError('u [m, n], prev_id [m]')
    m, n = u.shape
    ids = np.zeros(m, dtype=np.int32)
    nxt, k, nc = (np.array([v], dtype=np.int32) for v in (int(next_id), 0, 0))
    mean, fac = np.zeros((VMX_NS_MAX_CLUSTERS, n)), np.zeros((VMX_NS_MAX_CLUSTERS, n, n))
    rc = lib.vmx_nested_cluster_points(int(device), _dp(u), m, n, _ip(prev_id), _ip(nxt), _ip(ids), _ip(k), _ip(nc), _dp(mean), _dp(fac))
    if rc != 0:
        raise EngineError(lib.vmx_last_error().decode())
    return dict(ids=ids, k=int(k[0]), n_clusters=int(nc[0]), next_id=int(nxt[0]), mean=mean[:int(nc[0])], C=fac[:int(nc[0])])


EXPORTED_SYMBOLS = [
    'vmx_last_error', 'vmx_struct_size', 'vmx_create', 'vmx_destroy', 'vmx_set_template', 'vmx_set_fftlog', 'vmx_set_fftlog_padding', 'vmx_set_spline_extrapolation', 'vmx_set_fvoigt_table', 'vmx_add_gk_table', 'vmx_add_gk_table_mock',
    'vmx_add_pipeline', 'vmx_pipeline_set_tracer_evolution', 'vmx_pipeline_set_odd_terms', 'vmx_pipeline_set_odd_operator', 'vmx_set_shotnoise_table',
    'vmx_item_set_additive_template', 'vmx_add_item', 'vmx_item_add_metal', 'vmx_item_set_metal_static', 'vmx_item_set_metal_basis', 'vmx_item_set_metal_kron', 'vmx_set_metal_beta_override', 'vmx_item_add_broadband', 'vmx_item_set_matrix', 'vmx_item_set_matrix_csr',
    'vmx_item_set_mask', 'vmx_item_set_data', 'vmx_item_set_mock_pool', 'vmx_set_mock_index', 'vmx_item_set_mock_factor', 'vmx_item_get_mock_pool', 'vmx_host_alloc', 'vmx_host_free', 'vmx_set_global_invcov', 'vmx_add_prior', 'vmx_finalize',
    'vmx_model_size', 'vmx_pipeline_column', 'vmx_eval', 'vmx_eval_device', 'vmx_eval_device_mocks', 'vmx_fit_migrad', 'vmx_ensemble_run', 'vmx_ensemble_run_many', 'vmx_ensemble_run_many_moves', 'vmx_ensemble_run_many_cov', 'vmx_ensemble_cov_factor', 'vmx_ensemble_run_pt', 'vmx_ensemble_run_pt_adapt', 'vmx_ensemble_run_slice', 'vmx_chain_store_create', 'vmx_chain_store_destroy', 'vmx_chain_store_reserve', 'vmx_chain_store_rows', 'vmx_chain_store_append', 'vmx_chain_store_fetch', 'vmx_chain_store_summary', 'vmx_chain_store_order_stats', 'vmx_chain_store_best', 'vmx_ensemble_set_chain_store', 'vmx_sample_store_create', 'vmx_sample_store_destroy', 'vmx_sample_store_put', 'vmx_sample_store_counts', 'vmx_sample_store_fetch', 'vmx_sample_store_summary', 'vmx_sample_store_order_stats', 'vmx_sample_store_best', 'vmx_nested_run', 'vmx_nested_run_clustered', 'vmx_nested_run_phantoms', 'vmx_nested_cluster_points', 'vmx_nested_run_many', 'vmx_nested_run_many_phantoms', 'vmx_smc_run', 'vmx_smc_run_many', 'vmx_smc_run_kept', 'vmx_smc_run_many_kept', 'vmx_derived_const_hint', 'vmx_sync', 'vmx_set_constant_nl_hint', 'vmx_set_direct_pk', 'vmx_set_linear_spectra', 'vmx_item_set_marg_matrix', 'vmx_marg_coeff', 'vmx_marg_coeff_device', 'vmx_marg_layout', 'vmx_set_quadratic_form', 'vmx_set_quadratic_form_kind', 'vmx_set_static_poly', 'vmx_set_mu_quadrature', 'vmx_set_mu_rule_box', 'vmx_get_mu_nodes', 'vmx_set_parameter_transform', 'vmx_stream', 'vmx_last_stream', 'vmx_set_lanes', 'vmx_debug_read', 'vmx_debug_math', 'vmx_debug_poison_scratch', 'vmx_matvec_device', 'vmx_matmul_host',
    'vmx_set_profiling', 'vmx_set_profiling_mask', 'vmx_get_timings', 'vmx_kernel_name']


# --------------------------------------------------------------------------------------
# lowering: Problem -> descriptors
# --------------------------------------------------------------------------------------
class Lowering:
    """Resolves every name-keyed lookup of the reference's per-call code into theta columns."""

    def __init__(self, problem, extra_names=()):
        self.prob = problem
        self.names = sorted(set(problem.params) | set(extra_names))
        self.slot = {n: i for i, n in enumerate(self.names)}
        self.theta0 = np.array([problem.params.get(n, 0.0) for n in self.names], dtype=np.float64)

    def s(self, name):
        return self.slot.get(name, -1) if name is not None else -1

    def need(self, name):
        if name not in self.slot:
            raise KeyError(f'parameter {name!r} is required by the configured model but missing from '
                           '[parameters]')
        return self.slot[name]

    # -- tracers (reference vega/utils.py:45-82; metals.py:289-293 for the beta override)
    def tracer(self, tr, pk_opts=None, xi_opts=None, beta_name=None):
        t = Tracer()
        t.bias_slot = self.s('bias_' + tr.name)
        t.bias_eta_slot = self.s('bias_eta_' + tr.name)
        t.beta_slot = self.s(beta_name or ('beta_' + tr.name))
        if (t.bias_slot >= 0) + (t.bias_eta_slot >= 0) + (t.beta_slot >= 0) < 2:
            raise KeyError('For each tracer, you need to specify two of these three: (bias, bias_eta, beta). '
                           f'Offending tracer: {tr.name}')
        if t.bias_slot >= 0 and t.beta_slot >= 0:
            t.bias_eta_slot = -1    # "If all three are given, we use bias and beta"
        t.is_lya = int(tr.name == 'LYA')
        t.discrete = int(tr.type == 'discrete')
        t.vd_sigma_slot = -1
        if pk_opts is not None and pk_opts.velocity_dispersion is not None and t.discrete:
            t.vd_sigma_slot = self.need(f'sigma_velo_disp_{pk_opts.velocity_dispersion}_{tr.name}')
        t.evol_kind = 0
        t.alpha_slot = -1
        if xi_opts is not None:
            if xi_opts.evol_model.get(tr.name, 'standard') == 'croom':
                if tr.name != 'QSO':
                    raise ValueError('the Croom bias evolution only applies to QSO')
                t.evol_kind = 1
            else:
                t.alpha_slot = self.need('alpha_' + tr.name)
        return t

    def scale(self, pipe, is_peak):
        """Static resolution of ScaleParameters.get_ap_at (reference scale_parameters.py:38-160)."""
        sc = self.prob.scale
        if pipe.metal_corr and not sc.metal_scaling:
            return SCALE_UNIT, (-1, -1)

        def bao():
            if sc.parametrisation == 'ap_at':
                return SCALE_AP_AT, (self.need('ap'), self.need('at'))
            if sc.parametrisation == 'aiso_epsilon':
                return SCALE_AISO_EPS, (self.need('aiso'), self.need('epsilon'))
            return SCALE_PHI_ALPHA, (self.need('phi'), self.need('alpha'))

        def fullshape():
            if sc.parametrisation != 'phi_alpha' and not sc.full_shape_alpha:
                raise ValueError('Only the "phi_alpha" parametrisation works with split full-shape. '
                                 'Set full-shape-alpha to True for other parametrisations.')
            if sc.parametrisation == 'ap_at':
                return SCALE_AP_AT, (self.need('ap_full'), self.need('at_full'))
            if sc.parametrisation == 'aiso_epsilon':
                return SCALE_AISO_EPS, (self.need('aiso_full'), self.need('epsilon_full'))
            phi = 'phi_full' if sc.full_shape else 'phi_smooth'
            if sc.full_shape_alpha:
                alpha = 'alpha_full'
            elif is_peak:
                alpha = 'alpha'
            elif sc.two_alpha_smooth:
                alpha = f'alpha_smooth_{pipe.corr_name}'
            else:
                alpha = 'alpha_smooth'
            return SCALE_PHI_ALPHA, (self.need(phi), self.need(alpha))

        if sc.full_shape:
            return fullshape()
        if is_peak:
            return bao()
        if sc.smooth_scaling:
            return fullshape()
        return SCALE_UNIT, (-1, -1)

    def pipeline(self, engine, pipe, component, fast_metals=False, beta_names=(None, None),
                 growth_rate_override=None):
        pk, xi = pipe.pk, pipe.xi
        if xi.single_multipole >= 0 and (xi.single_multipole % 2 or xi.single_multipole > xi.ell_max):
            raise ValueError(f'single_multipole = {xi.single_multipole} is not one of the even multipoles <= ell_max')
        if (xi.relativistic or xi.asymmetry) and self.prob.scale.two_alpha_smooth:
            raise NotImplementedError('odd multipoles with two-alpha-smooth: the reference looks up alpha_smooth_None for these terms '
                                      '(vega/correlation_func.py:514, vega/scale_parameters.py:155-156) - there is nothing to reproduce')
        if xi.ell_max not in (0, 2, 4, 6):
            raise NotImplementedError(f'ell_max = {xi.ell_max} is not supported (even, <= 6)')
        is_peak = component == 'peak'
        n1, n2 = pipe.tracer1.name, pipe.tracer2.name
        params = self.prob.params

        d = PipeDesc()
        d.tracer[0] = self.tracer(pipe.tracer1, pk, xi, beta_names[0])
        d.tracer[1] = self.tracer(pipe.tracer2, pk, xi, beta_names[1])
        d.same_tracer = int(n1 == n2)
        if growth_rate_override is not None:
            d.growth_rate_slot, d.growth_rate_default = -1, growth_rate_override
        else:
            d.growth_rate_slot, d.growth_rate_default = self.s('growth_rate'), DEFAULT_GROWTH_RATE
        d.fast_metals = int(fast_metals)
        d.pk_lin_kind = PKLIN[component]
        d.is_peak = int(is_peak)

        d.uvb, d.heii = int(pk.uvb), int(pk.heii)
        for f in ('bias_gamma_slot', 'bias_prim_slot', 'lambda_uv_slot', 'bias_gamma_e_slot', 'lambda_heii_slot'):
            setattr(d, f, -1)
        lya = 'LYA' in (n1, n2)
        if pk.uvb and lya:
            d.bias_gamma_slot, d.bias_prim_slot = self.need('bias_gamma'), self.need('bias_prim')
            d.lambda_uv_slot = self.need('lambda_uv')
        if pk.heii and lya:
            d.bias_gamma_e_slot, d.bias_prim_slot = self.need('bias_gamma_e'), self.need('bias_prim')
            d.lambda_heii_slot = self.need('lambda_HeII')
        if not lya:
            d.uvb = d.heii = 0

        d.hcd_model = HCD[pk.hcd_model or 'none'] if lya else 0
        d.bias_hcd_slot = d.beta_hcd_slot = d.l0_hcd_slot = -1
        d.l0_default = 1.0
        if d.hcd_model:
            # per-correlation names win (reference power_spectrum.py:281-288)
            name = f'bias_hcd_{pipe.corr_name}'
            d.bias_hcd_slot = self.slot[name] if name in self.slot else self.need('bias_hcd')
            name = f'beta_hcd_{pipe.corr_name}'
            d.beta_hcd_slot = self.slot[name] if name in self.slot else self.need('beta_hcd')
            d.l0_hcd_slot = (self.need('L0_hcd') if pk.hcd_model == 'Rogers' else
                             self.s('L0_sinc') if pk.hcd_model == 'sinc' else self.s('L0_fvoigt'))
            if pk.hcd_model == 'fvoigt':
                engine._set_fvoigt(pk.fvoigt_table)

        skip_nl = pk.skip_nl_in_peak and is_peak
        nl = 'none' if (pk.small_scale_nl is None or skip_nl) else pk.small_scale_nl
        d.arinyo_power = 0.0
        for i in range(6):
            d.arinyo_slot[i] = -1
        if nl == 'arinyo':
            two = 'LY' in n1 and 'LY' in n2
            one = 'LY' in n1 or 'LY' in n2
            d.arinyo_power = 1.0 if two else (0.5 if one else 0.0)
            if not one:
                nl = 'none'
            else:
                for i, key in enumerate(('q1', 'q2', 'kv', 'av', 'bv', 'kp')):
                    d.arinyo_slot[i] = self.s('dnl_arinyo_' + key) if key == 'q2' else self.need('dnl_arinyo_' + key)
        if nl == 'mcdonald' and not (n1 == 'LYA' and n2 == 'LYA'):
            raise ValueError('dnl_mcdonald only applies to LYA x LYA')
        d.nl_model = NL[nl]

        d.gk_table = -1
        d.mock_los_slot, d.mock_los_size = -1, 0.0
        bs_rp = bs_rt = mock_rp = mock_rt = 0.0
        if pk.use_gk:
            # frozen at the parameters of the first call (reference power_spectrum.py:139-141, :494-495)
            bs_rp = params.get(f'par binsize {pipe.dataset}', pk.bin_size_rp)
            bs_rt = params.get(f'per binsize {pipe.dataset}', pk.bin_size_rt)
        if pk.mock_bin_size is not None:
            # a second binning factor (reference power_spectrum.py:143-160); static unless it follows a parameter
            mock_rp = mock_rt = pk.mock_bin_size
            if pk.mock_los_smoothing in ('growth', 'amplitude'):
                # the binning kernel follows a parameter: static as long as that parameter is not sampled
                name = 'growth_rate' if pk.mock_los_smoothing == 'growth' else 'los_smooth_amp'
                sampled = set((self.prob.sample_params or {}).get('limits', {}))
                if name in sampled:
                    # ... and a factor of its own in the mu loop, per walker, when it is (the plain 1000-point loop: no
                    # tables, no node rule); the table keeps the transverse factor
                    d.mock_los_slot, d.mock_los_size = self.need(name), float(pk.mock_bin_size)
                    mock_rp = 0.0
                else:
                    mock_rp *= 1 + params[name]
            elif pk.mock_los_smoothing == 'only-los':
                mock_rt = 0.0
        if pk.use_gk or pk.mock_bin_size is not None:
            d.gk_table = engine._gk_table(float(bs_rp), float(bs_rt), float(mock_rp), float(mock_rt))

        d.peak_nl = int(is_peak)
        d.sigma_nl_par_slot, d.sigma_nl_per_slot = self.s('sigmaNL_par'), self.s('sigmaNL_per')
        if is_peak and d.sigma_nl_par_slot < 0 and d.sigma_nl_per_slot < 0:
            raise ValueError('No parameters for peak NL found. Add sigmaNL_par and/or sigmaNL_per.')
        if is_peak and (d.sigma_nl_par_slot < 0 or d.sigma_nl_per_slot < 0) and 'growth_rate' not in self.slot:
            raise ValueError('growth_rate is needed to derive the missing sigmaNL parameter')

        terms = []
        d.exp_par_slot = d.exp_per_slot = -1
        if pk.fullshape_smoothing is not None and not skip_nl:
            if pk.fullshape_smoothing == 'gauss':
                main1, main2 = n1 in ('LYA', 'QSO'), n2 in ('LYA', 'QSO')
                if 'par_sigma_smooth' in self.slot or 'per_sigma_smooth' in self.slot:
                    par, per = self.s('par_sigma_smooth'), self.s('per_sigma_smooth')
                    par, per = (per if par < 0 else par), (par if per < 0 else per)
                    terms.append((par, per, 1.0))
                elif ('par_sigma_smooth_metals' in self.slot and 'per_sigma_smooth_metals' in self.slot
                      and not (main1 and main2)):
                    terms.append((self.slot['par_sigma_smooth_metals'], self.slot['per_sigma_smooth_metals'], 1.0))
                else:
                    for n in (n1, n2):
                        terms.append((self.need(f'par_sigma_smooth_{n}'), self.need(f'per_sigma_smooth_{n}'), 0.5))
            else:
                terms.append((self.need('par_sigma_smooth'), self.need('per_sigma_smooth'), 0.5))
                d.exp_par_slot, d.exp_per_slot = self.need('par_exp_smooth'), self.need('per_exp_smooth')
        d.n_smooth = len(terms)
        for i in range(VMX_MAX_SMOOTH):
            par, per, w = terms[i] if i < len(terms) else (-1, -1, 0.0)
            d.smooth_par_slot[i], d.smooth_per_slot[i], d.smooth_weight[i] = par, per, w

        d.vd_kind = VD[pk.velocity_dispersion]
        if d.vd_kind and 'discrete' not in (pipe.tracer1.type, pipe.tracer2.type):
            raise ValueError('velocity dispersion needs a discrete tracer')
        d.damping_scale = pk.damping_scale if pk.damping_scale is not None else 0.0
        d.damping_power = pk.damping_power

        d.n_ell = xi.ell_max // 2 + 1
        d.single_ell = xi.single_multipole // 2 if xi.single_multipole >= 0 else -1
        mode, slots = self.scale(pipe, is_peak)
        d.scale_mode = mode
        d.scale_slot[0], d.scale_slot[1] = slots
        d.drp_slot = self.s(pipe.delta_rp_name)
        d.croom_slot[0], d.croom_slot[1] = self.s('croom_par0'), self.s('croom_par1')
        # (2: `rescale-coords-systematics` - the term is evaluated on the rescaled coordinates, reference
        # correlation_func.py:470-475, :681-684)
        d.radiation = int(xi.radiation) * (2 if xi.rescale_coords_systematics else 1)
        for i, key in enumerate(('strength', 'asymmetry', 'lifetime', 'decrease')):
            d.rad_slot[i] = self.need('qso_rad_' + key) if xi.radiation else -1
        d.uv_shotnoise = int(xi.uv_shotnoise) * (2 if xi.rescale_coords_systematics else 1)
        for i in range(3):
            d.uvsn_slot[i] = -1
        if xi.uv_shotnoise:
            gamma = 'bias_gamma' if 'bias_gamma' in self.slot else 'bias_gamma_e'
            d.uvsn_slot[0], d.uvsn_slot[1] = self.need('uv_shotnoise_amp'), self.need('lambda_uv')
            d.uvsn_slot[2] = self.need(gamma)
            engine._set_shotnoise_table()
        d.z_eff = self.prob.z_eff
        return d


class ChainStore:
    """The recorded rows of E ensembles of W walkers over n columns kept on the device (include/vegamx.h: vmx_chain_store_*),
    made by :meth:`Engine.chain_store`.  While it is attached (:meth:`Engine.attach_chain_store`) every ensemble run of the engine
    appends the rows it records, device to device."""

    def __init__(self, engine, E, W, n, capacity):
        self.engine, self.E, self.W, self.n, self.capacity = engine, int(E), int(W), int(n), int(capacity)
        self._h = None
        handle = C.c_void_p()
        engine._check(engine.lib.vmx_chain_store_create(engine._h, self.E, self.W, self.n, self.capacity, C.byref(handle)))
        self._h = handle

    def _handle(self):
        if not self._h or not self.engine._h:
            raise EngineError('the chain store is closed')
        return self._h

    @property
    def rows(self):
        """The rows stored, per ensemble."""
        rows = C.c_int64()
        self.engine._check(self.engine.lib.vmx_chain_store_rows(self._handle(), C.byref(rows)))
        return int(rows.value)

    def reserve(self, capacity):
        """Room for ``capacity`` rows per ensemble (it never shrinks); the stored rows are kept."""
        self.engine._check(self.engine.lib.vmx_chain_store_reserve(self._handle(), int(capacity)))
        self.capacity = max(self.capacity, int(capacity))

    def append(self, chain, chain_lnl):
        """Upload the host rows ``chain`` [E, rows, W, n] with ``chain_lnl`` [E, rows, W] behind the stored ones."""
        chain, chain_lnl = _f64(chain), _f64(chain_lnl)
        if chain.ndim != 4 or chain.shape[0::2] != (self.E, self.W) or chain.shape[3] != self.n or chain_lnl.shape != chain.shape[:3]:
            raise ValueError(f'chain [{self.E}, rows, {self.W}, {self.n}], chain_lnl [{self.E}, rows, {self.W}]')
        self.engine._check(self.engine.lib.vmx_chain_store_append(self._handle(), chain.shape[1], _dp(chain), _dp(chain_lnl)))

    def fetch(self, row0=0, rows=None, lnl=True):
        """The rows [row0, row0 + rows) (None: to the end) as (chain [E, rows, W, n], chain_lnl [E, rows, W]; None without
        ``lnl``) - the arrays the run entries return."""
        row0 = int(row0)
        rows = self.rows - row0 if rows is None else int(rows)
        chain = np.empty((self.E, max(rows, 0), self.W, self.n))
        chain_lnl = np.empty(chain.shape[:3]) if lnl else None
        self.engine._check(self.engine.lib.vmx_chain_store_fetch(self._handle(), row0, rows, _dp(chain), _dp(chain_lnl) if lnl else None))
        return chain, chain_lnl

    def summary(self, first=0, c=5, moments=True, tau=True):
        """The summary of the rows from ``first`` on, computed where they are (vega_amd/csrc/vmx_chain.h;
        :func:`vega_amd.ensemble.chain_summary` is the same numbers bit for bit): ``dict(count [E], mean [E, n], sd [E, n],
        covariance [E, n, n], tau [E, n], window [E, n], n_eff [E])``.  Without ``moments`` only count, tau, window and n_eff
        cross to the host, without ``tau`` only count, mean, sd and covariance."""
        E, n = self.E, self.n
        count = np.zeros(E, dtype=np.int64)
        out = dict(count=count)
        mean, cov = (np.empty((E, n)), np.empty((E, n, n))) if moments else (None, None)
        t, window = (np.empty((E, n)), np.zeros((E, n), dtype=np.int64)) if tau else (None, None)
        i64p = C.POINTER(C.c_int64)
        self.engine._check(self.engine.lib.vmx_chain_store_summary(
            self._handle(), int(first), float(c), count.ctypes.data_as(i64p), None if mean is None else _dp(mean),
            None if cov is None else _dp(cov), None if t is None else _dp(t), None if window is None else window.ctypes.data_as(i64p)))
        if moments:
            out.update(mean=mean, sd=np.sqrt(np.diagonal(cov, axis1=1, axis2=2)), covariance=cov)
        if tau:
            with np.errstate(divide='ignore', invalid='ignore'):
                out.update(tau=t, window=window, n_eff=count.astype(np.float64) / np.max(t, axis=1))
        return out

    def order_statistics(self, ranks, first=0):
        """Exact order statistics of every (ensemble, column) over the rows from ``first`` on, found where they are
        (vmx_chain_store_order_stats, vega_amd/csrc/vmx_chain_select.h; :func:`vega_amd.ensemble.chain_order_statistics` is the
        same bits): [E, n, R], entry r the ``ranks[r]``-th smallest of the (rows - first) W values - 1 .. 32 ranks in any order,
        repeats allowed."""
        ranks = np.ascontiguousarray(np.atleast_1d(ranks), dtype=np.int64)
        if ranks.ndim != 1:
            raise ValueError('ranks: a list of whole numbers')
        values = np.empty((self.E, self.n, max(ranks.size, 1)))
        self.engine._check(self.engine.lib.vmx_chain_store_order_stats(
            self._handle(), int(first), ranks.size, ranks.ctypes.data_as(C.POINTER(C.c_int64)), _dp(values)))
        return values

    def best(self, first=0, position=True):
        """The best row of every ensemble over the rows from ``first`` on (vmx_chain_store_best;
        :func:`vega_amd.ensemble.chain_best` is the same numbers): ``dict(lnl_max [E], best [E, n], best_row [E] (from row 0 of
        the store), best_walker [E])``; without ``position`` no ``best``."""
        top, row, walker = np.empty(self.E), np.zeros(self.E, dtype=np.int64), np.zeros(self.E, dtype=np.int32)
        at = np.empty((self.E, self.n)) if position else None
        self.engine._check(self.engine.lib.vmx_chain_store_best(
            self._handle(), int(first), _dp(top), row.ctypes.data_as(C.POINTER(C.c_int64)), _ip(walker), None if at is None else _dp(at)))
        out = dict(lnl_max=top, best_row=row, best_walker=walker)
        if position:
            out['best'] = at
        return out

    def close(self):
        if self._h and self.engine._h:
            if self.engine._attached is self:
                self.engine.attach_chain_store(None)
            self.engine.lib.vmx_chain_store_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SampleStore:
    """E weighted, ragged sample sets over n columns kept on the device (include/vegamx.h: vmx_sample_store_*), made by
    :meth:`Engine.sample_store`: the posterior samples of nested or SMC runs, reduced where they are.  vega_amd/weighted.py is the
    same numbers on the host, bit for bit."""

    def __init__(self, engine, E, n, capacity):
        self.engine, self.E, self.n, self.capacity = engine, int(E), int(n), int(capacity)
        self._h = None
        handle = C.c_void_p()
        engine._check(engine.lib.vmx_sample_store_create(engine._h, self.E, self.n, self.capacity, C.byref(handle)))
        self._h = handle

    def _handle(self):
        if not self._h or not self.engine._h:
            raise EngineError('the sample store is closed')
        return self._h

    def put(self, e, x, lnl, w):
        """Replace set ``e`` by the rows ``x`` [count, n], ``lnl`` [count] and weights ``w`` [count] (finite, >= 0; they need not
        sum to 1); count 0 empties it."""
        x, lnl, w = _f64(x), _f64(lnl), _f64(w)
        if x.ndim != 2 or x.shape[1] != self.n or lnl.shape != x.shape[:1] or w.shape != x.shape[:1]:
            raise ValueError(f'x [count, {self.n}], lnl [count], w [count]')
        self.engine._check(self.engine.lib.vmx_sample_store_put(self._handle(), int(e), x.shape[0], _dp(x), _dp(lnl), _dp(w)))

    def counts(self):
        """The rows of every set [E]."""
        counts = np.zeros(self.E, dtype=np.int64)
        self.engine._check(self.engine.lib.vmx_sample_store_counts(self._handle(), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        return counts

    def fetch(self, e):
        """Set ``e`` as (x [count, n], lnl [count], w [count])."""
        e = int(e)
        if not 0 <= e < self.E:
            raise ValueError(f'set: 0 .. {self.E - 1}')
        count = int(self.counts()[e])
        x, lnl, w = np.empty((count, self.n)), np.empty(count), np.empty(count)
        self.engine._check(self.engine.lib.vmx_sample_store_fetch(self._handle(), e, _dp(x), _dp(lnl), _dp(w)))
        return x, lnl, w

    def summary(self):
        """``dict(count [E], S [E], n_eff [E], mean [E, n], sd [E, n], covariance [E, n, n], total [E] (Python integers), w_max
        [E])`` of every set, computed where the rows are (vmx_sample_store_summary;
        :func:`vega_amd.weighted.weighted_summary` per set is the same bits)."""
        E, n = self.E, self.n
        S, n_eff, w_max, mean, cov = np.empty(E), np.empty(E), np.empty(E), np.empty((E, n)), np.empty((E, n, n))
        total = np.zeros(E, dtype=np.uint64)
        self.engine._check(self.engine.lib.vmx_sample_store_summary(
            self._handle(), _dp(S), _dp(n_eff), _dp(mean), _dp(cov), total.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(w_max)))
        with np.errstate(invalid='ignore'):
            sd = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
        return dict(count=self.counts(), S=S, n_eff=n_eff, mean=mean, sd=sd, covariance=cov, total=[int(v) for v in total.tolist()],
                    w_max=w_max)

    def order_statistics(self, targets):
        """Weighted order statistics of every (set, column), found where the rows are (vmx_sample_store_order_stats;
        :func:`vega_amd.weighted.weighted_order_statistics` is the same bits): [E, n, R] for ``targets`` [E, R] (or [R], the same for
        every set) of whole numbers in [1, M_e], 1 .. 16 per set in any order, repeats allowed."""
        given = list(targets)
        rows = [list(r) for r in given] if given and np.ndim(given[0]) else [given] * self.E
        if len(rows) != self.E or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError(f'targets [{self.E}, R] or [R]')
        if any(int(t) < 0 or int(t) >= 2**64 for r in rows for t in r):
            raise ValueError('targets: whole numbers in [1, M]')
        t = np.array([[int(v) for v in r] for r in rows], dtype=np.uint64).reshape(self.E, -1)
        values = np.empty((self.E, self.n, max(t.shape[1], 1)))
        self.engine._check(self.engine.lib.vmx_sample_store_order_stats(
            self._handle(), t.shape[1], t.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(values)))
        return values

    def weighted_quantiles(self, q, total=None):
        """The inverted-CDF quantiles ``q`` (1 .. 16 values in [0, 1]) of every (set, column), [E, n, Q]: the order statistics at
        ``max(1, ceil(q M_e))``, the targets computed exactly on the host (:func:`vega_amd.weighted.weighted_targets`).  ``total``:
        the M of every set when a summary has handed them out already."""
        from .weighted import weighted_targets
        from .ensemble import check_quantiles
        q = check_quantiles(q)
        total = self.summary()['total'] if total is None else total
        return self.order_statistics([weighted_targets(q, M) if M > 0 else [1] * q.size for M in total])

    def best(self, position=True):
        """The row of the largest lnL of every set (vmx_sample_store_best; :func:`vega_amd.weighted.weighted_best`):
        ``dict(lnl_max [E], index [E], best [E, n])``; without ``position`` no ``best``."""
        top, index = np.empty(self.E), np.zeros(self.E, dtype=np.int64)
        at = np.empty((self.E, self.n)) if position else None
        self.engine._check(self.engine.lib.vmx_sample_store_best(
            self._handle(), _dp(top), index.ctypes.data_as(C.POINTER(C.c_int64)), None if at is None else _dp(at)))
        out = dict(lnl_max=top, index=index)
        if position:
            out['best'] = at
        return out

    def close(self):
        if self._h and self.engine._h:
            self.engine.lib.vmx_sample_store_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One vegamx engine handle on one GPU, built from a Problem."""

    def __init__(self, problem, max_batch=256, device=0, extra_names=(), metal_plan=None, kron_metals=True,
                 csr_threshold=None, static_poly=True, global_chi2_matrix=None):
        self.lib = load_library()
        self.prob = problem
        # engine_group: this engine's diagonal block of the global inverse covariance of a problem split over several engines
        self.global_chi2_matrix = None if global_chi2_matrix is None else _f64(global_chi2_matrix)
        # False: polynomial pipelines keep their per-walker P(k) -> xi path instead of the static spline-coefficient basis of
        # the template's spectra (include/vegamx.h: vmx_set_static_poly) - what direct_pk needs when metal terms are part of it
        self.static_poly = bool(static_poly)
        # fast_metals (see fast_metal_plan): per item, per metal pair ('pipeline', None) | ('share', leader index)
        # | ('static', xi vector) | ('basis', [3, n_model] Kaiser basis)
        self.metal_plan = metal_plan or {}
        self.kron_metals = bool(kron_metals)   # False: Kronecker-form metal matrices are uploaded dense (diagnosis)
        # a scipy.sparse distortion matrix stays in CSR form on the device when its density is below this fraction
        # (12 bytes per non-zero against 8 per entry, and the dense MFMA product wins for large batches well before that)
        self.csr_threshold = float(os.environ.get('VEGAMX_CSR_THRESHOLD', 0.3)) if csr_threshold is None else float(csr_threshold)
        self.csr_items = []
        self.metal_source = {}          # (item name, pair index) -> (global metal index, pipeline id, has matrix)
        self.low = Lowering(problem, extra_names)
        self.pipe_descs = {}            # pipeline id -> its PipeDesc as handed to vmx_add_pipeline (the bins taps below)
        # item name -> what vmx_item_set_additive_template / vmx_item_add_broadband were handed: {'template': (vector, slot,
        # default) or None, 'broadband': [(position, function, slots, basis)]}
        self.item_extras = {}
        self.names = self.low.names
        self.n_params = len(self.names)
        self.max_batch = int(max_batch)
        self._small_io = None
        self.lanes = 1
        self.nl_hint = 0                # (the level of set_constant_nl_hint, 0 until it is called)
        self._h = C.c_void_p()
        self._attached = None           # the chain store the ensemble runs append to (attach_chain_store)
        self._gk = {}
        self.device = int(device)
        self._check(self.lib.vmx_create(C.byref(self._h), int(device)))
        try:
            self._build()
        except Exception:
            self.close()
            raise

    # ---- helpers
    def _check(self, rc):
        if rc < 0:
            raise EngineError(self.lib.vmx_last_error().decode())
        return rc

    def _gk_table(self, bs_rp, bs_rt, mock_rp=0.0, mock_rt=0.0):
        key = (bs_rp, bs_rt, mock_rp, mock_rt)
        if key not in self._gk:
            self._gk[key] = self._check(self.lib.vmx_add_gk_table_mock(self._h, bs_rp, bs_rt, mock_rp, mock_rt))
        return self._gk[key]

    def _set_shotnoise_table(self):
        if getattr(self, '_shotnoise_set', False):
            return
        tau, a = static_terms.shotnoise_a()
        a = _f64(a)
        self._check(self.lib.vmx_set_shotnoise_table(self._h, _dp(a), a.size, float(tau[0]), float(tau[1] - tau[0])))
        self._shotnoise_set = True

    def _set_fvoigt(self, table):
        key = hash(np.ascontiguousarray(table).tobytes())
        if getattr(self, '_fvoigt_key', None) == key:
            return
        if getattr(self, '_fvoigt_key', None) is not None:
            raise NotImplementedError('all correlations must share one fvoigt table')
        x, f = _f64(table[:, 0]), _f64(table[:, 1])
        self._check(self.lib.vmx_set_fvoigt_table(self._h, _dp(x), _dp(f), x.size))
        self._fvoigt_key = key

    def close(self):
        if self._h:
            self.lib.vmx_destroy(self._h)       # (its chain stores go with it)
            self._h = C.c_void_p()
            self._attached = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- construction
    def _add_pipeline(self, desc, pipe, pk_lin=None):
        n = pipe.r.size
        pid = self._check(self.lib.vmx_add_pipeline(
            self._h, C.byref(desc), n, _dp(_f64(pipe.r)), _dp(_f64(pipe.mu)), _dp(_f64(pipe.z)),
            _dp(_f64(pipe.rel_z_evol)), _dp(_f64(pipe.xi_growth))))
        self.n_pipelines = pid + 1
        self.pipe_descs[pid] = desc
        if getattr(pipe, 'rel_z_evol_1', None) is not None:
            # new-bias-evolution: each tracer of a cross-correlation evolves with its own redshift
            self._check(self.lib.vmx_pipeline_set_tracer_evolution(
                self._h, pid, _dp(_f64(pipe.rel_z_evol_1)), _dp(_f64(pipe.rel_z_evol_2)), n))
        if pipe.xi.relativistic or pipe.xi.asymmetry:
            # static splines of the odd-multipole terms of this component's linear spectrum
            low, k = self.low, self.prob.k
            rows = [fftlog_op.hamilton_spline(k, pk_lin, ell, kind)
                    for kind, ell in (('rel', 1), ('rel', 3), ('asy', 0), ('asy', 2))]
            coef = _f64(np.stack([r[0] for r in rows]))
            slots = np.array([low.need(n_) if use else -1 for n_, use in (
                ('Arel1', pipe.xi.relativistic), ('Arel3', pipe.xi.relativistic), ('Aasy0', pipe.xi.asymmetry),
                ('Aasy2', pipe.xi.asymmetry), ('Aasy3', pipe.xi.asymmetry))], dtype=np.int32)
            self._check(self.lib.vmx_pipeline_set_odd_terms(self._h, pid, _dp(coef), coef.shape[1], rows[0][1],
                                                            rows[0][2], int(pipe.xi.relativistic),
                                                            int(pipe.xi.asymmetry), _ip(slots)))
            # ... and as operators of the spectrum, for `direct_pk` (the caller's spectrum is the terms' pk_lin then)
            ops = _f64(np.stack([fftlog_op.hamilton_spline_operator(k, ell, kind)
                                 for kind, ell in (('rel', 1), ('rel', 3), ('asy', 0), ('asy', 2))]))
            self._check(self.lib.vmx_pipeline_set_odd_operator(self._h, pid, _dp(ops), ops.shape[1], ops.shape[2]))
        return pid

    def _build(self):
        prob, low, lib = self.prob, self.low, self.lib
        k = _f64(prob.k)
        pk_peak = _f64(prob.pk_full - prob.pk_smooth)       # reference model.py:177
        delta2 = _f64(k**3 * prob.pk_fid / (2 * np.pi**2))  # reference power_spectrum.py:462
        n_mu = {it.core.pk.n_mu for it in prob.items.values()}
        for it in prob.items.values():
            n_mu |= {m.pipeline.pk.n_mu for m in it.metals}
        if len(n_mu) != 1:
            raise NotImplementedError('one engine holds one mu grid: correlations with different num_bins_muk go through engine_group.make_engine')
        pipes = [p for it in prob.items.values() for p in [it.core] + [m.pipeline for m in it.metals]]
        old = {p.xi.old_fftlog for p in pipes}
        if len(old) != 1:
            raise NotImplementedError('one engine holds one transform: correlations with different old_fftlog go through engine_group.make_engine')
        self.old_fftlog = old.pop()
        lowring = {p.xi.fht_lowring for p in pipes}
        extrap = {bool(getattr(p.xi, 'fht_extrap', False)) and not self.old_fftlog for p in pipes}
        if len(lowring) != 1 or len(extrap) != 1:
            raise NotImplementedError('one engine holds one operator set: correlations with different fht_lowring / fht_extrap go through engine_group.make_engine')
        lowring, self.fht_extrap = lowring.pop(), extrap.pop()
        self.fftlog_pads = (0, 0)
        if self.fht_extrap:
            # `fht_extrap = True` (reference pktoxi.py:41,141): the FFTLog's power-law pads ride behind the samples of every
            # P_ell row and the operators carry their columns (fftlog_op.xi_operator(extrap=True))
            n_pad = 2 ** int(np.ceil(np.log2(2 * k.size))) - k.size
            self.fftlog_pads = (n_pad // 2, n_pad - n_pad // 2)
            self._check(lib.vmx_set_fftlog_padding(self._h, *self.fftlog_pads))
        self._check(lib.vmx_set_template(self._h, k.size, _dp(k), _dp(pk_peak), _dp(_f64(prob.pk_smooth)),
                                         _dp(_f64(prob.pk_full)), _dp(delta2), n_mu.pop()))
        if self.old_fftlog:
            self._check(lib.vmx_set_spline_extrapolation(self._h, 1))
        for i, ell in enumerate((0, 2, 4, 6)):
            op, x0, h, n_knots = fftlog_op.hamilton_xi_operator(k, ell) if self.old_fftlog else \
                fftlog_op.xi_operator(k, ell, lowring=lowring, extrap=self.fht_extrap)
            op = _f64(op)
            self._check(lib.vmx_set_fftlog(self._h, i, _dp(op), op.shape[0], x0, h, n_knots))

        self.item_names = list(prob.items)
        self.model_slices = {}
        n_metals_total = 0
        off = 0
        self.pipe_index = {}
        for qi, (name, item) in enumerate(prob.items.items()):
            peak = self._add_pipeline(low.pipeline(self, item.core, 'peak'), item.core, pk_peak)
            smooth = self._add_pipeline(low.pipeline(self, item.core, 'smooth'), item.core, prob.pk_smooth)
            self.pipe_index[(name, 'peak')] = peak
            self.pipe_index[(name, 'smooth')] = smooth
            idesc = ItemDesc(item.model_grid.size, item.dist_grid.size, peak, smooth, low.need('bao_amp'))
            iid = self._check(lib.vmx_add_item(self._h, C.byref(idesc)))
            assert iid == qi

            if item.metals:
                opts = item.metal_opts
                main = (item.tracer1.name, item.tracer2.name)
                override = prob.growth_rate if (opts['fast_metals'] and 'growth_rate' in low.slot
                                                and prob.growth_rate is not None) else None
                beta_subst = {}
                plan = self.metal_plan.get(name)
                # `no-metal-decomp = False` (reference model.py:120-123, :181-186): the metal terms are computed per
                # component - on the smooth spectrum, and on the peak spectrum (with the peak's non-linear broadening)
                # times bao_amp - instead of once on the full spectrum: every pair enters twice
                if opts['no_metal_decomp']:
                    components = [('full', prob.pk_full, -1)]
                else:
                    if opts['fast_metals'] or any(kind != 'pipeline' for kind, _ in plan or ()):
                        raise NotImplementedError('no-metal-decomp = False with fast_metals is not accelerated (the '
                                                  "reference's metal caches then ignore the component)")
                    components = [('smooth', prob.pk_smooth, -1), ('peak', pk_peak, low.need('bao_amp'))]
                pair_pid = {}
                entry = 0
                for mi, pair in enumerate(item.metals):
                    n1, n2 = pair.names
                    if opts['single_metal_beta']:
                        # the substitution accumulates over the loop (reference metals.py:289-293)
                        for n in (n1, n2):
                            if n not in main:
                                low.need('beta_metals')
                                beta_subst[n] = 'beta_metals'
                    betas = (beta_subst.get(n1), beta_subst.get(n2))
                    fast = bool(opts['fast_metal_bias'])
                    kind, arg = plan[mi] if plan else ('pipeline', None)
                    for component, pk_lin, amplitude_slot in components:
                        if kind == 'pipeline':
                            pid = self._add_pipeline(
                                low.pipeline(self, pair.pipeline, component, fast_metals=fast, beta_names=betas,
                                             growth_rate_override=override), pair.pipeline, pk_lin)
                            if component != 'peak':
                                self.pipe_index[(name, pair.names)] = pid
                                pair_pid[mi] = pid
                        elif kind == 'share':
                            pid = pair_pid[arg]     # the reference's per-call cache hands this pair the leader's xi
                        else:
                            pid = -1
                        md = MetalDesc()
                        md.pipeline = pid
                        md.amplitude_slot = amplitude_slot
                        # direct_pk (reference model.py:188-207, :120-123): the metal terms are part of the direct model only with
                        # `no-metal-decomp = False`, computed on the caller's spectrum - the smooth-spectrum entries here
                        md.in_direct = int(component == 'smooth')
                        md.tracer[0] = low.tracer(pair.pipeline.tracer1, beta_name=betas[0])
                        md.tracer[1] = low.tracer(pair.pipeline.tracer2, beta_name=betas[1])
                        md.same_tracer = int(n1 == n2)
                        if override is not None:
                            md.growth_rate_slot, md.growth_rate_default = -1, override
                        else:
                            md.growth_rate_slot, md.growth_rate_default = low.s('growth_rate'), DEFAULT_GROWTH_RATE
                        md.extra_bias_slot = -1
                        if (not pair.cross_with_main) and opts['separate_metal_auto_biases'] and n1 != n2:
                            found = [c for c in pair.auto_bias_names if c in low.slot]
                            if not found:
                                raise ValueError(f'Separate metal auto biases is on, but no {pair.auto_bias_names[0]} '
                                                 f'or {pair.auto_bias_names[1]} parameter found for {pair.names}.')
                            md.extra_bias_slot = low.slot[found[0]]
                        md.apply_bias = int(fast)
                        md.multiplicity = 2.0 if pair.double_count else 1.0
                        self._check(lib.vmx_item_add_metal(self._h, iid, C.byref(md)))
                        if component != 'peak':
                            self.metal_source[(name, mi)] = (n_metals_total, pid, pair.matrix is not None)
                        n_metals_total += 1
                        if kind == 'static':
                            vec = _f64(arg)
                            self._check(lib.vmx_item_set_metal_static(self._h, iid, entry, _dp(vec), vec.size))
                        elif kind == 'basis':
                            basis = _f64(arg)
                            assert basis.shape == (3, item.model_grid.size)
                            self._check(lib.vmx_item_set_metal_basis(self._h, iid, entry, _dp(basis), basis.shape[1]))
                        elif getattr(pair, 'kron', None) is not None and self.kron_metals:
                            # new_metals matrices are Kronecker products: two small products per walker instead of one
                            # [n_model]^2 product
                            a_rp = _f64(pair.kron[0])
                            b_rt = None if pair.kron[1] is None else _f64(pair.kron[1])
                            n_rt = item.model_grid.size // a_rp.shape[0]
                            self._check(lib.vmx_item_set_metal_kron(self._h, iid, entry, _dp(a_rp), a_rp.shape[0],
                                                                    None if b_rt is None else _dp(b_rt), n_rt))
                        elif pair.matrix is not None:
                            dense = _f64(pair.matrix.toarray() if hasattr(pair.matrix, 'toarray') else pair.matrix)
                            self._check(lib.vmx_item_set_matrix(self._h, iid, MAT_METAL, entry, dense.shape[0],
                                                                dense.shape[1], _dp(dense)))
                        entry += 1

            extras = self.item_extras[name] = {'template': None, 'broadband': []}
            if item.inst_sys_table is not None:
                vec = _f64(static_terms.instrumental_systematics_template(item))
                extras['template'] = (vec, low.s('desi_inst_sys_amp'), static_terms.DESI_INST_SYS_DEFAULT_AMP)
                self._check(lib.vmx_item_set_additive_template(self._h, iid, _dp(vec), vec.size,
                                                               low.s('desi_inst_sys_amp'),
                                                               static_terms.DESI_INST_SYS_DEFAULT_AMP))
            for term in item.broadband:
                grid = item.model_grid if term.pos == 'pre' else item.dist_grid
                pos = BB_POS[(term.pos, term.kind)]
                if term.func == 'broadband_sky':
                    slots = np.array([low.need(term.name + '-scale-sky'), low.need(term.name + '-sigma-sky')],
                                     dtype=np.int32)
                    window = ((grid.rp >= 0.) & (grid.rp < grid.rp_binsize)).astype(np.float64)
                    basis = _f64(np.stack([grid.rt, window]))
                    func = BB_SKY
                else:
                    if term.coords == 'r,mu':
                        r1, r2 = grid.r / 100., grid.mu
                    else:
                        r1 = grid.r / 100. * grid.mu
                        r2 = grid.r / 100. * np.sqrt(1 - grid.mu**2)
                    p1 = np.arange(term.r1[0], term.r1[1] + 1, term.r1[2])
                    p2 = np.arange(term.r2[0], term.r2[1] + 1, term.r2[2])
                    slots, rows = [], []
                    for i in p1:
                        for j in p2:
                            slots.append(low.need(f'{term.name} ({i},{j})'))
                            rows.append(r1**i * r2**j)
                    slots = np.array(slots, dtype=np.int32)
                    basis = _f64(np.stack(rows))
                    func = BB_POLY
                if slots.size > 16:
                    raise NotImplementedError('more than 16 coefficients in one broadband term')
                extras['broadband'].append((pos, func, slots, basis))
                self._check(lib.vmx_item_add_broadband(self._h, iid, pos, func, slots.size, _ip(slots),
                                                       _dp(basis), basis.shape[1]))

            if item.distortion is not None:
                dm = item.distortion
                if hasattr(dm, 'tocsr') and dm.nnz < self.csr_threshold * dm.shape[0] * dm.shape[1]:
                    # the reference's own representation (scipy csr_array, vega/data.py:342-346), kept as is
                    csr = dm.tocsr().copy()
                    csr.sum_duplicates()        # canonical form: sorted, one entry per (row, column)
                    csr.sort_indices()
                    ptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
                    idx = np.ascontiguousarray(csr.indices, dtype=np.int32)
                    val = _f64(csr.data)
                    self._check(lib.vmx_item_set_matrix_csr(self._h, iid, csr.shape[0], csr.shape[1],
                                                            ptr.ctypes.data_as(C.POINTER(C.c_int64)), _ip(idx), _dp(val)))
                    self.csr_items.append(name)
                else:
                    dense = _f64(dm.toarray() if hasattr(dm, 'toarray') else dm)
                    self._check(lib.vmx_item_set_matrix(self._h, iid, MAT_DISTORTION, 0, dense.shape[0],
                                                        dense.shape[1], _dp(dense)))
            idx = np.flatnonzero(item.model_mask).astype(np.int32)
            if idx.size != item.data_size:
                raise ValueError(f'{name}: model mask keeps {idx.size} bins but the data mask {item.data_size}')
            self._check(lib.vmx_item_set_mask(self._h, iid, _ip(idx), idx.size))
            self._check(lib.vmx_item_set_data(self._h, iid, _dp(_f64(item.masked_data_vec)), idx.size))
            if getattr(item, 'marg_diff2coeff', None) is not None:
                # best-fit template coefficients = M . residual (reference vega_interface.py:546-579)
                m = _f64(item.marg_diff2coeff)
                self._check(lib.vmx_item_set_marg_matrix(self._h, iid, _dp(m), m.shape[0], m.shape[1]))
            if item.cov is not None and prob.global_cov is None and self.global_chi2_matrix is None:
                cinv = _f64(item.chi2_matrix)      # C^-1, or P^T C^-1 P with marginalize-in-fit (setup.py)
                self._check(lib.vmx_item_set_matrix(self._h, iid, MAT_INVCOV, 0, cinv.shape[0], cinv.shape[1],
                                                    _dp(cinv)))
            self.model_slices[name] = slice(off, off + item.dist_grid.size)
            off += item.dist_grid.size

        if prob.global_cov is not None or self.global_chi2_matrix is not None:
            g = self.global_chi2_matrix if self.global_chi2_matrix is not None else _f64(prob.global_masks()['chi2_matrix'])
            self._check(lib.vmx_set_global_invcov(self._h, _dp(g), g.shape[0]))
        for pname, (mean, sigma) in prob.priors.items():
            self._check(lib.vmx_add_prior(self._h, low.need(pname), float(mean), float(sigma)))
        # applicability guard of the mu node rule: the box it is validated on (mu_quadrature.rule_box)
        from .mu_quadrature import rule_box
        box = rule_box(low.names)
        if box:
            slots = np.array([low.slot[n] for n in box], dtype=np.int32)
            lo = _f64([box[n][0] for n in box])
            hi = _f64([box[n][1] for n in box])
            self._check(lib.vmx_set_mu_rule_box(self._h, slots.size, _ip(slots), _dp(lo), _dp(hi)))
        self.mu_rule_box = box
        if not self.static_poly:
            self._check(lib.vmx_set_static_poly(self._h, 0))
        self._check(lib.vmx_finalize(self._h, self.n_params, self.max_batch))
        self.model_size = self._check(lib.vmx_model_size(self._h))
        # chi2-only evaluations run as a static quadratic form around the configured parameter values when the
        # configuration allows it (include/vegamx.h: vmx_set_quadratic_form)
        self.quadratic_form = bool(self._check(lib.vmx_set_quadratic_form(self._h, _dp(_f64(low.theta0)))))

    # ---- evaluation
    def theta_from_params(self, params=None):
        theta = self.low.theta0.copy()
        if params:
            for name, value in params.items():
                if name == 'peak':
                    continue
                if name not in self.low.slot:
                    raise KeyError(f'unknown parameter {name!r}: rebuild the engine with extra_names')
                theta[self.low.slot[name]] = value
        return theta

    def eval(self, theta, want_model=False):
        """theta [B, n_params] -> (chi2 [B], status [B], model [B, model_size] or None)."""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim == 1:
            theta = theta[None, :]
        B = theta.shape[0]
        if theta.shape[1] != self.n_params:
            raise ValueError(f'theta must have {self.n_params} columns')
        if not want_model and B <= 8:
            # small chi2-only calls are latency-bound: persistent in / out buffers with their pointers made once (building
            # three ctypes pointers costs as much as two of the chain's kernels)
            io = self._small_io
            if io is None:
                t_in, c_out, s_out = np.empty((8, self.n_params)), np.empty(8), np.empty(8, dtype=np.int32)
                io = self._small_io = (t_in, c_out, s_out, _dp(t_in), _dp(c_out), _ip(s_out))
            io[0][:B] = theta
            if self.lib.vmx_eval(self._h, io[3], B, io[4], None, io[5]) < 0:
                raise EngineError(self.lib.vmx_last_error().decode())
            return io[1][:B].copy(), io[2][:B].copy(), None
        theta = _f64(theta)
        chi2 = np.empty(B)
        status = np.empty(B, dtype=np.int32)
        model = np.empty((B, self.model_size)) if want_model else None
        self._check(self.lib.vmx_eval(self._h, _dp(theta), B, _dp(chi2), _dp(model) if want_model else None,
                                      _ip(status)))
        return chi2, status, model

    def eval_device(self, d_theta_ptr, B, d_chi2_ptr, d_model_ptr=None, d_status_ptr=None):
        self._check(self.lib.vmx_eval_device(self._h, d_theta_ptr, B, d_chi2_ptr, d_model_ptr, d_status_ptr))

    def sync(self):
        self._check(self.lib.vmx_sync(self._h))

    def eval_device_mocks(self, d_theta_ptr, B, d_chi2_ptr, d_mock_ptr, d_status_ptr=None):
        """``eval_device`` for walkers that bring their own mock rows: ``d_mock_ptr`` int32 [B] in device memory, per walker the
        pool row it is compared with (include/vegamx.h: vmx_eval_device_mocks)."""
        self._check(self.lib.vmx_eval_device_mocks(self._h, d_theta_ptr, B, d_chi2_ptr, d_status_ptr, d_mock_ptr))

    def set_mock_factor(self, name, chol, fiducial_masked):
        """Cholesky factor of item ``name``'s (scaled) masked covariance and its fiducial model on the masked bins: the mocks of a
        ``fit_migrad(..., mock_stream=...)`` run are made from them on the device (include/vegamx.h: vmx_item_set_mock_factor)."""
        qi = self.item_names.index(name)
        chol, fid = _f64(chol), _f64(fiducial_masked)
        self._check(self.lib.vmx_item_set_mock_factor(self._h, qi, _dp(chol), _dp(fid), fid.size))

    def pinned_empty(self, shape):
        """A float64 array of ``shape`` in page-locked host memory (include/vegamx.h: vmx_host_alloc) - for buffers the library
        copies from asynchronously.  Kept per engine and reused while it is large enough; the memory lives until `close()`, so the
        array must not be used after that."""
        count = int(np.prod(shape))
        kept = self.__dict__.get('_pinned')
        if kept is None or kept[1] < count:
            if kept is not None:
                self._check(self.lib.vmx_host_free(self._h, kept[0]))
                self._pinned = None
            ptr = C.c_void_p()
            self._check(self.lib.vmx_host_alloc(self._h, C.byref(ptr), count * 8))
            self._pinned = kept = (ptr, count)
        flat = np.ctypeslib.as_array(C.cast(kept[0], C.POINTER(C.c_double)), shape=(kept[1],))
        return flat[:count].reshape(shape)

    def get_mock_pool(self, name, n_mocks):
        """The first ``n_mocks`` rows of item ``name``'s mock pool, as the device holds them."""
        qi = self.item_names.index(name)
        n = self.prob.items[name].data_size
        out = np.empty((n_mocks, n))
        self._check(self.lib.vmx_item_get_mock_pool(self._h, qi, _dp(out), n_mocks, n))
        return out

    def fit_migrad(self, plan, theta0, mock_rows=None, const_hint=-1, chunk=0, lanes=0, mock_stream=None):
        """MIGRAD fits of ``theta0.shape[0]`` parameter rows on the device (include/vegamx.h: vmx_fit_migrad).  ``plan``:
        :meth:`vega_amd.migrad.MigradMinimizer.plan` with ``free`` = indices into the engine's parameter columns; ``mock_rows``:
        the pool row every fit is fitted to (None: the items' data).  Returns (per-stage result dicts, statistics of the run)."""
        stages = plan['stages']
        if not 1 <= len(stages) <= VMX_FIT_MAX_STAGES:
            raise ValueError(f'1 .. {VMX_FIT_MAX_STAGES} Minuit objects per fit')
        theta0 = _f64(theta0)
        F = theta0.shape[0]
        if theta0.ndim != 2 or theta0.shape[1] != self.n_params:
            raise ValueError(f'theta0 must have {self.n_params} columns')
        spec = FitSpec()
        spec.n_stages, spec.n_params = len(stages), self.n_params
        spec.iterate, spec.maxfcn, spec.up, spec.tol = int(plan['iterate']), int(plan['maxfcn']), float(plan['up']), float(plan['tol'])
        for k, st in enumerate(stages):
            free = np.asarray(st['free'], dtype=int)
            if not 1 <= free.size <= VMX_FIT_MAXN:
                raise NotImplementedError(f'{free.size} free parameters: the device-resident fits take 1 .. {VMX_FIT_MAXN} per Minuit object')
            cs = spec.stage[k]
            cs.n = free.size
            for i, (j, lim, err) in enumerate(zip(free, st['limits'], st['errors'])):
                lo, hi = (None, None) if lim is None else lim
                lo = None if lo is None or not np.isfinite(lo) else float(lo)
                hi = None if hi is None or not np.isfinite(hi) else float(hi)
                cs.col[i], cs.has_lo[i], cs.has_hi[i] = int(j), int(lo is not None), int(hi is not None)
                cs.lo[i], cs.hi[i], cs.err[i] = lo or 0., hi or 0., float(err)
        outs, res = [], (FitResultArrays * len(stages))()
        for k, st in enumerate(stages):
            n = len(st['free'])
            o = dict(x=np.zeros((F, n)), ext=np.zeros((F, n)), V=np.zeros((F, n, n)), fval=np.zeros(F), edm=np.zeros(F),
                     flags=np.zeros(F, dtype=np.int32), nfcn=np.zeros(F, dtype=np.int64), n_iter=np.zeros(F, dtype=np.int32))
            outs.append(o)
            r = res[k]
            r.x, r.ext, r.V, r.fval, r.edm = _dp(o['x']), _dp(o['ext']), _dp(o['V']), _dp(o['fval']), _dp(o['edm'])
            r.flags, r.nfcn, r.n_iter = _ip(o['flags']), o['nfcn'].ctypes.data_as(C.POINTER(C.c_int64)), _ip(o['n_iter'])
        rows = None if mock_rows is None else np.ascontiguousarray(mock_rows, dtype=np.int32)
        if rows is not None and rows.shape != (F,):
            raise ValueError('mock_rows: one pool row per fit')
        opt = FitOptions(int(const_hint), int(chunk), int(lanes), 0, None)
        if mock_stream is not None:
            # the mocks are made while the fits run: `draws` [F, stride] float64 filled by a producer thread, `counter` int32 [1]
            # counting the complete rows (include/vegamx.h: vmx_mock_stream)
            draws, counter = mock_stream['draws'], mock_stream['counter']
            if draws.dtype != np.float64 or not draws.flags.c_contiguous or draws.shape[0] != F or counter.dtype != np.int32:
                raise ValueError('mock_stream: draws float64 [n_fits, stride] C-contiguous, counter int32')
            ms = MockStream(F, int(mock_stream.get('wave', 0)), _dp(draws), draws.shape[1], _ip(counter),
                            float(mock_stream.get('timeout', 0.)))
            opt.mocks = C.pointer(ms)
        stats = FitStats()
        self._check(self.lib.vmx_fit_migrad(self._h, C.byref(spec), F, _dp(theta0), None if rows is None else _ip(rows),
                                            C.byref(opt), res, C.byref(stats)))
        info = {name: getattr(stats, name) for name, _ in FitStats._fields_ if not name.endswith('by_batch')}
        info['calls_by_batch'] = dict(zip(FIT_BATCH_BINS, list(stats.calls_by_batch)))
        info['evaluations_by_batch'] = dict(zip(FIT_BATCH_BINS, list(stats.evaluations_by_batch)))
        return outs, info

    def _sampled_box(self, cols, lo, hi, theta_fixed, **state):
        """What the three samplers' calls take alike: ``cols`` / ``lo`` / ``hi`` / ``theta_fixed`` as the library reads them, and the
        check of the run's state, given by name: points [rows, n] and their lnL [rows], float64, updated in place.  Returns the four
        arrays and rows."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        lo, hi, theta_fixed = _f64(lo), _f64(hi), _f64(theta_fixed)
        _in_place(np.float64, **state)
        (pname, points), (lname, lnl) = state.items()
        rows = points.shape[0]
        if points.shape != (rows, cols.size) or lnl.shape != (rows,) or theta_fixed.shape != (self.n_params,):
            raise ValueError(f'{pname} [rows, n], {lname} [rows], theta_fixed [n_params]')
        return cols, lo, hi, theta_fixed, rows

    def _ensemble_arrays(self, ndim, cols, lo, hi, theta_fixed, x, lnl, accepted, step0, n_steps, thin, keep_chain, *, a, log_norm,
                         seed, stream, const_hint, chunk, lanes):
        """What :meth:`ensemble_run` (``ndim`` 2: x [W, n]) and :meth:`ensemble_run_many` (3: x [E, W, n]) hand the library alike:
        the box and the state checked as :meth:`_sampled_box` checks them, the chain [(E,) rows, W, n] with its lnL (None: not
        kept), the spec, the call's arguments from ``x`` to the options, and the statistics; last, what the pointers borrow."""
        _in_place(np.float64, x=x, lnl=lnl)
        _in_place(np.int64, accepted=accepted)
        if x.ndim != ndim or lnl.shape != x.shape[:-1] or accepted.shape != x.shape[:-1]:
            raise ValueError('x [W, n], lnl [W], accepted [W]' if ndim == 2 else 'x [E, W, n], lnl [E, W], accepted [E, W]')
        cols, lo, hi, theta_fixed, _ = self._sampled_box(cols, lo, hi, theta_fixed, x=x.reshape(-1, x.shape[-1]), lnl=lnl.reshape(-1))
        step0, n_steps, thin = int(step0), int(n_steps), int(thin)
        rows = max(0, (step0 + n_steps) // thin - step0 // thin) if thin >= 1 else 0
        chain = np.empty(x.shape[:-2] + (rows,) + x.shape[-2:]) if keep_chain else None
        chain_lnl = np.empty(x.shape[:-2] + (rows, x.shape[-2])) if keep_chain else None
        spec = EnsembleSpec(self.n_params, cols.size, _ip(cols), _dp(lo), _dp(hi), float(a), float(log_norm), int(seed), int(stream),
                            _dp(theta_fixed))
        opt = EnsembleOptions(int(const_hint), int(chunk), int(lanes), 0)
        args = (_dp(x), _dp(lnl), accepted.ctypes.data_as(C.POINTER(C.c_int64)), step0, n_steps, thin,
                _dp(chain) if keep_chain else None, _dp(chain_lnl) if keep_chain else None, C.byref(opt))
        return spec, args, chain, chain_lnl, EnsembleStats(), (cols, lo, hi, theta_fixed, opt)

    def _ensemble_ladders(self, own, cols, lo, hi, theta_fixed, x, lnl, accepted, betas, streams, mock_rows, moves, step0, n_steps,
                          thin, keep_chain, **spec_kw):
        """What :meth:`ensemble_run_pt` (``own`` False: betas [T]) and :meth:`ensemble_run_pt_adapt` (True: betas [G, T], updated
        in place) hand the library alike: x [G, T, W, n] checked and passed on to :meth:`_ensemble_arrays` as G T ensembles, the
        ladder, streams and mocks checked.  Returns (G, T), the call's arguments before and after ``swap_every``, the chain
        [G, T, rows, W, n] with its lnL (None: not kept), the statistics with ``per_ensemble`` [G, T, 3] and ``swaps``
        [G, T - 1, 2]; last, what the pointers borrow."""
        _in_place(np.float64, x=x, lnl=lnl, **({'betas': betas} if own else {}))
        _in_place(np.int64, accepted=accepted)
        if x.ndim != 4:
            raise ValueError('x [G, T, W, n], lnl [G, T, W], accepted [G, T, W]')
        G, T, W, n = x.shape
        spec, args, chain, chain_lnl, stats, held = self._ensemble_arrays(
            3, cols, lo, hi, theta_fixed, x.reshape(G * T, W, n), lnl.reshape(G * T, W), accepted.reshape(G * T, W), step0, n_steps,
            thin, keep_chain, **spec_kw)
        if not own:
            betas = np.ascontiguousarray(betas, dtype=np.float64)
        streams = np.ascontiguousarray(streams, dtype=np.uint64)
        if mock_rows is not None:
            mock_rows = np.ascontiguousarray(mock_rows, dtype=np.int32)
        if betas.shape != ((G, T) if own else (T,)) or streams.shape != (G, T) or (mock_rows is not None and mock_rows.shape != (G,)):
            raise ValueError(f"betas [{'G, T' if own else 'T'}], streams [G, T], mock_rows [G]")
        per = np.zeros((G, T, 3), dtype=np.int64)
        swaps = np.zeros((G, max(T - 1, 0), 2), dtype=np.int64)
        if _ensemble_cov(moves) is not None:
            raise ValueError("moves: 'cov' does not run on a temperature ladder")
        mv = _ensemble_moves(moves)
        i64 = C.POINTER(C.c_int64)
        head = (self._h, C.byref(spec), G, T, W, _dp(betas), streams.ctypes.data_as(C.POINTER(C.c_uint64)),
                None if mock_rows is None else _ip(mock_rows), *args[:6])
        tail = (*args[6:], C.byref(stats), per.ctypes.data_as(i64), None if mv is None else C.byref(mv), swaps.ctypes.data_as(i64))
        if keep_chain:      # (views of what the library fills)
            chain, chain_lnl = chain.reshape((G, T) + chain.shape[1:]), chain_lnl.reshape((G, T) + chain_lnl.shape[1:])
        return (G, T), head, tail, chain, chain_lnl, stats, per, swaps, (held, spec, betas, streams, mock_rows, mv)

    def ensemble_run(self, cols, lo, hi, theta_fixed, x, lnl, accepted, step0, n_steps, thin=1, a=2.0, log_norm=0.0, seed=0,
                     stream=0, const_hint=-1, chunk=0, lanes=0, keep_chain=True, moves=None):
        """``n_steps`` steps of the ensemble sampler on the device (include/vegamx.h: vmx_ensemble_run): ``cols`` the sampled
        parameter columns with their box [lo, hi], ``theta_fixed`` the row of the others, ``x`` [W, n] / ``lnl`` [W] / ``accepted``
        int64 [W] the walkers' state (updated in place), ``step0`` the global index of the first step.  Returns (chain [rows, W, n],
        chain_lnl [rows, W], statistics), rows = (step0 + n_steps) // thin - step0 // thin.  ``moves`` (None: the stretch move
        through vmx_ensemble_run): the mixture of :meth:`ensemble_run_many`, run as the set of one."""
        if moves is not None:
            _in_place(np.float64, x=x, lnl=lnl)
            _in_place(np.int64, accepted=accepted)
            if x.ndim != 2:
                raise ValueError('x [W, n], lnl [W], accepted [W]')
            chain, chain_lnl, st = self.ensemble_run_many(
                cols, lo, hi, theta_fixed, x[None], lnl[None], accepted[None], [stream], step0, n_steps, thin=thin, a=a,
                log_norm=log_norm, seed=seed, const_hint=const_hint, chunk=chunk, lanes=lanes, keep_chain=keep_chain, moves=moves)
            st.pop('per_ensemble')
            return (chain[0], chain_lnl[0], st) if keep_chain else (None, None, st)
        spec, args, chain, chain_lnl, stats, _held = self._ensemble_arrays(
            2, cols, lo, hi, theta_fixed, x, lnl, accepted, step0, n_steps, thin, keep_chain, a=a, log_norm=log_norm, seed=seed,
            stream=stream, const_hint=const_hint, chunk=chunk, lanes=lanes)
        self._check(self.lib.vmx_ensemble_run(self._h, C.byref(spec), x.shape[0], *args, C.byref(stats)))
        return chain, chain_lnl, _stats_dict(stats)

    def ensemble_run_many(self, cols, lo, hi, theta_fixed, x, lnl, accepted, streams, step0, n_steps, mock_rows=None, thin=1, a=2.0,
                          log_norm=0.0, seed=0, const_hint=-1, chunk=0, lanes=0, keep_chain=True, moves=None):
        """``n_steps`` steps of E independent ensembles in one device run (include/vegamx.h: vmx_ensemble_run_many): ``x`` [E, W, n]
        / ``lnl`` [E, W] / ``accepted`` int64 [E, W] the walkers' state (updated in place), ``streams`` [E] the Philox stream of every
        ensemble, ``mock_rows`` [E] the pool row every ensemble is compared with (None: the installed data); the rest as for
        :meth:`ensemble_run`.  Returns (chain [E, rows, W, n], chain_lnl [E, rows, W], statistics); the statistics carry
        ``per_ensemble`` int64 [E, 3]: accepted, rejected outside the box, rejected for a failed model.  ``moves`` (None:
        vmx_ensemble_run_many, the stretch move): a mapping with ``weights`` (stretch, DE, snooker), ``gamma0``, ``sigma``,
        ``gamma_s`` and optionally ``flags`` - the mixture of vmx_ensemble_run_many_moves
        (:func:`vega_amd.ensemble.resolve_moves` makes one).  With a fourth weight - the covariance move - and ``cov_scale`` the run
        is vmx_ensemble_run_many_cov, and the statistics carry ``cov_fallbacks`` int64 [E]: the half-steps whose factor fell back
        to the diagonal."""
        spec, args, chain, chain_lnl, stats, _held = self._ensemble_arrays(
            3, cols, lo, hi, theta_fixed, x, lnl, accepted, step0, n_steps, thin, keep_chain, a=a, log_norm=log_norm, seed=seed,
            stream=0, const_hint=const_hint, chunk=chunk, lanes=lanes)
        E, W = x.shape[:2]
        if streams is not None:
            streams = np.ascontiguousarray(streams, dtype=np.uint64)
        if mock_rows is not None:
            mock_rows = np.ascontiguousarray(mock_rows, dtype=np.int32)
        if (streams is not None and streams.shape != (E,)) or (mock_rows is not None and mock_rows.shape != (E,)):
            raise ValueError('streams [E], mock_rows [E]')
        per = np.zeros((E, 3), dtype=np.int64)
        head = (self._h, C.byref(spec), E, W, None if streams is None else streams.ctypes.data_as(C.POINTER(C.c_uint64)),
                None if mock_rows is None else _ip(mock_rows), *args, C.byref(stats), per.ctypes.data_as(C.POINTER(C.c_int64)))
        if moves is None:
            self._check(self.lib.vmx_ensemble_run_many(*head))
        else:
            mv, cv = _ensemble_moves(moves), _ensemble_cov(moves)
            if cv is None:
                self._check(self.lib.vmx_ensemble_run_many_moves(*head, C.byref(mv)))
            else:
                fallbacks = np.zeros(E, dtype=np.int64)
                self._check(self.lib.vmx_ensemble_run_many_cov(*head, C.byref(mv), C.byref(cv), fallbacks.ctypes.data_as(C.POINTER(C.c_int64))))
                return chain, chain_lnl, dict(_stats_dict(stats), per_ensemble=per, cov_fallbacks=fallbacks)
        return chain, chain_lnl, dict(_stats_dict(stats), per_ensemble=per)

    def chain_store(self, E, W, n, capacity):
        """A :class:`ChainStore` on this engine's device: ``capacity`` rows of E ensembles of W walkers over n columns."""
        return ChainStore(self, E, W, n, capacity)

    def sample_store(self, E, n, capacity):
        """A :class:`SampleStore` on this engine's device: E weighted sample sets of up to ``capacity`` rows over n columns."""
        return SampleStore(self, E, n, capacity)

    def attach_chain_store(self, store=None):
        """While ``store`` is attached, every ``ensemble_run*`` call appends the rows it records to it on the device (include/vegamx.h:
        vmx_ensemble_set_chain_store) - with ``keep_chain=False`` nothing of the chain crosses to the host.  None detaches."""
        if store is not None and store.engine is not self:
            raise ValueError('the chain store belongs to another engine')
        self._check(self.lib.vmx_ensemble_set_chain_store(self._h, None if store is None else store._handle()))
        self._attached = store

    def ensemble_cov_factor(self, x):
        """The factor stage of the covariance move alone (include/vegamx.h: vmx_ensemble_cov_factor): the halves ``x`` [E, H, n] give
        (mean [E, n], factor [E, n, n] lower, flag int32 [E]: 1 the Cholesky factor, 0 the diagonal fallback)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 3:
            raise ValueError('x [E, H, n]')
        E, H, n = x.shape
        mean, factor, flag = np.zeros((E, n)), np.zeros((E, n, n)), np.zeros(E, dtype=np.int32)
        self._check(self.lib.vmx_ensemble_cov_factor(self._h, E, H, n, _dp(x), _dp(mean), _dp(factor), _ip(flag)))
        return mean, factor, flag

    def ensemble_run_slice(self, cols, lo, hi, theta_fixed, x, lnl, accepted, streams, mu, step0, n_steps, mock_rows=None, thin=1,
                           log_norm=0.0, seed=0, const_hint=-1, chunk=0, lanes=0, keep_chain=True, mu0=1.0, tune_steps=100,
                           max_expansions=32, max_contractions=64, flags=0):
        """``n_steps`` steps of ensemble slice sampling for E independent ensembles in one device run (include/vegamx.h:
        vmx_ensemble_run_slice): the state as for :meth:`ensemble_run_many`, ``mu`` float64 [E] the scales (updated in place).
        Returns (chain [E, rows, W, n], chain_lnl [E, rows, W], statistics); the statistics carry ``slice_counts`` int64 [E, 8] in
        the order of ``SLICE_COUNT_NAMES`` and ``rounds``.  The steps with global index below ``tune_steps`` tune ``mu``."""
        spec, args, chain, chain_lnl, stats, _held = self._ensemble_arrays(
            3, cols, lo, hi, theta_fixed, x, lnl, accepted, step0, n_steps, thin, keep_chain, a=2.0, log_norm=log_norm, seed=seed,
            stream=0, const_hint=const_hint, chunk=chunk, lanes=lanes)
        _in_place(np.float64, mu=mu)
        E, W = x.shape[:2]
        if streams is not None:
            streams = np.ascontiguousarray(streams, dtype=np.uint64)
        if mock_rows is not None:
            mock_rows = np.ascontiguousarray(mock_rows, dtype=np.int32)
        if (streams is not None and streams.shape != (E,)) or (mock_rows is not None and mock_rows.shape != (E,)) or mu.shape != (E,):
            raise ValueError('streams [E], mock_rows [E], mu [E]')
        counts = np.zeros((E, VMX_SLICE_COUNTS), dtype=np.int64)
        sl = EnsembleSlice(float(mu0), int(tune_steps), int(max_expansions), int(max_contractions), int(flags))
        self._check(self.lib.vmx_ensemble_run_slice(
            self._h, C.byref(spec), E, W, None if streams is None else streams.ctypes.data_as(C.POINTER(C.c_uint64)),
            None if mock_rows is None else _ip(mock_rows), *args, C.byref(stats), C.byref(sl), _dp(mu),
            counts.ctypes.data_as(C.POINTER(C.c_int64))))
        st = _stats_dict(stats)
        return chain, chain_lnl, dict(st, slice_counts=counts, rounds=st['host_synchronisations'] - 1)

    def ensemble_run_pt(self, cols, lo, hi, theta_fixed, x, lnl, accepted, betas, streams, step0, n_steps, swap_every=1, mock_rows=None,
                        thin=1, a=2.0, log_norm=0.0, seed=0, const_hint=-1, chunk=0, lanes=0, keep_chain=True, moves=None):
        """``n_steps`` steps of G temperature ladders of T rungs in one device run (include/vegamx.h: vmx_ensemble_run_pt): ``x``
        [G, T, W, n] / ``lnl`` [G, T, W] / ``accepted`` int64 [G, T, W] the walkers' state (updated in place; lnl untempered),
        ``betas`` [T] the ladder, ``streams`` [G, T] the Philox stream of every rung, ``mock_rows`` [G] the pool row of every ladder
        (None: the installed data), ``swap_every`` the steps between swap sweeps (0: none); the rest as for
        :meth:`ensemble_run_many`.  Returns (chain [G, T, rows, W, n], chain_lnl [G, T, rows, W], statistics); the statistics
        carry ``per_ensemble`` int64 [G, T, 3] and ``swaps`` int64 [G, T - 1, 2]: proposed and accepted per pair of rungs."""
        _shape, head, tail, chain, chain_lnl, stats, per, swaps, _held = self._ensemble_ladders(
            False, cols, lo, hi, theta_fixed, x, lnl, accepted, betas, streams, mock_rows, moves, step0, n_steps, thin, keep_chain,
            a=a, log_norm=log_norm, seed=seed, stream=0, const_hint=const_hint, chunk=chunk, lanes=lanes)
        self._check(self.lib.vmx_ensemble_run_pt(*head, int(swap_every), *tail))
        return chain, chain_lnl, dict(_stats_dict(stats), per_ensemble=per, swaps=swaps)

    def ensemble_run_pt_adapt(self, cols, lo, hi, theta_fixed, x, lnl, accepted, betas, streams, step0, n_steps, swap_every=1,
                              adaptation_lag=10000.0, adaptation_time=100.0, adapt_until=-1, mock_rows=None, thin=1, a=2.0,
                              log_norm=0.0, seed=0, const_hint=-1, chunk=0, lanes=0, keep_chain=True, moves=None):
        """:meth:`ensemble_run_pt` with a ladder of its own for every one of the G ladders, moved on the device after every swap
        sweep (include/vegamx.h: vmx_ensemble_run_pt_adapt): ``betas`` float64 [G, T] (updated in place), ``adaptation_lag`` /
        ``adaptation_time`` ptemcee's, in sweeps; the sweep after global step s adapts iff ``adapt_until`` < 0 or s <
        ``adapt_until``.  The statistics carry, beside ``per_ensemble`` and ``swaps``, ``beta_hist`` [sweeps, G, T] - the ladders
        after every sweep of the call - and ``adapt_skipped`` int64 [G], the sweeps whose new ladder the guard dropped."""
        (G, T), head, tail, chain, chain_lnl, stats, per, swaps, _held = self._ensemble_ladders(
            True, cols, lo, hi, theta_fixed, x, lnl, accepted, betas, streams, mock_rows, moves, step0, n_steps, thin, keep_chain,
            a=a, log_norm=log_norm, seed=seed, stream=0, const_hint=const_hint, chunk=chunk, lanes=lanes)
        step0, n_steps, swap_every = int(step0), int(n_steps), int(swap_every)
        sweeps = max(0, (step0 + n_steps) // swap_every - step0 // swap_every) if swap_every > 0 and n_steps >= 0 and step0 >= 0 else 0
        hist = np.zeros((sweeps, G, T))
        skipped = np.zeros(G, dtype=np.int64)
        ad = EnsembleAdapt(float(adaptation_lag), float(adaptation_time), int(adapt_until), 0, 0)
        self._check(self.lib.vmx_ensemble_run_pt_adapt(*head, swap_every, *tail, C.byref(ad), _dp(hist) if sweeps else None,
                                                       skipped.ctypes.data_as(C.POINTER(C.c_int64))))
        return chain, chain_lnl, dict(_stats_dict(stats), per_ensemble=per, swaps=swaps, beta_hist=hist, adapt_skipped=skipped)

    def nested_run(self, cols, lo, hi, theta_fixed, live_u, live_lnl, iteration, n_iterations, threads, num_repeats, log_norm=0.0,
                   seed=0, stream=0, const_hint=-1, chunk=0, lanes=0, draw_live=False, stop=None, clusters=None, cluster_flags=None,
                   phantoms=None, phantom_capacity=None):
        """Up to ``n_iterations`` iterations of the nested sampler on the device (include/vegamx.h: vmx_nested_run): ``cols`` the
        sampled parameter columns with their box [lo, hi], ``theta_fixed`` the row of the others, ``live_u`` [nlive, n] in the unit
        cube / ``live_lnl`` [nlive] the run's state (updated in place; drawn first with ``draw_live``), ``iteration`` the global
        index of the next iteration.  ``stop(iterations, dead_lnl [K], live_lnl [nlive])`` is asked after every iteration; a true
        answer ends the call.  Returns (dead_u [m K, n], dead_lnl [m K], dead_nlive [m K], iteration + m, statistics) for the m
        iterations done.  ``clusters`` (a :class:`vega_amd.nested.ClusterState`, updated in place, the ids of this call's dead
        appended to its ``dead``): the run with clustering (vmx_nested_run_clustered); ``cluster_flags`` overrides the flags word
        (0: the entry runs what vmx_nested_run runs).  ``phantoms`` (a :class:`vega_amd.nested.PhantomState`: its ``fraction`` of
        the accepted points inside the walks is kept and this call's are appended to it, in the canonical order): the run
        through vmx_nested_run_phantoms, with or without ``clusters``; ``phantom_capacity`` overrides the rows of the record's
        arrays (threads (num_repeats - 1) per iteration: what the call can keep at the most)."""
        cols, lo, hi, theta_fixed, nlive = self._sampled_box(cols, lo, hi, theta_fixed, live_u=live_u, live_lnl=live_lnl)
        K, n_iterations = int(threads), max(0, int(n_iterations))
        rows = n_iterations * max(K, 0)
        dead_u, dead_lnl, dead_n = np.empty((rows, cols.size)), np.empty(rows), np.empty(rows, dtype=np.int32)
        spec = NestedSpec(self.n_params, cols.size, _ip(cols), _dp(lo), _dp(hi), nlive, K, int(num_repeats), 0, float(log_norm),
                          int(seed), int(stream), _dp(theta_fixed))
        raised = []

        def _stop(_user, iterations, p_dead, p_live):
            try:
                return 1 if stop(int(iterations), np.ctypeslib.as_array(p_dead, (K,)), np.ctypeslib.as_array(p_live, (nlive,))) else 0
            except BaseException as exc:        # (an exception cannot cross the C frames: end the call, raise it afterwards)
                raised.append(exc)
                return 1

        callback = NESTED_STOP(_stop) if stop is not None else NESTED_STOP()
        opt = NestedOptions(int(const_hint), int(chunk), int(lanes), 1 if draw_live else 0, callback, None)
        stats = NestedStats()
        it = C.c_int64(int(iteration))
        if phantoms is not None:
            n = cols.size
            cap = rows * max(0, int(num_repeats) - 1) if phantom_capacity is None else int(phantom_capacity)
            size = max(cap, 0)
            ph_u, ph_lnl, ph_birth = np.empty((size, n)), np.empty(size), np.empty(size)
            ph_it, ph_k, ph_r = np.empty(size, dtype=np.int64), np.empty(size, dtype=np.int32), np.empty(size, dtype=np.int32)
            ph_c = np.zeros(size, dtype=np.int32) if clusters is not None else None
            ph = NestedPhantoms(float(phantoms.fraction), cap, _dp(ph_u), _dp(ph_lnl), _dp(ph_birth),
                                ph_it.ctypes.data_as(C.POINTER(C.c_int64)), _ip(ph_k), _ip(ph_r), None if ph_c is None else _ip(ph_c),
                                0, 0, 0)
            cl, dead_c, next_id = None, None, None
            if clusters is not None:
                if clusters.live_cluster.dtype != np.int32 or clusters.live_cluster.shape != (nlive,) or \
                        not clusters.live_cluster.flags['C_CONTIGUOUS']:
                    raise ValueError('clusters.live_cluster: a contiguous int32 array [nlive]')
                dead_c, next_id = np.zeros(rows, dtype=np.int32), C.c_int32(int(clusters.next_id))
                cl = NestedClusters(_ip(clusters.live_cluster), C.pointer(next_id), _ip(dead_c),
                                    VMX_NS_CLUSTER if cluster_flags is None else int(cluster_flags), 0)
            self._check(self.lib.vmx_nested_run_phantoms(self._h, C.byref(spec), _dp(live_u), _dp(live_lnl), C.byref(it), n_iterations,
                                                         _dp(dead_u), _dp(dead_lnl), _ip(dead_n), C.byref(opt), C.byref(stats),
                                                         None if cl is None else C.byref(cl), C.byref(ph)))
            if clusters is not None:
                clusters.next_id = int(next_id.value)
                clusters.dead.append(dead_c[:int(stats.iterations) * K])
            c = int(ph.count)
            phantoms.append(ph_u[:c], ph_lnl[:c], ph_birth[:c], np.stack([ph_it[:c], ph_k[:c], ph_r[:c]], axis=1),
                            None if ph_c is None else ph_c[:c])
        elif clusters is None:
            self._check(self.lib.vmx_nested_run(self._h, C.byref(spec), _dp(live_u), _dp(live_lnl), C.byref(it), n_iterations,
                                                _dp(dead_u), _dp(dead_lnl), _ip(dead_n), C.byref(opt), C.byref(stats)))
        else:
            if clusters.live_cluster.dtype != np.int32 or clusters.live_cluster.shape != (nlive,) or \
                    not clusters.live_cluster.flags['C_CONTIGUOUS']:
                raise ValueError('clusters.live_cluster: a contiguous int32 array [nlive]')
            dead_c, next_id = np.zeros(rows, dtype=np.int32), C.c_int32(int(clusters.next_id))
            flags = VMX_NS_CLUSTER if cluster_flags is None else int(cluster_flags)
            cl = NestedClusters(_ip(clusters.live_cluster), C.pointer(next_id), _ip(dead_c), flags, 0)
            self._check(self.lib.vmx_nested_run_clustered(self._h, C.byref(spec), _dp(live_u), _dp(live_lnl), C.byref(it), n_iterations,
                                                          _dp(dead_u), _dp(dead_lnl), _ip(dead_n), C.byref(opt), C.byref(stats),
                                                          C.byref(cl)))
            clusters.next_id = int(next_id.value)
            clusters.dead.append(dead_c[:int(stats.iterations) * K])
        if raised:
            raise raised[0]
        m = int(stats.iterations) * K
        return dead_u[:m], dead_lnl[:m], dead_n[:m], int(it.value), _stats_dict(stats)

    def nested_run_many(self, cols, lo, hi, theta_fixed, live_u, live_lnl, iteration, streams, n_iterations, threads, num_repeats,
                        mock_rows=None, log_norm=0.0, seed=0, const_hint=-1, chunk=0, lanes=0, draw_live=False, stop=None, phantoms=None):
        """Up to ``n_iterations`` iterations of each of E independent nested-sampling runs in one device run (include/vegamx.h:
        vmx_nested_run_many): ``live_u`` [E, nlive, n] / ``live_lnl`` [E, nlive] the runs' state and ``iteration`` int64 [E] their
        next iterations (all updated in place; a run without a finite live lnL keeps what it had), ``streams`` [E] the Philox
        stream of every run, ``mock_rows`` [E] the pool row every run is compared with (None: the installed data); the rest as for
        :meth:`nested_run`.  ``stop(run, iterations, dead_lnl [K], live_lnl [nlive])`` is asked after every iteration of every
        run; a true answer ends that run.  Returns (dead: per run (dead_u [m K, n], dead_lnl [m K], dead_nlive [m K]) for its m
        iterations done, status int32 [E], iterations_done int32 [E], statistics); the statistics carry ``per_run`` int64
        [E, 3]: rows evaluated, rows that were a thread's own position, set rounds the run took part in.  ``phantoms`` (a
        :class:`PhantomArrays` of E runs, at least ``n_iterations threads (num_repeats - 1)`` rows each): the set through
        vmx_nested_run_many_phantoms - every run's kept phantom points of this call are written into it (``phantoms.run(e)``); the
        runs themselves are the same runs."""
        _in_place(np.float64, live_u=live_u, live_lnl=live_lnl)
        _in_place(np.int64, iteration=iteration)
        if live_u.ndim != 3 or live_lnl.shape != live_u.shape[:2]:
            raise ValueError('live_u [E, nlive, n], live_lnl [E, nlive]')
        E, nlive = live_u.shape[:2]
        cols, lo, hi, theta_fixed, _ = self._sampled_box(cols, lo, hi, theta_fixed, live_u=live_u.reshape(-1, live_u.shape[-1]),
                                                         live_lnl=live_lnl.reshape(-1))
        if streams is not None:
            streams = np.ascontiguousarray(streams, dtype=np.uint64)
        if mock_rows is not None:
            mock_rows = np.ascontiguousarray(mock_rows, dtype=np.int32)
        if iteration.shape != (E,) or (streams is not None and streams.shape != (E,)) or \
                (mock_rows is not None and mock_rows.shape != (E,)):
            raise ValueError('iteration [E], streams [E], mock_rows [E]')
        K, n_iterations = int(threads), max(0, int(n_iterations))
        rows = n_iterations * max(K, 0)
        dead_u, dead_lnl, dead_n = np.empty((E, rows, cols.size)), np.empty((E, rows)), np.empty((E, rows), dtype=np.int32)
        status, done, per = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32), np.zeros((E, 3), dtype=np.int64)
        spec = NestedSpec(self.n_params, cols.size, _ip(cols), _dp(lo), _dp(hi), nlive, K, int(num_repeats), 0, float(log_norm),
                          int(seed), 0, _dp(theta_fixed))
        raised = []

        def _stop(_user, run, iterations, p_dead, p_live):
            try:
                return 1 if stop(int(run), int(iterations), np.ctypeslib.as_array(p_dead, (K,)),
                                 np.ctypeslib.as_array(p_live, (nlive,))) else 0
            except BaseException as exc:        # (an exception cannot cross the C frames: end the run, raise it afterwards)
                raised.append(exc)
                return 1

        callback = NESTED_SET_STOP(_stop) if stop is not None else NESTED_SET_STOP()
        opt = NestedSetOptions(int(const_hint), int(chunk), int(lanes), 1 if draw_live else 0, callback, None)
        stats = NestedStats()
        args = (self._h, C.byref(spec), E, None if streams is None else streams.ctypes.data_as(C.POINTER(C.c_uint64)),
                None if mock_rows is None else _ip(mock_rows), _dp(live_u), _dp(live_lnl), iteration.ctypes.data_as(C.POINTER(C.c_int64)),
                _ip(status), n_iterations, _dp(dead_u), _dp(dead_lnl), _ip(dead_n), _ip(done), C.byref(opt), C.byref(stats),
                per.ctypes.data_as(C.POINTER(C.c_int64)))
        if phantoms is None:
            self._check(self.lib.vmx_nested_run_many(*args))
        else:
            if not isinstance(phantoms, PhantomArrays) or phantoms.E != E or phantoms.n != cols.size:
                raise ValueError('phantoms: a PhantomArrays of the set\'s E runs and n sampled parameters')
            ph = phantoms.struct()
            self._check(self.lib.vmx_nested_run_many_phantoms(*args, C.byref(ph)))
        if raised:
            raise raised[0]
        dead = [(dead_u[e, :int(done[e]) * K].copy(), dead_lnl[e, :int(done[e]) * K].copy(), dead_n[e, :int(done[e]) * K].copy())
                for e in range(E)]
        return dead, status, done, dict(_stats_dict(stats), per_run=per)

    def nested_cluster_points(self, u, prev_id, next_id):
        """:func:`cluster_points` of this engine's device."""
        return cluster_points(u, prev_id, next_id, device=self.device)

    def _smc_arrays(self, ndim, cols, lo, hi, theta_fixed, u, lnl, n_stages, kept, topups, *, ess, sweeps, log_norm, seed, stream,
                    const_hint, chunk, lanes, draw):
        """What :meth:`smc_run` (``ndim`` 2: u [N, n]) and :meth:`smc_run_many` (3: u [E, N, n]) hand the library alike: the box and
        the particles checked as :meth:`_sampled_box` checks them; the spec; the call's arguments from ``n_stages`` to the record;
        its last arguments - with ``kept`` the SmcKeep of the positions' record and ``topups`` (a pointer to the rounds owed, or
        None), then the options and the statistics; ``stages(done, *run)``: the stage dicts of the first ``done`` record rows (of
        run ``run``); the statistics; last, what the pointers borrow."""
        _in_place(np.float64, u=u, lnl=lnl)
        if u.ndim != ndim or lnl.shape != u.shape[:-1]:
            raise ValueError('u [rows, n], lnl [rows]' if ndim == 2 else 'u [E, N, n], lnl [E, N]')
        cols, lo, hi, theta_fixed, _ = self._sampled_box(cols, lo, hi, theta_fixed, u=u.reshape(-1, u.shape[-1]), lnl=lnl.reshape(-1))
        n_stages, N = max(0, int(n_stages)), u.shape[-2]
        lead = u.shape[:-2] + (n_stages,)
        rec, rec_lnl, rec_anc = np.zeros(lead + (VMX_SMC_REC,)), np.empty(lead + (N,)), np.empty(lead + (N,), dtype=np.int32)
        rec_u = np.empty(lead + (N, cols.size)) if kept else None
        spec = SmcSpec(self.n_params, cols.size, _ip(cols), _dp(lo), _dp(hi), N, int(sweeps), float(ess), float(log_norm), int(seed),
                       int(stream), _dp(theta_fixed))
        opt = SmcOptions(int(const_hint), int(chunk), int(lanes), 1 if draw else 0)
        keep_arg = SmcKeep(_dp(rec_u), topups, 0) if kept else None
        stats = SmcStats()

        def stages(done, *run):
            r, r_lnl, r_anc = rec[run], rec_lnl[run], rec_anc[run]
            out = [dict(beta_prev=float(r[k, 0]), beta=float(r[k, 1]), ess=float(r[k, 2]), lnl=r_lnl[k].copy(), anc=r_anc[k].copy(),
                        accepted=int(r[k, 3]), scale=float(r[k, 4]), cholesky=bool(r[k, 5])) for k in range(int(done))]
            if kept:
                for k, row in enumerate(out):
                    row['u'] = rec_u[run][k].copy()
            return out

        tail = ((C.byref(keep_arg),) if kept else ()) + (C.byref(opt), C.byref(stats))
        return spec, (n_stages, _dp(rec), _dp(rec_lnl), _ip(rec_anc)), tail, stages, stats, (cols, lo, hi, theta_fixed, opt, keep_arg)

    def smc_run(self, cols, lo, hi, theta_fixed, u, lnl, stage, beta, scale, n_stages, ess, sweeps, log_norm=0.0, seed=0, stream=0,
                const_hint=-1, chunk=0, lanes=0, draw=False, keep=False, topups_left=None):
        """Up to ``n_stages`` stages of the tempered SMC sampler on the device (include/vegamx.h: vmx_smc_run): ``cols`` the sampled
        parameter columns with their box [lo, hi], ``theta_fixed`` the row of the others, ``u`` [N, n] in the unit cube / ``lnl``
        [N] the particles (updated in place; drawn first with ``draw``), ``stage`` the global index of the next stage, ``beta`` and
        ``scale`` its inverse temperature and proposal scale.  Returns (record: one dict per stage done with beta_prev, beta, ess,
        lnl (before reweighting), anc, accepted, scale, cholesky; stage, beta, scale afterwards; statistics).

        ``keep`` or ``topups_left`` (an int) go through vmx_smc_run_kept: every stage dict also carries ``u``, the particles at the
        stage's entry, the call goes on at beta = 1 with up to ``topups_left`` posterior rounds (``n_stages`` bounds both kinds), and
        the rounds still owed are returned after ``scale``."""
        kept = bool(keep) or topups_left is not None
        owed = C.c_int32(int(topups_left or 0))
        spec, recs, tail, stages, stats, _held = self._smc_arrays(
            2, cols, lo, hi, theta_fixed, u, lnl, n_stages, kept, C.pointer(owed), ess=ess, sweeps=sweeps, log_norm=log_norm,
            seed=seed, stream=stream, const_hint=const_hint, chunk=chunk, lanes=lanes, draw=draw)
        st, b, sc = C.c_int64(int(stage)), C.c_double(float(beta)), C.c_double(float(scale))
        run = self.lib.vmx_smc_run_kept if kept else self.lib.vmx_smc_run
        self._check(run(self._h, C.byref(spec), _dp(u), _dp(lnl), C.byref(st), C.byref(b), C.byref(sc), *recs, *tail))
        out = (stages(stats.stages), int(st.value), float(b.value), float(sc.value))
        return out + ((int(owed.value),) if kept else ()) + (_stats_dict(stats),)

    def smc_run_many(self, cols, lo, hi, theta_fixed, u, lnl, stage, beta, scale, streams, n_stages, ess, sweeps, mock_rows=None,
                     log_norm=0.0, seed=0, const_hint=-1, chunk=0, lanes=0, draw=False, keep=False, topups_left=None):
        """Up to ``n_stages`` stage rounds of E independent SMC runs in one device run (include/vegamx.h: vmx_smc_run_many): ``u``
        [E, N, n] / ``lnl`` [E, N] the particles, ``stage`` int64 [E] / ``beta`` [E] / ``scale`` [E] the runs' own state (all updated
        in place; a failed run's part is left as it was), ``streams`` [E] the Philox stream of every run, ``mock_rows`` [E] the pool
        row every run is compared with (None: the installed data); the rest as for :meth:`smc_run`.  Returns (records: for every
        run the list of stage dicts of the stages done, status int32 [E], stages_done int32 [E], statistics); the statistics
        carry ``per_run`` int64 [E, 4]: accepted, rows that were a particle's own position, rejected for a failed model, rows
        evaluated.

        ``keep`` or ``topups_left`` (int32 [E], updated in place: the posterior rounds every run still owes) go through
        vmx_smc_run_many_kept: every stage dict also carries ``u``, the run's particles at the stage's entry."""
        _in_place(np.float64, beta=beta, scale=scale)
        _in_place(np.int64, stage=stage)
        kept = bool(keep) or topups_left is not None
        if topups_left is not None:
            _in_place(np.int32, topups_left=topups_left)
        spec, recs, tail, stages, stats, _held = self._smc_arrays(
            3, cols, lo, hi, theta_fixed, u, lnl, n_stages, kept, None if topups_left is None else _ip(topups_left), ess=ess,
            sweeps=sweeps, log_norm=log_norm, seed=seed, stream=0, const_hint=const_hint, chunk=chunk, lanes=lanes, draw=draw)
        E = u.shape[0]
        if streams is not None:
            streams = np.ascontiguousarray(streams, dtype=np.uint64)
        if mock_rows is not None:
            mock_rows = np.ascontiguousarray(mock_rows, dtype=np.int32)
        if stage.shape != (E,) or beta.shape != (E,) or scale.shape != (E,) or (streams is not None and streams.shape != (E,)) or \
                (mock_rows is not None and mock_rows.shape != (E,)):
            raise ValueError('stage [E], beta [E], scale [E], streams [E], mock_rows [E]')
        if topups_left is not None and topups_left.shape != (E,):
            raise ValueError('topups_left [E]')
        status, done, per = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32), np.zeros((E, 4), dtype=np.int64)
        run = self.lib.vmx_smc_run_many_kept if kept else self.lib.vmx_smc_run_many
        self._check(run(self._h, C.byref(spec), E, None if streams is None else streams.ctypes.data_as(C.POINTER(C.c_uint64)),
                        None if mock_rows is None else _ip(mock_rows), _dp(u), _dp(lnl), stage.ctypes.data_as(C.POINTER(C.c_int64)),
                        _dp(beta), _dp(scale), _ip(status), *recs, _ip(done), *tail, per.ctypes.data_as(C.POINTER(C.c_int64))))
        return [stages(done[e], e) for e in range(E)], status, done, dict(_stats_dict(stats), per_run=per)

    def derived_const_hint(self, cols):
        """The table level that batches whose rows differ only in the columns ``cols`` allow (include/vegamx.h:
        vmx_derived_const_hint): 0, 1 (Arinyo parameters shared) or 2 (and the Gaussian-factor parameters)."""
        varies = np.zeros(self.n_params, dtype=np.int32)
        varies[np.asarray(cols, dtype=int)] = 1
        return self._check(self.lib.vmx_derived_const_hint(self._h, _ip(varies)))

    def set_constant_nl_hint(self, on=True, gaussian=False):
        """For ``eval_device``: the caller asserts that the Arinyo parameters - with ``gaussian`` also the smoothing,
        peak-broadening and Gaussian velocity-dispersion parameters - are identical for all walkers of a batch
        (violations are flagged per walker, never silently wrong)."""
        self._check(self.lib.vmx_set_constant_nl_hint(self._h, 0 if not on else 2 if gaussian else 1))
        self.nl_hint = 0 if not on else 2 if gaussian else 1

    def stream_handle(self):
        """hipStream_t of the engine as an integer (for ``torch.cuda.ExternalStream``)."""
        return int(self.lib.vmx_stream(self._h))

    def last_stream_handle(self):
        """hipStream_t of the last ``eval_device`` (with two lanes: the lane it ran on)."""
        return int(self.lib.vmx_last_stream(self._h))

    def set_lanes(self, lanes):
        """1 or 2 batches in flight for chi2-only ``eval_device`` calls (include/vegamx.h: vmx_set_lanes); the second lane
        borrows every static tensor of the engine."""
        self._check(self.lib.vmx_set_lanes(self._h, int(lanes)))
        self.lanes = int(lanes)

    def set_data(self, name, masked_data):
        qi = self.item_names.index(name)
        d = _f64(masked_data)
        self._check(self.lib.vmx_item_set_data(self._h, qi, _dp(d), d.size))

    def set_mock_pool(self, name, pool):
        """Masked mock data vectors [n_mocks, n_masked] of item ``name`` (Monte-Carlo fits)."""
        qi = self.item_names.index(name)
        pool = _f64(np.atleast_2d(pool))
        self._check(self.lib.vmx_item_set_mock_pool(self._h, qi, _dp(pool), pool.shape[0], pool.shape[1]))

    def set_mock_index(self, index=None):
        """Per-walker pool row used as data in the following evaluations (None: the items' own data)."""
        if index is None:
            self._check(self.lib.vmx_set_mock_index(self._h, None, 0))
        else:
            idx = np.ascontiguousarray(index, dtype=np.int32)
            self._check(self.lib.vmx_set_mock_index(self._h, _ip(idx), idx.size))

    def set_invcov(self, name, invcov):
        qi = self.item_names.index(name)
        m = _f64(invcov)
        self._check(self.lib.vmx_item_set_matrix(self._h, qi, MAT_INVCOV, 0, m.shape[0], m.shape[1], _dp(m)))

    def debug_read(self, what, index=0, count=0):
        out = np.empty(count)
        n = self.lib.vmx_debug_read(self._h, what, index, _dp(out), out.size)
        if n < 0:
            raise EngineError(self.lib.vmx_last_error().decode())
        return out[:n]

    def pk_multipoles(self, B=1):
        """P_ell(k) of the last evaluation (batch size B): dict pipeline id -> [B, 4, nk] for the pipelines that form
        their multipoles per walker (the stage tap behind `model_pk`, reference model.py:106-107)."""
        nk = self.prob.k.size
        nkp = (nk + sum(self.fftlog_pads) + 31) // 32 * 32          # (a row: the samples, then the FFTLog's power-law pads)
        out = {}
        n_cols = None
        for pid in range(self.n_pipelines):
            col = self.lib.vmx_pipeline_column(self._h, pid)
            if -3 < col < 0:            # (-1 / -2: an error code; <= -3 encodes "no column" and the column count)
                raise EngineError(self.lib.vmx_last_error().decode())
            if col < -2:
                n_cols = -3 - col
                continue
            out[pid] = col
        if n_cols is None:
            n_cols = len(out)
        pl = self.debug_read(0, 0, 4 * B * n_cols * nkp).reshape(4, n_cols, B, nkp)      # pipeline-major columns
        return {pid: np.ascontiguousarray(pl[:, col, :, :nk].transpose(1, 0, 2)) for pid, col in out.items()}

    def metal_xi(self, item_name, pair_index):
        """Correlation of one metal pair in the last evaluation (walker 0): after its metal matrix, before the
        bias product and the multiplicity."""
        g, pid, has_matrix = self.metal_source[(item_name, pair_index)]
        n = self.prob.items[item_name].model_grid.size
        cap = self.max_batch * ((n + 31) // 32 * 32)
        if has_matrix:
            return self.debug_read(3, g, cap)[:n].copy()
        return self.debug_read(1, pid, cap)[:n].copy()

    def set_direct_pk(self, pk=None):
        """direct_pk mode: per-walker linear spectra [B, nk] (None: back to the fiducial template)."""
        if pk is None:
            self._check(self.lib.vmx_set_direct_pk(self._h, None, 0, 0))
            return
        pk = _f64(np.atleast_2d(pk))
        self._check(self.lib.vmx_set_direct_pk(self._h, _dp(pk), pk.shape[0], pk.shape[1]))

    QUADRATIC_FORM_KINDS = {'auto': 0, 'q': 1, 'factored': 2}

    def set_quadratic_form_kind(self, kind='auto'):
        """'auto' (the cheaper form per engine), 'q' (the half-form matrix Q', nq^2 flops per walker) or 'factored'
        (|| U r0 - F dx ||^2, 2 n_masked nq flops: model grids much finer than the data grid) - include/vegamx.h:
        vmx_set_quadratic_form_kind."""
        self._check(self.lib.vmx_set_quadratic_form_kind(self._h, self.QUADRATIC_FORM_KINDS[kind]))

    # ---- operands of the spline-bins stage (include/vegamx.h: vmx_debug_read 6 ... 19, 4 [9]; vmx_debug_math)
    ROUTE_BITS = {'general': 1, 'static_taps': 2, 'static': 4, 'static_nw': 8, 'lean': 16, 'group': 32, 'static_group': 64,
                  'assemble_quad': 128, 'assemble_quad_general': 256, 'quad_plain': 512, 'same_grid': 1024, 'poly_bins': 2048}
    # (the order of VMX_DEBUG_SCALARS in include/vegamx.h; tests/test_xi_bins_host.py holds the two together)
    BINS_SCALAR_NAMES = ('AP', 'AT', 'DRP', 'EV1A', 'EV1B', 'EV2A', 'EV2B', 'BIAS1', 'BB1', 'BIAS2', 'BB2',
                         'RAD_S', 'RAD_A', 'RAD_L', 'RAD_D', 'RAD_IL', 'RAD_ID')
    BINS_STATIC_NAMES = ('r', 'rp', 'rt', 'z', 'relz', 'lnrelz', 'lnrelz2', 'growth')
    MATH_FUNCTIONS = {'log': 0, 'exp': 1, 'rsqrt': 2}

    def bins_route(self):
        """The bins kernels the last evaluation launched: the set of ROUTE_BITS names (vmx_debug_read 4 [9])."""
        mask = int(self.debug_read(4, 0, 10)[9])
        return {name for name, bit in self.ROUTE_BITS.items() if mask & bit}

    FFTLOG_FORM_BITS = {'gemv1': 1, 'gemv': 2, 'mfma64': 4, 'mfma32': 8, 'ring': 16, 'batch_x': 32, 'batch_y': 64, 'k_limit': 128}

    def fftlog_form(self):
        """The form the FFTLog o spline product of the last evaluation took: the set of FFTLOG_FORM_BITS names, with 'nb2' / 'nb4'
        / 'nb8' for the streaming kernel's columns per pass (vmx_debug_read 4 [10]; empty: no such product ran)."""
        mask = int(self.debug_read(4, 0, 11)[10])
        form = {name for name, bit in self.FFTLOG_FORM_BITS.items() if mask & bit}
        if mask >> 8:
            form.add(f'nb{mask >> 8}')
        return form

    def bins_scalar_index(self):
        """{'NS': row length, 'AP': index, ...} of a walker's scalars as the bins kernels read them (vmx_debug_read 7)."""
        idx = self.debug_read(7, 0, 32).astype(int)
        names = ('NS',) + self.BINS_SCALAR_NAMES
        assert idx.size == len(names)
        return dict(zip(names, idx.tolist()))

    def bins_scalars(self, B):
        """The walkers' scalars of the last evaluation [B, n_pipelines, NS] (vmx_debug_read 6)."""
        ns = self.bins_scalar_index()['NS']
        return self.debug_read(6, 0, B * self.n_pipelines * ns).reshape(B, self.n_pipelines, ns).copy()

    def bins_static(self, pid):
        """The per-bin static arrays of a pipeline as uploaded: {'r', 'rp', 'rt', 'z', 'relz', 'lnrelz', 'lnrelz2', 'growth'}."""
        n = int(self.bins_grid(pid)['n'])
        arr = self.debug_read(8, pid, 8 * n).reshape(8, n)
        return {name: arr[i].copy() for i, name in enumerate(self.BINS_STATIC_NAMES)}

    def bins_grid(self, pid):
        """The spline grid and the pipeline's place on it (vmx_debug_read 9)."""
        g = self.debug_read(9, pid, 32)
        out = dict(n_coef=int(g[0]), ncp=int(g[1]), same_grid=bool(g[2]), extrapolate=bool(g[3]), n_columns=int(g[4]))
        per_ell = g[5:21].reshape(4, 4)
        out.update(x0=per_ell[:, 0].copy(), h=per_ell[:, 1].copy(), inv_h=per_ell[:, 2].copy(), xlast=per_ell[:, 3].copy())
        out.update(column=int(g[21]), n=int(g[22]), n_pad=int(g[23]), split_evol=bool(g[24]), static_basis=int(g[25]),
                   static_bins=bool(g[26]), odd_x0=float(g[27]), odd_h=float(g[28]), odd_ncoef=int(g[29]))
        return out

    def bins_coefficients(self, B):
        """The spline coefficients of the last evaluation [4, n_columns, B, ncp] (vmx_debug_read 2)."""
        g = self.bins_grid(0)
        return self.debug_read(2, 0, 4 * B * g['n_columns'] * g['ncp']).reshape(4, g['n_columns'], B, g['ncp']).copy()

    def bins_xi(self, pid, B):
        """xi of a pipeline in the last evaluation [B, n_pad] (vmx_debug_read 1)."""
        g = self.bins_grid(pid)
        return self.debug_read(1, pid, B * g['n_pad']).reshape(B, g['n_pad']).copy()

    def quad_vector(self, name, B):
        """(x' - x0' [B, nq_pad], x0' [nq_pad]) of an item after a chi2-only evaluation (vmx_debug_read 10, 11)."""
        qi = self.item_names.index(name)
        x0 = self.debug_read(11, qi, self.prob.items[name].model_grid.size + 128).copy()      # (nq <= n_model + 64, padded to 32)
        return self.debug_read(10, qi, B * x0.size).reshape(B, x0.size).copy(), x0

    def lean_groups(self, static=False):
        """The groups of lean (static: of static-coordinate) pipelines whose bins arrive pre-summed (vmx_debug_read 13 / 18): a
        list of dict(n, n_pad, presum, members=[(pipeline, factor kind, factor index)])."""
        what = 18 if static else 13
        n_groups = int(self.debug_read(what, -1, 1)[0])
        out = []
        for g in range(n_groups):
            d = self.debug_read(what, g, 64)
            members = [tuple(int(v) for v in d[5 + 3 * m:8 + 3 * m]) for m in range(int(d[1]))]
            out.append(dict(n=int(d[2]), n_pad=int(d[3]), presum=bool(d[4]), members=members))
        return out

    def lean_group_sum(self, g, B, static=False):
        """The pre-summed array [B, n_pad] of group g after an evaluation that summed on the way (vmx_debug_read 14 / 19)."""
        n_pad = self.lean_groups(static)[g]['n_pad']
        return self.debug_read(19 if static else 14, g, B * n_pad).reshape(B, n_pad).copy()

    def poly_coefficients(self):
        """The static coefficient basis [4, n_static, 3, ncp] (vmx_debug_read 15)."""
        g = self.bins_grid(0)
        n_static = sum(self.bins_grid(p)['static_basis'] >= 0 for p in range(self.n_pipelines))
        return self.debug_read(15, 0, 4 * n_static * 3 * g['ncp']).reshape(4, n_static, 3, g['ncp']).copy()

    def odd_coefficients(self, pid):
        """The odd-multipole coefficient rows [4, odd_ncoef] of a pipeline (vmx_debug_read 16)."""
        n = self.bins_grid(pid)['odd_ncoef']
        return self.debug_read(16, pid, 4 * n).reshape(4, n).copy()

    def metal_factors(self, B):
        """The metal pairs' walker factors [B, 3, n_metals] of the last evaluation (vmx_debug_read 17)."""
        n = len(self.metal_source)
        return self.debug_read(17, 0, B * 3 * n).reshape(B, 3, n).copy()

    def poly_bins(self, pid):
        """The static basis on the bins of a pipeline [3, n_pad], None for a pipeline without (vmx_debug_read 12)."""
        g = self.bins_grid(pid)
        if not g['static_bins']:
            return None
        return self.debug_read(12, pid, 3 * g['n_pad']).reshape(3, g['n_pad']).copy()

    def debug_math(self, which, x):
        """vmx_log / vmx_exp / vmx_rsqrt of the kernels, elementwise on the device ('log' | 'exp' | 'rsqrt')."""
        x = _f64(np.ravel(x))
        out = np.empty_like(x)
        self._check(self.lib.vmx_debug_math(self._h, self.MATH_FUNCTIONS[which], _dp(x), x.size, _dp(out)))
        return out

    def last_form(self):
        """Form the last evaluation took: 'full' (distortion + C^-1 products), 'q' or 'factored'."""
        return ('full', 'q', 'factored')[int(self.debug_read(4, 0, 9)[8])]

    def set_quadratic_form(self, on=True):
        """Switch the quadratic form of chi2-only evaluations on (expansion point: the configured parameter values) or
        off (every evaluation runs the full chain).  Returns whether the form is in use."""
        ref = _f64(self.low.theta0)
        self.quadratic_form = bool(self._check(self.lib.vmx_set_quadratic_form(self._h, _dp(ref) if on else None))) and on
        return self.quadratic_form

    def mu_nodes(self):
        """(mu, w) of the extra nodes of the mu rule as the engine holds them."""
        n = self._check(self.lib.vmx_get_mu_nodes(self._h, None, None, 0))
        mu, w = np.empty(n), np.empty(n)
        self._check(self.lib.vmx_get_mu_nodes(self._h, _dp(mu), _dp(w), n))
        return mu, w

    def set_mu_quadrature(self, node_rule=True):
        """True: the node rule that reproduces the reference's 1000-point mu sums from 178 evaluations (default);
        False: the 1000-point loop itself.  Returns the setting in effect."""
        return bool(self._check(self.lib.vmx_set_mu_quadrature(self._h, int(bool(node_rule)))))

    def set_linear_spectra(self, pk_full, pk_smooth):
        """Replace the template's linear spectra (``Model.compute(pars, pk_full, pk_smooth)``, reference
        model.py:157-187); the peak spectrum is their difference (model.py:177)."""
        pk_full, pk_smooth = _f64(pk_full), _f64(pk_smooth)
        if pk_full.shape != (self.prob.k.size,) or pk_smooth.shape != pk_full.shape:
            raise ValueError('pk_full and pk_smooth live on the template k grid')
        peak = _f64(pk_full - pk_smooth)
        self._check(self.lib.vmx_set_linear_spectra(self._h, _dp(peak), _dp(pk_smooth), _dp(pk_full), pk_full.size))

    def marg_coeff(self, name, B):
        """Marginalisation-template coefficients [B, n_templates] of item ``name`` for the last evaluation (its batch
        size B): the static map of the residual, applied by the engine's product kernels."""
        qi = self.item_names.index(name)
        nt = self.prob.items[name].marg_diff2coeff.shape[0]
        out = np.empty((B, nt))
        self._check(self.lib.vmx_marg_coeff(self._h, qi, _dp(out), B))
        return out

    def marg_layout(self):
        """{item name: (first column, count)} of the rows ``marg_coeff_device`` writes, and their total width - items in the
        engine's order, those without templates left out (include/vegamx.h: vmx_marg_layout)."""
        layout = {}
        for qi, name in enumerate(self.item_names):
            off, cnt = C.c_int32(0), C.c_int32(0)
            total = self._check(self.lib.vmx_marg_layout(self._h, qi, C.byref(off), C.byref(cnt)))
            if cnt.value > 0:
                layout[name] = (off.value, cnt.value)
        return layout, (total if self.item_names else 0)

    def marg_coeff_device(self, d_theta_ptr, B, d_out_ptr, ld, d_status_ptr=None):
        """Marginalisation-template coefficients of B walkers in device memory as rows of ``d_out_ptr`` [B][ld] (columns:
        ``marg_layout``), NaN where a walker's model failed; enqueued on the engine's stream, nothing crosses PCIe
        (include/vegamx.h: vmx_marg_coeff_device).  ``last_form()`` then tells which route served the call."""
        self._check(self.lib.vmx_marg_coeff_device(self._h, d_theta_ptr, B, d_out_ptr, ld, d_status_ptr))

    def set_parameter_transform(self, scale=None, shift=None):
        """Parameter-level blinding: every walker becomes scale * theta + shift (per column) before the model and the
        priors read it; None switches it off."""
        if scale is None:
            self._check(self.lib.vmx_set_parameter_transform(self._h, None, None))
            return
        scale, shift = _f64(scale), _f64(shift)
        if scale.shape != (self.n_params,) or shift.shape != (self.n_params,):
            raise ValueError('scale and shift hold one value per parameter column')
        self._check(self.lib.vmx_set_parameter_transform(self._h, _dp(scale), _dp(shift)))

    def set_metal_beta_override(self, beta=None):
        """Set-up hook: every tracer of a bias-free metal pipeline takes ``beta`` (None: back to the parameters)."""
        self._check(self.lib.vmx_set_metal_beta_override(self._h, int(beta is not None), 0.0 if beta is None else float(beta)))

    def matvec_device(self, d_A, rows, cols_padded, d_x, B, d_y):
        self._check(self.lib.vmx_matvec_device(self._h, d_A, rows, cols_padded, d_x, B, d_y))

    def matmul_host(self, A, X):
        """X @ A.T on the GPU for host arrays A [rows, cols], X [B, cols] (the product kernels of the chain)."""
        A, X = _f64(A), _f64(X)
        Y = np.empty((X.shape[0], A.shape[0]))
        self._check(self.lib.vmx_matmul_host(self._h, _dp(A), A.shape[0], A.shape[1], _dp(X), X.shape[0], _dp(Y)))
        return Y

    def set_profiling(self, on):
        self._check(self.lib.vmx_set_profiling(self._h, int(bool(on))))

    def set_profiling_classes(self, names, stride=1):
        """Time only the named kernel classes (see timings()) while profiling is on - every ``stride``-th launch of them
        (1 .. 16)."""
        index = {self.lib.vmx_kernel_name(i).decode(): i for i in range(VMX_N_KERNELS)}
        mask = 0
        for name in names:
            mask |= 1 << index[name]
        self._check(self.lib.vmx_set_profiling_mask(self._h, mask | ((min(max(int(stride), 1), 16) - 1) << 28)))

    def timings(self, reset=True):
        ms = np.zeros(VMX_N_KERNELS)
        n = np.zeros(VMX_N_KERNELS, dtype=np.int64)
        self._check(self.lib.vmx_get_timings(self._h, _dp(ms), n.ctypes.data_as(C.POINTER(C.c_int64)), int(reset)))
        return {self.lib.vmx_kernel_name(i).decode(): (float(ms[i]), int(n[i])) for i in range(VMX_N_KERNELS)}
