"""ctypes binding of libksfd_hip.so (include/ksfd_hip.h).

This is the binding INTEGRATION.md shows for the reference side.  There is no CPU fallback: if the
shared library is missing or no MI355X is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

from .config import CConfig, ProblemConfig
from .layout import PETSC, SOA, HDF5  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libksfd_hip.so')
NKCLASS = 14

OK, EINVAL, EHIP, ENOMEM, ELINEAR, ENAN, EREJECT, ECOMM = range(8)

# kernel classes of ksfd_profile / ksfd_bench_kernel
KC_RHS, KC_JVP, KC_MULTIDOT, KC_GSUPDATE, KC_LINCOMB, KC_BASISAXPY, KC_FINISH, KC_REDUCE, \
    KC_GFIELD, KC_VELOCITY, KC_MISC, KC_HALO, KC_MG, KC_SPECTRAL = range(14)
PC_NONE, PC_MULTIGRID, PC_POLYNOMIAL, PC_SPECTRAL, PC_DIRECT, PC_BANDED = 1, 2, 4, 8, 16, 32      # bits of StepStats.pc_used
PC_MG_COARSE_DIRECT = 64    # ... a V cycle of the call ended in a direct coarse solve (set_mg_coarse kind 1)
DIRECT_MAX = 32768      # KSFD_DIRECT_MAX: largest F * local points of the direct solver (pc_type 5)
MG_DIRECT_MAX = 2048    # KSFD_MG_DIRECT_MAX: largest F * points of a level the direct coarse solver of the V cycle takes
MG_COARSE_CHEB, MG_COARSE_LU = 0, 1      # kind of set_mg_coarse


class KSFDError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('ksfd_hip error %d: %s' % (code, msg))
        self.code = code


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_int32)
ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)


class CDist(C.Structure):
    _fields_ = [('rank', C.c_int32), ('size', C.c_int32), ('transport', C.c_int32), ('device', C.c_int32),
                ('nccl_id', C.c_void_p), ('exchange', EXCHANGE_FN), ('allreduce', ALLREDUCE_FN),
                ('ctx', C.c_void_p), ('alltoall', ALLTOALL_FN)]


class StepOpts(C.Structure):
    _fields_ = [('rtol', C.c_double), ('atol', C.c_double), ('adapt', C.c_int32), ('max_reject', C.c_int32),
                ('clip_lo', C.c_double), ('clip_hi', C.c_double), ('dt_min', C.c_double), ('dt_max', C.c_double),
                ('safety', C.c_double), ('reject_safety', C.c_double),
                ('ksp_rtol', C.c_double), ('ksp_atol', C.c_double),
                ('ksp_restart', C.c_int32), ('ksp_max_it', C.c_int32), ('pc_type', C.c_int32),
                ('reserved', C.c_int32)]


class StepStats(C.Structure):
    _fields_ = [('accepted', C.c_int32), ('rejections', C.c_int32), ('linear_its', C.c_int32),
                ('rhs_evals', C.c_int32), ('jvp_evals', C.c_int32), ('pc_used', C.c_int32),
                ('wrms', C.c_double), ('h_used', C.c_double), ('ksp_resid', C.c_double), ('bytes', C.c_double),
                ('launches', C.c_int32), ('host_syncs', C.c_int32), ('residual_evals', C.c_int32),
                ('predicted_final', C.c_int32)]


class Profile(C.Structure):
    _fields_ = [('ms', C.c_double * NKCLASS), ('bytes', C.c_double * NKCLASS), ('launches', C.c_int64 * NKCLASS),
                ('alg_bytes', C.c_double * NKCLASS)]


class DeflationStats(C.Structure):
    _fields_ = [('restarts', C.c_int32), ('kept', C.c_int32), ('stage_its', C.c_int32 * 4),
                ('true_resid_fail', C.c_int32), ('projections', C.c_int32), ('rounding_passes', C.c_int32),
                ('reserved', C.c_int32)]


class MGCoarseInfo(C.Structure):
    _fields_ = [('kind', C.c_int32), ('level', C.c_int32), ('nlevels', C.c_int32), ('F', C.c_int32), ('n', C.c_int64 * 3),
                ('unknowns', C.c_int64), ('factorizations', C.c_int32), ('solves', C.c_int32), ('fallbacks', C.c_int32),
                ('reserved', C.c_int32)]


class MGTailInfo(C.Structure):
    _fields_ = [('level', C.c_int32), ('nlevels', C.c_int32), ('max_points', C.c_int64), ('points', C.c_int64 * 8),
                ('lds_bytes', C.c_int64), ('launches', C.c_int64)]


class MGLevelInfo(C.Structure):
    _fields_ = [('level', C.c_int32), ('nlevels', C.c_int32), ('end_level', C.c_int32), ('F', C.c_int32), ('n', C.c_int64 * 3),
                ('sloc', C.c_int64), ('points', C.c_int64), ('path', C.c_int32), ('f32', C.c_int32), ('coef32', C.c_int32),
                ('can_fuse', C.c_int32), ('have_setup', C.c_int32), ('coarse_sweeps', C.c_int32), ('lam_max', C.c_double),
                ('ratio', C.c_double)]


class StageInfo(C.Structure):
    _fields_ = [('fuse_stage', C.c_int32), ('guess_on', C.c_int32), ('path', C.c_int32), ('rhs_strip', C.c_int32),
                ('seg', C.c_int32), ('nseg', C.c_int32), ('nstrips', C.c_int32), ('rows', C.c_int32), ('overlap', C.c_int32),
                ('dots_done', C.c_int32 * 4), ('guess_n', C.c_int32 * 4), ('bnorm2', C.c_double * 4), ('gb', C.c_double * 16),
                ('guess_c', C.c_double * 16), ('wrms', C.c_double), ('below', C.c_double)]


# regimes of ksfd_stage_rhs, operations of ksfd_stage_jvp, and the kernel paths both report
STAGE_PLAIN, STAGE_SPECTRAL, STAGE_MULTIGRID = range(3)
SJ_ACTION, SJ_RESIDUAL32, SJ_POLY = range(3)
JP_STRIP2D, JP_LDS3D, JP_STRIP3D, JP_GENERIC = range(4)

# parts of ksfd_mg_part (KSFD_MGP_*) and the kernel paths ksfd_mg_level_info reports
MGP_COEF, MGP_RESTRICT, MGP_PROLONG_ADD, MGP_OPERATOR, MGP_DINV, MGP_DINV_APPLY, MGP_SMOOTH, MGP_CYCLE = range(8)
MGP_TAIL = 8                                        # the coarse tail of set_mg_tail, at its first level
MG_PATH_STRIP2D, MG_PATH_STRIP3D, MG_PATH_GENERIC = 0, 2, 3

ROT_MAXIN, ROT_MAXOUT = 121, 18     # KSFD_ROT_MAXIN / KSFD_ROT_MAXOUT: limits of the basis rotation kernel
BENCH_ROTATE, BENCH_ROTATE_COMPOSED = 100, 101      # ksfd_bench_kernel: one-pass rotation 31 -> 11 vectors / 11 basis combinations
# operations of ksfd_krylov_op (KSFD_KOP_*), and the longest cycle of the pipelined solver (KSFD_ASYNC_MAXK)
KOP_LINCOMB, KOP_MULTIDOT, KOP_MULTIDOT_GRAM, KOP_GS_UPDATE, KOP_BASIS_AXPY, KOP_GS_UPDATE_DEV, KOP_GMRES_COEF = range(7)
ASYNC_MAXK = 32
BENCH_MGC_SETUP, BENCH_MGC_APPLY, BENCH_MGC_FACTOR_COLUMNS = 104, 105, 106    # ... set-up / apply of the exact coarse solve, per-column factorization of the same matrix
BENCH_BAND_FACTOR, BENCH_BAND_SOLVE = 102, 103      # ... one factorization (assembly included) / one solve of the banded direct solver

# the tuning word of set_tuning: KSFD_TUNE_* of include/ksfd_hip.h, name for name (tests/test_tuning_cpu.py), where each bit is described.
# A word replaces every switch, so a word that is to change one switch of a default handle is TUNE_FUSED | that bit
TUNE_FUSED, TUNE_RECOMPUTE_JVP, TUNE_NO_OVERLAP, TUNE_ASYNC_GMRES, TUNE_NO_RECYCLE, TUNE_RECYCLE_ALL = (1 << b for b in range(6))
TUNE_REC_KEEP_MASK = 7 << 6
(TUNE_POLY_FP64, TUNE_UNFUSED_STAGE, TUNE_NO_ZERO_COPY, TUNE_UNFUSED_SMOOTHER, TUNE_GENERIC_RHS3D, TUNE_NO_SPEC_GUESS, TUNE_NO_RHS_CARRY,
 TUNE_NO_SPEC_PREDICT, TUNE_NO_RESTART_GROWTH, TUNE_COLD_POWER, TUNE_MG_FP64, TUNE_REC_MG, TUNE_OWN_DOTS, TUNE_OLD_BOUNDARY,
 TUNE_NO_GPLANE) = (1 << b for b in range(9, 24))
MG_EAGER = -7           # KSFD_MG_EAGER: power_its of set_mg_params that launches the coarse cycle kernel by kernel


def TUNE_REC_KEEP(v):
    """KSFD_TUNE_REC_KEEP(v): the field of the tuning word that keeps v leading Arnoldi vectors per stage (0: the count in force)"""
    return (v & 7) << 6

_lib = None

# every symbol include/ksfd_hip.h declares (checked by tests/test_abi.py without a GPU)
ABI_SYMBOLS = [
    'ksfd_kernel_class_name', 'ksfd_rccl_unique_id', 'ksfd_create', 'ksfd_destroy', 'ksfd_last_error', 'ksfd_update_params', 'ksfd_set_stage_params',
    'ksfd_local_range', 'ksfd_local_size', 'ksfd_set_state', 'ksfd_get_state', 'ksfd_device_state',
    'ksfd_device_plane_stride', 'ksfd_device_interior_offset', 'ksfd_set_source', 'ksfd_rhs', 'ksfd_jvp',
    'ksfd_velocity', 'ksfd_velocity_max', 'ksfd_groom', 'ksfd_count_worms', 'ksfd_scale_rho', 'ksfd_mul_rho', 'ksfd_jacobian_nnz', 'ksfd_jacobian_csr', 'ksfd_set_state_random', 'ksfd_snapshot_begin', 'ksfd_snapshot_wait', 'ksfd_checkpoint',
    'ksfd_default_step_opts', 'ksfd_step', 'ksfd_get_last_error_vector', 'ksfd_set_profiling',
    'ksfd_get_profile', 'ksfd_synchronize', 'ksfd_bench_kernel', 'ksfd_set_tuning', 'ksfd_set_mg_params', 'ksfd_set_poly_params',
    'ksfd_spectral_apply', 'ksfd_set_spectral_params', 'ksfd_direct_apply', 'ksfd_banded_apply',
    'ksfd_set_deflation', 'ksfd_get_deflation_stats', 'ksfd_basis_rotate', 'ksfd_basis_capacity', 'ksfd_krylov_op',
    'ksfd_set_mg_agglomerate', 'ksfd_set_mg_coarse', 'ksfd_get_mg_coarse_info', 'ksfd_mg_coarse_apply', 'ksfd_mg_level_info', 'ksfd_mg_part',
    'ksfd_set_mg_tail', 'ksfd_get_mg_tail_info', 'ksfd_stage_rhs', 'ksfd_stage_jvp',
]


def load():
    """dlopen libksfd_hip.so and declare signatures.  Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KSFDError(EHIP, 'libksfd_hip.so not built (run `python -c "import __graft_entry__ as g; g.build()"` '
                              'or `make -C ksfd_amd/csrc`); there is no CPU fallback')
    L = C.CDLL(LIB_PATH)
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    L.ksfd_kernel_class_name.restype = C.c_char_p
    L.ksfd_kernel_class_name.argtypes = [C.c_int32]
    L.ksfd_rccl_unique_id.argtypes = [vp]
    L.ksfd_create.argtypes = [C.POINTER(CConfig), C.POINTER(CDist), C.POINTER(vp)]
    L.ksfd_destroy.argtypes = [vp]
    L.ksfd_destroy.restype = None
    L.ksfd_last_error.argtypes = [vp]
    L.ksfd_last_error.restype = C.c_char_p
    L.ksfd_update_params.argtypes = [vp, C.POINTER(CConfig)]
    L.ksfd_set_stage_params.argtypes = [vp, C.c_int32, C.POINTER(CConfig)]
    L.ksfd_local_range.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ksfd_local_size.argtypes = [vp]
    L.ksfd_local_size.restype = C.c_int64
    L.ksfd_set_state.argtypes = [vp, dp, C.c_int32]
    L.ksfd_get_state.argtypes = [vp, dp, C.c_int32]
    L.ksfd_device_state.argtypes = [vp]
    L.ksfd_device_state.restype = vp
    L.ksfd_device_plane_stride.argtypes = [vp]
    L.ksfd_device_plane_stride.restype = C.c_int64
    L.ksfd_device_interior_offset.argtypes = [vp]
    L.ksfd_device_interior_offset.restype = C.c_int64
    L.ksfd_set_source.argtypes = [vp, C.c_int32, C.c_int32, dp, C.c_int32]
    L.ksfd_rhs.argtypes = [vp, C.c_double, dp, dp, C.c_int32]
    L.ksfd_jvp.argtypes = [vp, dp, dp, dp, C.c_int32]
    L.ksfd_velocity.argtypes = [vp, dp, dp, C.c_int32]
    L.ksfd_velocity_max.argtypes = [vp, dp]
    L.ksfd_groom.argtypes = [vp]
    L.ksfd_count_worms.argtypes = [vp, dp]
    L.ksfd_scale_rho.argtypes = [vp, C.c_double]
    L.ksfd_mul_rho.argtypes = [vp, dp]
    L.ksfd_snapshot_begin.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    L.ksfd_snapshot_wait.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(C.c_double))]
    L.ksfd_checkpoint.argtypes = [vp, C.c_int32]
    L.ksfd_set_state_random.argtypes = [vp, C.POINTER(C.c_int64), dp, C.c_double]
    L.ksfd_jacobian_nnz.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.ksfd_jacobian_csr.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), dp]
    L.ksfd_default_step_opts.argtypes = [C.POINTER(StepOpts)]
    L.ksfd_default_step_opts.restype = None
    L.ksfd_step.argtypes = [vp, dp, dp, C.POINTER(StepOpts), C.POINTER(StepStats)]
    L.ksfd_get_last_error_vector.argtypes = [vp, dp, C.c_int32]
    L.ksfd_set_profiling.argtypes = [vp, C.c_int32]
    L.ksfd_get_profile.argtypes = [vp, C.POINTER(Profile), C.c_int32]
    L.ksfd_synchronize.argtypes = [vp]
    L.ksfd_bench_kernel.argtypes = [vp, C.c_int32, C.c_int32, dp, dp]
    L.ksfd_set_tuning.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.ksfd_set_mg_params.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double]
    L.ksfd_set_poly_params.argtypes = [vp, C.c_int32, C.c_double, C.c_double]
    L.ksfd_spectral_apply.argtypes = [vp, C.c_double, dp, dp, C.c_int32]
    L.ksfd_set_spectral_params.argtypes = [vp, C.c_double, C.c_int32]
    L.ksfd_direct_apply.argtypes = [vp, C.c_double, dp, dp, C.c_int32]
    L.ksfd_banded_apply.argtypes = [vp, C.c_double, dp, dp, C.c_int32]
    L.ksfd_set_deflation.argtypes = [vp, C.c_int32, C.c_int32]
    L.ksfd_get_deflation_stats.argtypes = [vp, C.POINTER(DeflationStats)]
    L.ksfd_basis_capacity.argtypes = [vp]
    L.ksfd_basis_capacity.restype = C.c_int32
    L.ksfd_basis_rotate.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, C.c_int32]
    L.ksfd_krylov_op.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp, C.c_double, C.c_double, dp, dp, dp, C.c_int32]
    L.ksfd_set_mg_coarse.argtypes = [vp, C.c_int32, C.c_int32]
    L.ksfd_set_mg_agglomerate.argtypes = [vp, C.c_int64]
    L.ksfd_get_mg_coarse_info.argtypes = [vp, C.POINTER(MGCoarseInfo)]
    L.ksfd_set_mg_tail.argtypes = [vp, C.c_int64]
    L.ksfd_get_mg_tail_info.argtypes = [vp, C.POINTER(MGTailInfo)]
    L.ksfd_mg_coarse_apply.argtypes = [vp, C.c_double, C.c_int32, dp, dp]
    L.ksfd_mg_level_info.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.POINTER(MGLevelInfo)]
    L.ksfd_mg_part.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, dp, dp, dp, dp]
    L.ksfd_stage_rhs.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, dp, dp, dp, C.POINTER(StageInfo), C.c_int32]
    L.ksfd_stage_jvp.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, dp, dp, dp, dp, dp, C.c_int32]
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def rccl_unique_id():
    """128-byte ncclUniqueId (call on rank 0, broadcast to the other ranks)."""
    buf = C.create_string_buffer(128)
    rc = load().ksfd_rccl_unique_id(C.cast(buf, C.c_void_p))
    if rc:
        raise KSFDError(rc, (load().ksfd_last_error(None) or b'').decode())
    return bytes(buf.raw)


def default_step_opts(**kw):
    o = StepOpts()
    load().ksfd_default_step_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError('unknown step option %r' % k)
        setattr(o, k, v)
    return o


class KSFDHip:
    """Owns one ksfd_handle (one GPU / one slab).  Host arrays are numpy float64, flat, local slab."""

    def __init__(self, cfg: ProblemConfig, dist: CDist = None):
        self.L = load()
        self.cfg = cfg
        self._ccfg = cfg.as_ctypes()
        self._dist = dist
        h = C.c_void_p()
        rc = self.L.ksfd_create(C.byref(self._ccfg), C.byref(dist) if dist is not None else None, C.byref(h))
        if rc:
            raise KSFDError(rc, (self.L.ksfd_last_error(None) or b'').decode())
        self.h = h
        self.F = cfg.F
        self.nlocal = int(self.L.ksfd_local_size(h))        # F * local points
        b, e = C.c_int64(), C.c_int64()
        self.L.ksfd_local_range(h, C.byref(b), C.byref(e))
        self.slow_range = (b.value, e.value)

    def close(self):
        if getattr(self, 'h', None):
            self.L.ksfd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise KSFDError(rc, (self.L.ksfd_last_error(self.h) or b'').decode())

    def _vec(self, a, n=None):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if a.size != (n if n is not None else self.nlocal):
            raise ValueError('expected %d doubles, got %d' % (n if n is not None else self.nlocal, a.size))
        return a

    # ---- state
    def set_state(self, u, layout=SOA):
        u = self._vec(u)
        self._chk(self.L.ksfd_set_state(self.h, _dp(u), layout))

    def get_state(self, layout=SOA):
        out = np.empty(self.nlocal)
        self._chk(self.L.ksfd_get_state(self.h, _dp(out), layout))
        return out

    def update_params(self, cfg: ProblemConfig):
        self.cfg = cfg
        self._ccfg = cfg.as_ctypes()
        self._chk(self.L.ksfd_update_params(self.h, C.byref(self._ccfg)))

    def set_stage_params(self, stage, cfg=None):
        """ps.values(t_stage) for the stage-th RHS evaluation of the next steps (None clears; stage -1 = all four)"""
        if cfg is None:
            self._chk(self.L.ksfd_set_stage_params(self.h, int(stage), None))
        else:
            c = cfg.as_ctypes()
            self._chk(self.L.ksfd_set_stage_params(self.h, int(stage), C.byref(c)))

    def set_source(self, field, src, stage=-1):
        if src is None:
            self._chk(self.L.ksfd_set_source(self.h, stage, field, None, SOA))
        else:
            s = self._vec(src, self.nlocal // self.F)
            self._chk(self.L.ksfd_set_source(self.h, stage, field, _dp(s), SOA))

    # ---- operators
    def rhs(self, u=None, t=0.0, layout=SOA):
        out = np.empty(self.nlocal)
        up = _dp(self._vec(u)) if u is not None else None
        self._chk(self.L.ksfd_rhs(self.h, float(t), up, _dp(out), layout))
        return out

    def jvp(self, v, u=None, layout=SOA):
        out = np.empty(self.nlocal)
        v = self._vec(v)
        up = _dp(self._vec(u)) if u is not None else None
        self._chk(self.L.ksfd_jvp(self.h, up, _dp(v), _dp(out), layout))
        return out

    def velocity(self, u=None):
        n = self.cfg.dim * (self.nlocal // self.F)
        out = np.empty(n)
        up = _dp(self._vec(u)) if u is not None else None
        self._chk(self.L.ksfd_velocity(self.h, up, _dp(out), SOA))
        return out

    def velocity_max(self):
        v = np.zeros(3)
        self._chk(self.L.ksfd_velocity_max(self.h, _dp(v)))
        return v

    # ---- outer-loop helpers
    def groom(self):
        self._chk(self.L.ksfd_groom(self.h))

    def count_worms(self):
        t = C.c_double()
        self._chk(self.L.ksfd_count_worms(self.h, C.byref(t)))
        return t.value

    def scale_rho(self, f):
        self._chk(self.L.ksfd_scale_rho(self.h, float(f)))

    def mul_rho(self, factor):
        f = self._vec(factor, self.nlocal // self.F)
        self._chk(self.L.ksfd_mul_rho(self.h, _dp(f)))

    def snapshot_begin(self, layout=SOA):
        """start an asynchronous copy of the state to pinned host memory; returns the slot to pass to snapshot_wait"""
        slot = C.c_int32()
        self._chk(self.L.ksfd_snapshot_begin(self.h, layout, C.byref(slot)))
        return slot.value

    def snapshot_wait(self, slot):
        """numpy view (no copy) of the pinned buffer; valid until the second-next snapshot_begin"""
        ptr = C.POINTER(C.c_double)()
        self._chk(self.L.ksfd_snapshot_wait(self.h, slot, C.byref(ptr)))
        return np.ctypeslib.as_array(ptr, shape=(self.nlocal,))

    def checkpoint(self):
        """device-side copy of the state + the solver's step-to-step memory (one slot)"""
        self._chk(self.L.ksfd_checkpoint(self.h, 0))

    def restore(self):
        self._chk(self.L.ksfd_checkpoint(self.h, 1))

    def set_state_random(self, z_coarse, rho0=9000.0):
        """start_values on the device: z_coarse indexed [i,j,k] (x first) on the global coarse grid (ksfdsolver2.py:580-639)"""
        z = np.asarray(z_coarse, dtype=np.float64)
        nc = (C.c_int64 * 3)(*(list(z.shape) + [1, 1, 1])[:3])
        zf = np.ascontiguousarray(z.ravel(order='F'))
        self._chk(self.L.ksfd_set_state_random(self.h, nc, _dp(zf), float(rho0)))

    def jacobian_csr(self):
        """Assembled df/du at the resident state: (rowptr, col, val), local rows, global columns, unknown = F*point + dof
        (the reference's Vec ordering; KSFD/ksfdsym.py:814-886 + ksfdMat.pyx:55-180)."""
        nr, nnz = C.c_int64(), C.c_int64()
        self._chk(self.L.ksfd_jacobian_nnz(self.h, C.byref(nr), C.byref(nnz)))
        rowptr = np.empty(nr.value + 1, dtype=np.int64)
        col = np.empty(nnz.value, dtype=np.int64)
        val = np.empty(nnz.value)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        self._chk(self.L.ksfd_jacobian_csr(self.h, ip(rowptr), ip(col), _dp(val)))
        return rowptr, col, val

    # ---- step
    def step(self, t, h, opts=None, raise_on_error=True):
        """One TS.step().  Returns (t_new, h_next, StepStats, rc)."""
        opts = opts or default_step_opts()
        tt, hh, st = C.c_double(t), C.c_double(h), StepStats()
        rc = self.L.ksfd_step(self.h, C.byref(tt), C.byref(hh), C.byref(opts), C.byref(st))
        if rc and raise_on_error:
            self._chk(rc)
        return tt.value, hh.value, st, rc

    def last_error(self):
        return (self.L.ksfd_last_error(self.h) or b'').decode()

    def last_error_vector(self, layout=SOA):
        out = np.empty(self.nlocal)
        self._chk(self.L.ksfd_get_last_error_vector(self.h, _dp(out), layout))
        return out

    # ---- measurement
    def set_profiling(self, on=True, only=None):
        """only: kernel class name ('jvp', ...) -- time just that class (cheaper: each event pair costs device time)"""
        code = int(bool(on))
        if on and only is not None:
            names = [self.L.ksfd_kernel_class_name(i).decode() for i in range(NKCLASS)]
            code = 2 + names.index(only)
        self._chk(self.L.ksfd_set_profiling(self.h, code))

    def profile(self, reset=False):
        p = Profile()
        self._chk(self.L.ksfd_get_profile(self.h, C.byref(p), int(reset)))
        names = [self.L.ksfd_kernel_class_name(i).decode() for i in range(NKCLASS)]
        return {n: dict(ms=p.ms[i], bytes=p.bytes[i], launches=p.launches[i], alg_bytes=p.alg_bytes[i]) for i, n in enumerate(names)}

    def synchronize(self):
        self._chk(self.L.ksfd_synchronize(self.h))

    def bench_kernel(self, cls, reps=20):
        ms, by = C.c_double(), C.c_double()
        self._chk(self.L.ksfd_bench_kernel(self.h, cls, reps, C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def set_mg_params(self, nu=0, ncoarse_max=0, power_its=0, ratio=0.0, coarse_tol=0.0):
        self._chk(self.L.ksfd_set_mg_params(self.h, nu, ncoarse_max, power_its, ratio, coarse_tol))

    def set_poly_params(self, max_degree, target=0.0, mg_threshold=0.0):
        self._chk(self.L.ksfd_set_poly_params(self.h, int(max_degree), float(target), float(mg_threshold)))

    def spectral_apply(self, shift, v, layout=SOA):
        """z = (shift*I - J0)^-1 v, J0 = constant-coefficient part of the Jacobian at the resident state (test entry)"""
        out = np.empty(self.nlocal)
        v = self._vec(v)
        self._chk(self.L.ksfd_spectral_apply(self.h, float(shift), _dp(v), _dp(out), layout))
        return out

    def direct_apply(self, shift, v, layout=SOA):
        """z = (shift*I - J)^-1 v by the direct solver's dense LU (pc_type 5), J = the Jacobian at the resident state (test entry)"""
        out = np.empty(self.nlocal)
        v = self._vec(v)
        self._chk(self.L.ksfd_direct_apply(self.h, float(shift), _dp(v), _dp(out), layout))
        return out

    def banded_apply(self, shift, v, layout=SOA):
        """z = (shift*I - J)^-1 v by the banded LU of the folded ring (pc_type 6, 1-D handles), J = the Jacobian at the resident state
        (test entry)"""
        out = np.empty(self.nlocal)
        v = self._vec(v)
        self._chk(self.L.ksfd_banded_apply(self.h, float(shift), _dp(v), _dp(out), layout))
        return out

    def set_mg_coarse(self, kind, max_unknowns=0):
        """Coarse solve of the multigrid V cycle.  kind 0 (MG_COARSE_CHEB): Chebyshev on the coarsest level, the default; 1 (MG_COARSE_LU):
        exact solve (dense LU + explicit inverse, rebuilt per set-up).  max_unknowns > 0: the cycle ends on the finest level below level 0
        with at most that many unknowns (<= MG_DIRECT_MAX), else on the coarsest.  KSFDError(EINVAL) leaves the handle as it was."""
        self._chk(self.L.ksfd_set_mg_coarse(self.h, int(kind), int(max_unknowns)))

    def set_mg_agglomerate(self, max_points):
        """Coarse-level agglomeration of the multigrid hierarchy on slab ranks (collective: every rank passes the same value).  0: off, the
        default.  > 0: levels below level 0 with at most that many GLOBAL points, and the level the 4-rows-per-rank rule would refuse,
        are replicated on every rank and coarsening goes on by the single-rank rule.  The hierarchy is rebuilt.  No effect on a handle
        without a halo transport; KSFDError(EINVAL) leaves the handle as it was."""
        self._chk(self.L.ksfd_set_mg_agglomerate(self.h, int(max_points)))

    def set_mg_tail(self, max_points):
        """The coarse tail of the multigrid V cycle in one workgroup launch (opt-in; collective on handles with a transport).  0: off, the
        default.  > 0: the sub-cycle from the first level t >= 1 below which every level is whole on this rank, has at most that many
        points and fits the LDS together, down to the level the cycle ends on and back, runs as ONE launch with the level vectors in
        the LDS.  No level qualifies: the cycle stays as it is (mg_tail_info()['level'] == -1).  Excludes set_mg_coarse(1);
        KSFDError(EINVAL) leaves the handle as it was.  Afterwards the hierarchy counts as not set up."""
        self._chk(self.L.ksfd_set_mg_tail(self.h, int(max_points)))

    def mg_tail_info(self):
        """dict(level (first tail level or -1), nlevels, max_points, points (per tail level), lds_bytes, launches (over the life of the
        handle))"""
        s = MGTailInfo()
        self._chk(self.L.ksfd_get_mg_tail_info(self.h, C.byref(s)))
        return dict(level=s.level, nlevels=s.nlevels, max_points=int(s.max_points), points=[int(x) for x in s.points[:s.nlevels]],
                    lds_bytes=int(s.lds_bytes), launches=int(s.launches))

    def mg_coarse_info(self):
        """the level the V cycle ends on and the counters of the exact coarse solve over the life of the handle:
        dict(kind, level, nlevels, F, n (3 extents), unknowns, factorizations, solves, fallbacks)"""
        s = MGCoarseInfo()
        self._chk(self.L.ksfd_get_mg_coarse_info(self.h, C.byref(s)))
        return dict(kind=s.kind, level=s.level, nlevels=s.nlevels, F=s.F, n=tuple(int(x) for x in s.n), unknowns=int(s.unknowns),
                    factorizations=s.factorizations, solves=s.solves, fallbacks=s.fallbacks)

    def mg_coarse_apply(self, shift, v, op=1):
        """on the level the V cycle ends on, at the resident state (test entry): op 0: (shift*I - J_c) v by the level's operator kernels,
        op 1: the direct coarse solve of v.  v, result: F * points of that level, SoA (x fastest, field slowest)"""
        n = self.mg_coarse_info()['unknowns']
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if v.size != n:
            raise ValueError('mg_coarse_apply: vector of %d entries, the level has %d unknowns' % (v.size, n))
        out = np.empty(n)
        self._chk(self.L.ksfd_mg_coarse_apply(self.h, float(shift), int(op), _dp(v), _dp(out)))
        return out

    def mg_level_info(self, level, shift=None):
        """geometry and kernel choice of one level of the V cycle (test entry, ksfd_mg_level_info): dict(level, nlevels, end_level, F, n,
        sloc, points, path, f32, coef32, can_fuse); with a shift, after a cold set-up at it, also have_setup, lam_max, ratio and
        coarse_sweeps.  Afterwards the hierarchy counts as not set up."""
        s = MGLevelInfo()
        self._chk(self.L.ksfd_mg_level_info(self.h, int(level), int(shift is not None), float(shift or 0.0), C.byref(s)))
        return dict(level=s.level, nlevels=s.nlevels, end_level=s.end_level, F=s.F, n=tuple(int(x) for x in s.n), sloc=int(s.sloc),
                    points=int(s.points), path=s.path, f32=bool(s.f32), coef32=s.coef32, can_fuse=bool(s.can_fuse),
                    have_setup=bool(s.have_setup), coarse_sweeps=s.coarse_sweeps, lam_max=s.lam_max, ratio=s.ratio)

    def mg_part(self, part, level, in0=None, in1=None, variant=0, nu=0, shift=0.0, ratio=0.0):
        """one part of the V cycle on host vectors through the wrappers the cycle calls (test entry, ksfd_mg_part; include/ksfd_hip.h has
        the parts and their variants).  Vectors: (planes, owned points of the level) or flat.  Returns out0 as (planes, points); COEF
        returns (planes, fp32 copy or None), DINV_APPLY (z, z2, rcopy)."""
        fine = self.mg_level_info(level)                   # refuses a handle without a hierarchy and a level out of range
        F, nlig = fine['F'], fine['F'] - 1
        coarse = self.mg_level_info(level + 1) if part in (MGP_RESTRICT, MGP_PROLONG_ADD) and level + 1 < fine['nlevels'] else fine
        n_in0, n_in1 = F * fine['points'], F * (coarse['points'] if part == MGP_PROLONG_ADD else fine['points'])
        planes, pts = {MGP_COEF: (3 + nlig, fine['points']), MGP_RESTRICT: (F, coarse['points']),
                       MGP_DINV: (F * F, fine['points'])}.get(part, (F, fine['points']))

        def vec(a, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
            if a.size != n:
                raise ValueError('mg_part: vector of %d entries, expected %d' % (a.size, n))
            return a
        a0, a1 = vec(in0, n_in0), vec(in1, n_in1)
        out0 = np.full((planes, pts), np.nan)
        out1 = np.full((2 * F if part == MGP_DINV_APPLY else planes, pts), np.nan) if part in (MGP_COEF, MGP_DINV_APPLY) else None
        p = lambda a: None if a is None else _dp(a)
        self._chk(self.L.ksfd_mg_part(self.h, int(part), int(level), int(variant), int(nu), float(shift), float(ratio),
                                      p(a0), p(a1), p(out0), p(out1)))
        if part == MGP_COEF:
            return out0, (out1 if fine['coef32'] & 2 else None)
        if part == MGP_DINV_APPLY:
            return out0, out1[:F], out1[F:]
        return out0

    def set_deflation(self, keep, carry_stages=False):
        """GMRES with deflated restarting for the stage solves: keep harmonic Ritz vectors (0 = off, at most 16) survive a restart;
        carry_stages: the kept space also serves the later stages of a step attempt"""
        self._chk(self.L.ksfd_set_deflation(self.h, int(keep), int(bool(carry_stages))))

    def deflation_stats(self):
        """of the last step() call: dict(restarts, kept, stage_its[4], true_resid_fail, projections, rounding_passes)"""
        s = DeflationStats()
        self._chk(self.L.ksfd_get_deflation_stats(self.h, C.byref(s)))
        return dict(restarts=s.restarts, kept=s.kept, stage_its=list(s.stage_its), true_resid_fail=s.true_resid_fail,
                    projections=s.projections, rounding_passes=s.rounding_passes)

    def basis_capacity(self):
        """vectors the Krylov basis V holds (restart length that fits + 1)"""
        return int(self.L.ksfd_basis_capacity(self.h))

    def basis_rotate(self, P, vin, layout=SOA):
        """V[:, :nout] <- V[:, :nin] P on the device (test entry): P (nin, nout), vin (nin, nlocal); returns (nin, nlocal) -- rows
        nout.. come back as they went in"""
        P = np.ascontiguousarray(P, dtype=np.float64)
        nin, nout = P.shape
        vin = np.ascontiguousarray(vin, dtype=np.float64)
        if vin.shape != (nin, self.nlocal):
            raise ValueError('expected vin of shape (%d, %d), got %r' % (nin, self.nlocal, vin.shape))
        out = np.empty((nin, self.nlocal))
        self._chk(self.L.ksfd_basis_rotate(self.h, nin, nout, _dp(P), _dp(vin), _dp(out), layout))
        return out

    def krylov_op(self, op, k, vecs=None, coef=None, alpha=1.0, beta=0.0, want_norm=False, layout=SOA):
        """one Krylov vector kernel through the solvers' launch wrappers (test entry, ksfd_krylov_op): vecs (nvec, nlocal) with the basis
        in rows 0..k-1 and w in row k (LINCOMB: its k inputs); returns (all nvec rows as the device left them, scalars).  KOP_GMRES_COEF:
        coef = the reduced rows of columns 0..k-1 one after the other, no vectors; returns (None, scalars)."""
        k = int(k)
        if op == KOP_GMRES_COEF:
            rows = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
            if k >= 0 and rows.size != k * k + 2 * k:
                raise ValueError('expected %d reduced numbers, got %d' % (k * k + 2 * k, rows.size))
            sc = np.full(max(k, 0) * (k + 3) + max(k, 0) * (k + 1) + k + 1 + 1, np.nan)
            self._chk(self.L.ksfd_krylov_op(self.h, op, k, 0, _dp(rows), float(alpha), float(beta), None, None, _dp(sc), layout))
            return None, sc[:-1]
        vecs = np.ascontiguousarray(vecs, dtype=np.float64)
        if vecs.ndim != 2 or vecs.shape[1] != self.nlocal:
            raise ValueError('expected vecs of shape (nvec, %d), got %r' % (self.nlocal, vecs.shape))
        nvec = k if op == KOP_LINCOMB else k + 1
        cap = self.basis_capacity()
        kmax = {KOP_LINCOMB: min(6, cap), KOP_MULTIDOT: cap - 1, KOP_MULTIDOT_GRAM: min(32, cap - 1), KOP_GS_UPDATE: cap - 1,
                KOP_BASIS_AXPY: cap - 1, KOP_GS_UPDATE_DEV: min(ASYNC_MAXK, cap - 1)}.get(op, -1)
        if (0 if op == KOP_MULTIDOT else 1) <= k <= kmax and vecs.shape[0] != nvec:      # a k the library takes: it will read nvec vectors
            raise ValueError('operation %d with k = %d takes %d vectors, got %d' % (op, k, nvec, vecs.shape[0]))
        c = np.ascontiguousarray(coef if coef is not None else np.zeros(max(k, 1)), dtype=np.float64).reshape(-1)
        if c.size < k:
            raise ValueError('expected %d coefficients, got %d' % (k, c.size))
        out = np.empty_like(vecs)
        sc = np.full(2 * max(k, 0) + 2, np.nan)
        self._chk(self.L.ksfd_krylov_op(self.h, op, k, int(bool(want_norm)), _dp(c), float(alpha), float(beta), _dp(vecs), _dp(out), _dp(sc), layout))
        n = {KOP_MULTIDOT: k + 1, KOP_MULTIDOT_GRAM: 2 * k + 1}.get(op, 1 if want_norm else 0)
        return out, sc[:n]

    def stage_rhs(self, regime, hstep, Y=None, nstages=4, finish=None, layout=SOA):
        """the stage right-hand sides of one attempt through the functions the step calls (test entry, ksfd_stage_rhs): Y (nstages - 1,
        nlocal) the caller's stage vectors, four of them with finish = (atol, rtol).  Returns (b (nstages, nlocal), info dict, fin) with
        fin = None or (new state, error vector); info: fuse_stage, guess_on, path, rhs_strip, seg, nseg, nstrips, rows, overlap,
        dots_done[4], guess_n[4], bnorm2[4], gb (4, 4), guess_c (4, 4), wrms, below."""
        nstages = int(nstages)
        ny = 4 if finish is not None else max(nstages - 1, 0)
        yv = None
        if Y is not None:
            yv = np.ascontiguousarray(Y, dtype=np.float64).reshape(-1)
            if 1 <= nstages <= 4 and yv.size != ny * self.nlocal:
                raise ValueError('stage_rhs: expected %d stage vectors of %d doubles, got %d doubles' % (ny, self.nlocal, yv.size))
        b = np.full((max(nstages, 1), self.nlocal), np.nan)
        fin = np.full((2, self.nlocal), np.nan) if finish is not None else None
        atol, rtol = finish if finish is not None else (0.0, 0.0)
        s = StageInfo()
        p = lambda a: None if a is None else _dp(a)
        self._chk(self.L.ksfd_stage_rhs(self.h, int(regime), nstages, float(hstep), float(atol), float(rtol), p(yv), _dp(b), p(fin),
                                        C.byref(s), layout))
        info = dict(fuse_stage=bool(s.fuse_stage), guess_on=bool(s.guess_on), path=s.path, rhs_strip=bool(s.rhs_strip), seg=s.seg, nseg=s.nseg,
                    nstrips=s.nstrips, rows=s.rows, overlap=bool(s.overlap), dots_done=[bool(x) for x in s.dots_done], guess_n=list(s.guess_n),
                    bnorm2=list(s.bnorm2), gb=np.array(s.gb).reshape(4, 4), guess_c=np.array(s.guess_c).reshape(4, 4), wrms=s.wrms, below=s.below)
        return b, info, (None if fin is None else (fin[0], fin[1]))

    def stage_jvp(self, op, v, y=None, mode=1, shift=1.0, alpha=0.0, beta=0.0, coef=None, layout=SOA):
        """one frozen Jacobian action at the resident state through the functions the solvers call (test entry, ksfd_stage_jvp).
        SJ_ACTION: modes 0..4 of op_jvp_frozen_halo; SJ_RESIDUAL32: the fp32 residual y - A v with ||r||^2 from its epilogue;
        SJ_POLY: sum_i coef[i] (A/shift)^i v by poly_apply.  Returns (out, dict(norm2, path, seg, nseg, nstrips, fp32, overlap, rows))."""
        v = self._vec(v)
        yv = self._vec(y) if y is not None else None
        c = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1) if coef is not None else None
        out = np.full(self.nlocal, np.nan)
        sc = np.full(8, np.nan)
        p = lambda a: None if a is None else _dp(a)
        self._chk(self.L.ksfd_stage_jvp(self.h, int(op), int(mode), float(shift), float(alpha), float(beta), (c.size - 1) if c is not None else 0,
                                        p(c), _dp(v), p(yv), _dp(out), _dp(sc), layout))
        return out, dict(norm2=sc[0], path=int(sc[1]), seg=int(sc[2]), nseg=int(sc[3]), nstrips=int(sc[4]), fp32=bool(sc[5]),
                         overlap=bool(sc[6]), rows=int(sc[7]))

    def set_spectral_params(self, from_stiffness=0.0, enable=-1):
        self._chk(self.L.ksfd_set_spectral_params(self.h, float(from_stiffness), int(enable)))

    def set_tuning(self, use_fused=-1, yseg=0, yseg_jvp=None):
        """use_fused: the tuning word, an OR of the TUNE_* constants of this module (the default handle is TUNE_FUSED).  Negative:
        no switch changes; any other word replaces every switch.  yseg / yseg_jvp: rows per wave segment, <= 0 keeps."""
        self._chk(self.L.ksfd_set_tuning(self.h, use_fused, yseg, yseg if yseg_jvp is None else yseg_jvp))
