"""ctypes binding of librqp_hip.so (include/rqp_abi.h).

This is the only module that touches the shared library.  There is NO fallback:
if the library is missing, or no HIP device is visible, the product path raises
(``RqpUnavailable``) -- it never routes to a CPU implementation.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RQP_LIB", os.path.join(_HERE, "lib", "librqp_hip.so"))

RQP_F32, RQP_F64 = 0, 1
RQP_TILE_SAME, RQP_TILE_F16, RQP_TILE_BF16 = 0, 1, 2
KERNELS = {"auto": 0, "generic": 1, "resident": 2, "resident2": 2, "wave": 3, "mfma": 4}     # enum rqp_kernel
RQP_ERR_ARG, RQP_ERR_STATE, RQP_ERR_UNSUPPORTED = -1, -2, -5
FLAG_LOW_MEMORY = 1          # rqp_dims.flags
FLAG_FULL_LADDER = 2
STATUS_STR = {0: "solved", 1: "max_iters_reached", 2: "nan_detected", 3: "primal_infeasible", 4: "dual_infeasible",
              5: "window_passes_exhausted", -1: "unsolved"}

# every symbol include/rqp_abi.h declares (tests check the .so exports all of them)
ABI_SYMBOLS = (
    "rqp_default_settings", "rqp_create", "rqp_setup", "rqp_update", "rqp_update_mats", "rqp_update_affine",
    "rqp_update_settings",
    "rqp_warm_start", "rqp_clear_primal_dual", "rqp_solve", "rqp_iterate", "rqp_compute_residuals",
    "rqp_get_state", "rqp_get_rhos", "rqp_get_K", "rqp_dispatch_history", "rqp_get_dispatch", "rqp_get_window", "rqp_set_window_passes", "rqp_set_polish", "rqp_get_polish", "rqp_set_adjoint", "rqp_adjoint", "rqp_set_sensitivity", "rqp_sensitivity",
    "rqp_ltv_workspace_bytes", "rqp_ltv_condense", "rqp_ltv_vectors", "rqp_ltv_adjoint_workspace_bytes",
    "rqp_ltv_condense_adjoint", "rqp_ltv_stage_rows", "rqp_ltv_stage_vectors", "rqp_ltv_stage_adjoint",
    "rqp_ltv_condense_rate", "rqp_ltv_vectors_rate", "rqp_ltv_rate_rows", "rqp_ltv_rate_bounds",
    "rqp_ltv_adjoint_rate_workspace_bytes", "rqp_ltv_condense_adjoint_rate", "rqp_kernel_name", "rqp_destroy", "rqp_strerror",
    "rqp_last_error", "rqp_version",
)


class RqpUnavailable(RuntimeError):
    """librqp_hip.so cannot be loaded / no MI355X visible."""


class RqpError(RuntimeError):
    """A C-ABI call returned a negative rqp_error (``code``)."""
    code = 0


class Dims(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("m", ctypes.c_int32), ("batch", ctypes.c_int32),
                ("shared_mats", ctypes.c_int32), ("dtype", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("tile_dtype", ctypes.c_int32), ("flags", ctypes.c_int32)]


class CSettings(ctypes.Structure):
    _fields_ = [("rho", ctypes.c_double), ("rho_min", ctypes.c_double), ("rho_max", ctypes.c_double),
                ("sigma", ctypes.c_double), ("adaptive_rho_tolerance", ctypes.c_double),
                ("eps_abs", ctypes.c_double), ("eq_tol", ctypes.c_double),
                ("adaptive_rho", ctypes.c_int32), ("max_iter", ctypes.c_int32),
                ("check_interval", ctypes.c_int32), ("warm_starting", ctypes.c_int32),
                ("eps_rel", ctypes.c_double), ("eps_prim_inf", ctypes.c_double), ("eps_dual_inf", ctypes.c_double),
                ("scaling", ctypes.c_int32), ("check_infeasibility", ctypes.c_int32)]


class AdjointIO(ctypes.Structure):
    """struct rqp_adjoint_io: device pointers (None = NULL)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("H", "A", "l", "u", "x", "z", "y", "status", "active", "dx", "dy",
                                                "dH", "dg", "dA", "dl", "du", "active_out", "adj_status", "adj_res")]


SENS_SHARED = {"dH": 1, "dg": 2, "dA": 4, "dl": 8, "du": 16}     # RQP_SENS_SHARED_* (rqp_sensitivity_io.shared_tangents)


class SensitivityIO(ctypes.Structure):
    """struct rqp_sensitivity_io: device pointers (None = NULL), ndir and the shared-tangent bits."""
    _fields_ = ([(f, ctypes.c_void_p) for f in ("H", "A", "l", "u", "x", "z", "y", "status", "active")] +
                [("ndir", ctypes.c_int32), ("shared_tangents", ctypes.c_int32)] +
                [(f, ctypes.c_void_p) for f in ("dH", "dg", "dA", "dl", "du", "dx", "dy", "dz", "active_out", "sens_status",
                                                "sens_res")])


LTV_HAS_K, LTV_HAS_C, LTV_HAS_XREF, LTV_HAS_UREF, LTV_BOUNDS_BATCHED = 1, 2, 4, 8, 16     # RQP_LTV_* (rqp_ltv_dims.flags)
LTV_STAGE_SHARED_E = 32                                                                   # (the rqp_ltv_stage_* calls only)
LTV_STAGE_WEIGHTS = 128                                                                   # Q, R per (instance, stage); no Qf


class LtvDims(ctypes.Structure):
    """struct rqp_ltv_dims."""
    _fields_ = [(f, ctypes.c_int32) for f in ("batch", "nx", "nu", "horizon", "dtype", "flags")]


class LtvAdjointIO(ctypes.Structure):
    """struct rqp_ltv_adjoint_io: device pointers (None = NULL)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("Ad", "Bd", "c", "x0", "xref", "uref", "Q", "R", "Qf", "K", "workspace",
                                                "dH", "dA", "dg", "dl", "du", "dAd", "dBd", "dc", "dx0", "dxref", "duref",
                                                "dQ", "dR", "dQf", "adjoint_workspace")]


class LtvStageAdjointIO(ctypes.Structure):
    """struct rqp_ltv_stage_adjoint_io: device pointers (None = NULL)."""
    _fields_ = [(f, ctypes.c_void_p) for f in ("E", "x0", "workspace", "dA_c", "dl_c", "du_c", "dA_full", "dl_full", "dE")]


class LtvRateAdjointIO(ctypes.Structure):
    """struct rqp_ltv_rate_adjoint_io: device pointers (None = NULL) and the two instance strides (elements)."""
    _fields_ = ([(f, ctypes.c_void_p) for f in ("S", "uprev", "dA_r", "dl_r", "du_r")] +
                [("dA_stride", ctypes.c_int64), ("dl_stride", ctypes.c_int64)] +
                [(f, ctypes.c_void_p) for f in ("dS", "duprev")])


class CInfo(ctypes.Structure):
    _fields_ = [("iter", ctypes.c_void_p), ("status", ctypes.c_void_p), ("rho_ind", ctypes.c_void_p),
                ("pri_res", ctypes.c_void_p), ("dua_res", ctypes.c_void_p), ("rho_estimate", ctypes.c_void_p),
                ("obj_val", ctypes.c_void_p), ("trace", ctypes.c_void_p), ("trace_cap", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


_lib = None


def load():
    """Load the library once; raise RqpUnavailable if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RqpUnavailable(
            "librqp_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C reluqp-py_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    # torch ships its own libamdhip64 (SONAME libamdhip64.so.7).  It must be mapped BEFORE our
    # library so that both bind to ONE HIP runtime (streams and pointers are shared with torch);
    # loading ours first would pull a second runtime from /opt/rocm into the process.
    import torch  # noqa: F401
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise RqpUnavailable("cannot load %s: %s" % (LIB_PATH, e))
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    H = ctypes.c_void_p  # opaque handle
    sig = {
        "rqp_default_settings": (ctypes.c_int, [ctypes.POINTER(CSettings)]),
        "rqp_create": (ctypes.c_int, [ctypes.POINTER(H), ctypes.POINTER(Dims), ctypes.POINTER(CSettings), ctypes.c_int]),
        "rqp_setup": (ctypes.c_int, [H, vp, vp, vp, vp, vp, vp]),
        "rqp_update": (ctypes.c_int, [H, vp, vp, vp, vp]),
        "rqp_update_mats": (ctypes.c_int, [H, vp, vp, vp]),
        "rqp_update_affine": (ctypes.c_int, [H, vp, ctypes.c_int32, vp, vp, vp, vp, vp]),
        "rqp_update_settings": (ctypes.c_int, [H, ctypes.POINTER(CSettings)]),
        "rqp_warm_start": (ctypes.c_int, [H, vp, vp, vp, ctypes.c_int, dbl, vp]),
        "rqp_clear_primal_dual": (ctypes.c_int, [H, vp]),
        "rqp_solve": (ctypes.c_int, [H, vp, vp, vp, ctypes.POINTER(CInfo), vp]),
        "rqp_iterate": (ctypes.c_int, [H, i32, vp]),
        "rqp_compute_residuals": (ctypes.c_int, [H, dbl, vp, vp, vp, vp, vp]),
        "rqp_get_state": (ctypes.c_int, [H, vp, vp, vp, vp, vp]),
        "rqp_get_rhos": (ctypes.c_int, [H, ctypes.POINTER(dbl), i32, ctypes.POINTER(i32)]),
        "rqp_get_K": (ctypes.c_int, [H, i32, i32, vp, vp]),
        "rqp_dispatch_history": (ctypes.c_int, [H, i32]),
        "rqp_get_dispatch": (ctypes.c_int, [H, vp, vp, ctypes.POINTER(i32), vp]),
        "rqp_get_window": (ctypes.c_int, [H, ctypes.POINTER(i32), vp, vp]),
        "rqp_set_window_passes": (ctypes.c_int, [H, i32]),
        "rqp_set_polish": (ctypes.c_int, [H, i32, dbl, i32]),
        "rqp_get_polish": (ctypes.c_int, [H, vp, vp, vp]),
        "rqp_set_adjoint": (ctypes.c_int, [H, i32, dbl, i32]),
        "rqp_adjoint": (ctypes.c_int, [H, ctypes.POINTER(AdjointIO), vp]),
        "rqp_set_sensitivity": (ctypes.c_int, [H, i32]),
        "rqp_sensitivity": (ctypes.c_int, [H, ctypes.POINTER(SensitivityIO), vp]),
        "rqp_ltv_workspace_bytes": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.POINTER(ctypes.c_size_t)]),
        "rqp_ltv_condense": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int] + [vp] * 11),
        "rqp_ltv_vectors": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int] + [vp] * 13),
        "rqp_ltv_adjoint_workspace_bytes": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.POINTER(ctypes.c_size_t)]),
        "rqp_ltv_condense_adjoint": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int, ctypes.POINTER(LtvAdjointIO), vp]),
        "rqp_ltv_stage_rows": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int, i32] + [vp] * 4),
        "rqp_ltv_stage_vectors": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int, i32] + [vp] * 8),
        "rqp_ltv_stage_adjoint": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int, i32, ctypes.POINTER(LtvStageAdjointIO), vp]),
        "rqp_ltv_condense_rate": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int] + [vp] * 12),
        "rqp_ltv_vectors_rate": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int] + [vp] * 15),
        "rqp_ltv_rate_rows": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int, vp, vp, ctypes.c_int64, vp]),
        "rqp_ltv_rate_bounds": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int] + [vp] * 7 + [ctypes.c_int64, vp]),
        "rqp_ltv_adjoint_rate_workspace_bytes": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.POINTER(ctypes.c_size_t)]),
        "rqp_ltv_condense_adjoint_rate": (ctypes.c_int, [ctypes.POINTER(LtvDims), ctypes.c_int, ctypes.POINTER(LtvAdjointIO),
                                                         ctypes.POINTER(LtvRateAdjointIO), vp]),
        "rqp_kernel_name": (ctypes.c_char_p, [H]),
        "rqp_destroy": (ctypes.c_int, [H]),
        "rqp_strerror": (ctypes.c_char_p, [ctypes.c_int]),
        "rqp_last_error": (ctypes.c_char_p, [H]),
        "rqp_version": (ctypes.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(handle, rc, what, handleless=False):
    """``handleless=True`` (the rqp_ltv_* calls): the detail is the thread's last handle-less failure, rqp_last_error(NULL)."""
    if rc == 0:
        return
    lib = load()
    msg = lib.rqp_strerror(rc).decode()
    detail = lib.rqp_last_error(handle).decode() if (handle or handleless) else ""
    err = RqpError("%s failed: %s (%d)%s" % (what, msg, rc, (": " + detail) if detail else ""))
    err.code = rc
    raise err


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
