"""ctypes binding of the C ABI declared in include/ttcr_amd.h (libttcr_amd.so).

This is the stub a ttcrpy maintainer would mirror in Cython.  The library
is the product: if it is missing or has no HIP device, calls fail loudly -- there is no CPU
or oracle fallback anywhere in this package.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTCR_AMD_LIB") or os.path.join(HERE, "libttcr_amd.so")  # override: tuning builds only

TTCR_F32, TTCR_F64 = 0, 1
OK, ERR_VALUE, ERR_RUNTIME, ERR_DEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4

# every symbol include/ttcr_amd.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_U32 = C.c_uint32
_D = C.c_double
_I = C.c_int


class Timing(C.Structure):
    _fields_ = [("sweep_ms", C.c_double), ("total_ms", C.c_double), ("kernel_launches", C.c_longlong),
                ("node_updates", C.c_longlong), ("evaluated_updates", C.c_longlong), ("iterations", C.c_int),
                ("n_sources", C.c_int)]


SYMBOLS = {
    "ttcr_fsm_device_count": (_I, []),
    "ttcr_fsm_last_error": (C.c_char_p, []),
    "ttcr_fsm3d_create": (_I, [C.POINTER(_P), _I, _I, _U32, _U32, _U32, _D, _D, _D, _D, _D, _I, _I, _I, _I, _I]),
    "ttcr_fsm2d_create": (_I, [C.POINTER(_P), _I, _I, _U32, _U32, _D, _D, _D, _D, _D, _I, _I, _I, _I, _I]),
    "ttcr_fsm3d_create_multi": (_I, [C.POINTER(_P), _I, _I, _U32, _U32, _U32, _D, _D, _D, _D, _D, _I, _I, _I, _I, C.POINTER(_I), _I]),
    "ttcr_fsm2d_create_multi": (_I, [C.POINTER(_P), _I, _I, _U32, _U32, _D, _D, _D, _D, _D, _I, _I, _I, _I, C.POINTER(_I), _I]),
    "ttcr_fsm_n_devices": (_I, [_P]),
    "ttcr_fsm_destroy": (None, [_P]),
    "ttcr_fsm_set_slowness": (_I, [_P, _P, C.c_size_t]),
    "ttcr_fsm_set_slowness_device": (_I, [_P, _P, C.c_size_t]),
    "ttcr_fsm_set_slowness_c_order": (_I, [_P, _P, C.c_size_t]),
    "ttcr_fsm_get_slowness": (_I, [_P, _P, C.c_size_t]),
    "ttcr_fsm_raytrace": (_I, [_P, _I, _I, _P, _P, _I, _P, _P]),
    "ttcr_fsm_raytrace_multi": (_I, [_P, _I, _P, _P, _P, _P, _P, _P]),
    "ttcr_fsm_get_tt": (_I, [_P, _I, _P, C.c_size_t]),
    "ttcr_fsm_get_tt_device": (_I, [_P, _I, C.POINTER(_P)]),
    "ttcr_fsm_get_tt_device_view": (_I, [_P, _I, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_interp": (_I, [_P, _I, _I, _P, _P]),
    "ttcr_fsm_compute_slowness": (_I, [_P, _I, _P, _I, _P]),
    "ttcr_fsm_get_niter": (_I, [_P, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_get_changes": (_I, [_P, _I, C.POINTER(_D), _I, C.POINTER(_D), _I]),
    "ttcr_fsm_get_reference_changes": (_I, [_P, _I, C.POINTER(_D), _I, C.POINTER(_D), _I]),
    "ttcr_fsm_n_slots": (_I, [_P]),
    "ttcr_fsm_n_nodes": (C.c_size_t, [_P]),
    "ttcr_fsm_n_cells": (C.c_size_t, [_P]),
    "ttcr_fsm_set_option": (_I, [_P, C.c_char_p, _D]),
    "ttcr_fsm_last_timing": (_I, [_P, C.POINTER(Timing)]),
    "ttcr_fsm_last_kernel": (_I, [_P, C.c_char_p, C.c_size_t]),
    "ttcr_fsm_build_id": (C.c_char_p, []),
    "ttcr_fsm_unit_order": (_I, [_I, _I, _I, _I, _U32, _U32, _U32, C.POINTER(_U32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "ttcr_fsm_sweep_plan": (_I, [_I, _I, _I, _U32, _U32, _U32, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_double), _I, _I, _I, _I, _I, C.c_char_p, C.c_size_t,
                                 C.POINTER(C.c_longlong)]),
    "ttcr_fsm_stopping_stats": (_I, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "ttcr_fsm_prefill_swaps": (_I, [_P, C.POINTER(C.c_longlong)]),
    "ttcr_fsm_prefill_inline_fills": (_I, [_P, C.POINTER(C.c_longlong)]),
    "ttcr_fsm_chunk_dirty_marks": (_I, [_I, _I, _I, _I, _U32, _U32, _U32, C.POINTER(C.c_int32), C.c_size_t]),
    "ttcr_fsm_prefill_slice": (_I, [_I, C.c_uint64, _U32, _U32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ttcr_fsm_reference_change": (_I, [_P, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ttcr_fsm_rays_size": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_get_rays": (_I, [_P, _P, _P]),
    "ttcr_fsm_raytrace_rays": (_I, [_P, _I, _I, _P, _P, _I, _P, _P]),
    "ttcr_fsm_slot_rays_size": (_I, [_P, _I, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_get_slot_rays": (_I, [_P, _I, _P, _P]),
    "ttcr_fsm_raytrace_m": (_I, [_P, _I, _I, _P, _P, _I, _P, _P]),
    "ttcr_fsm_raytrace_rm": (_I, [_P, _I, _I, _P, _P, _I, _P, _P]),
    "ttcr_fsm_raytrace_multi_m": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I]),
    "ttcr_fsm_multi_m_size": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_get_multi_m": (_I, [_P, _P, _P, _P]),
    "ttcr_fsm_raytrace_multi_tape": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, C.POINTER(_P)]),
    "ttcr_fsm_tape_size": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_tape_bytes": (_I, [_P, C.POINTER(C.c_size_t)]),
    "ttcr_fsm_tape_device": (_I, [_P, C.POINTER(_I)]),
    "ttcr_fsm_tape_get_csr": (_I, [_P, _P, _P, _P]),
    "ttcr_fsm_tape_vjp": (_I, [_P, _P, _I, _P, _I]),
    "ttcr_fsm_tape_free": (_I, [_P]),
    "ttcr_fsm_raytrace_multi_adjoint": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, C.POINTER(_P)]),
    "ttcr_fsm_raytrace_multi_adjoint_cells": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, C.POINTER(_P)]),
    "ttcr_fsm_adjoint_model": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_model_raytrace_multi_adjoint": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, C.POINTER(_P), C.POINTER(_I)]),
    "ttcr_fsm_model_shape": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_model_tape_prolong": (_I, [_P, _P, _I, _P, _I]),
    "ttcr_fsm_model_tape_restrict": (_I, [_P, _P, _I, _P, _I]),
    "ttcr_fsm_model_device": (_I, [_P, C.POINTER(_I)]),
    "ttcr_fsm_model_prolong": (_I, [_P, C.POINTER(_I), _P, _I, _P, _I]),
    "ttcr_fsm_model_restrict": (_I, [_P, C.POINTER(_I), _P, _I, _P, _I]),
    "ttcr_fsm_adjoint_size": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_adjoint_bytes": (_I, [_P, C.POINTER(C.c_size_t)]),
    "ttcr_fsm_adjoint_device": (_I, [_P, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_get_field": (_I, [_P, C.c_size_t, _P]),
    "ttcr_fsm_adjoint_vjp": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_jvp": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_gn": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_adjoint_points": (_I, [_P, C.POINTER(C.c_size_t), _P]),
    "ttcr_fsm_adjoint_jvp_source": (_I, [_P, _P, _I, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_vjp_source": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_hold": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_release": (_I, [_P]),
    "ttcr_fsm_adjoint_hvp": (_I, [_P, _P, _I, _P, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_adjoint_newton": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_adjoint_jvp_block": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_vjp_block": (_I, [_P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_adjoint_gn_block": (_I, [_P, _I, _P, _I, _P, _I, _I, _P, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_adjoint_block_release": (_I, [_P]),
    "ttcr_fsm_adjoint_free": (_I, [_P]),
    "ttcr_fsm_normal_tile_edge": (_I, [_I]),
    "ttcr_fsm_normal_smooth": (_I, [_P, _P, _I, C.POINTER(_D), _P, _I]),
    "ttcr_fsm_normal_dot": (_I, [_P, _P, _I, _P, _I, C.POINTER(_D)]),
    "ttcr_fsm_normal_solve": (_I, [_P, _P, _I, _P, _I, _D, C.POINTER(_D), _D, _P, _I, _I, _D, _I, _I, _P, _I, C.POINTER(_I),
                                   C.POINTER(_I), C.POINTER(_D), C.POINTER(_D), C.POINTER(_I)]),
    "ttcr_fsm_normal_release": (_I, [_P]),
    "ttcr_fsm_joint_jvp": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_joint_gn": (_I, [_P, _P, _I, _P, _I, _P, _I, C.POINTER(_D), _P, _I, _P, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_joint_solve": (_I, [_P, _P, _I, _P, _I, _P, _I, _D, C.POINTER(_D), _D, C.POINTER(_D), C.POINTER(_D), _I, _D, _I, _P, _I, _P, _I,
                                  C.POINTER(_I), C.POINTER(_I), C.POINTER(_D), C.POINTER(_D), C.POINTER(_I)]),
    "ttcr_fsm_joint_release": (_I, [_P]),
    "ttcr_fsm_rcv_eval": (_I, [_P, C.c_size_t, _P, _I, C.POINTER(_I), _P, _I, _P, _I]),
    "ttcr_fsm_rcv_points": (_I, [_P, C.POINTER(_I), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_rcv_jvp": (_I, [_P, _P, _I, _P, _I]),
    "ttcr_fsm_rcv_vjp": (_I, [_P, _P, _I, _P, _I]),
    "ttcr_fsm_rjoint_jvp": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _I, C.POINTER(_I)]),
    "ttcr_fsm_rjoint_gn": (_I, [_P, _P, _I, _P, _I, _P, _I, C.POINTER(_D), _P, _I, _P, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_rjoint_solve": (_I, [_P, _P, _I, _P, _I, _P, _I, _D, C.POINTER(_D), _D, C.POINTER(_D), C.POINTER(_D), _I, _D, _I, _P, _I, _P, _I,
                                   C.POINTER(_I), C.POINTER(_I), C.POINTER(_D), C.POINTER(_D), C.POINTER(_I)]),
    "ttcr_fsm_rcv_release": (_I, [_P]),
    "ttcr_fsm_reloc_move": (_I, [_P, _P, _I, _P, _I]),
    "ttcr_fsm_reloc_get_points": (_I, [_P, C.POINTER(_D)]),
    "ttcr_fsm_reloc_gn": (_I, [_P, _P, _I, _P, _I, _P, _I, C.POINTER(_D), _P, _I]),
    "ttcr_fsm_reloc_solve": (_I, [_P, _P, _I, _P, _I, _P, _I, C.POINTER(_D), C.POINTER(_D), _I, _D, _P, _I, C.POINTER(_I), C.POINTER(_I),
                                  C.POINTER(_D), C.POINTER(_D)]),
    "ttcr_fsm_loc_geometry": (_I, [_P, C.POINTER(_I), C.POINTER(_D), C.POINTER(_D)]),
    "ttcr_fsm_loc_shape": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_loc_grid": (_I, [_P, C.c_size_t, C.POINTER(C.c_longlong), C.POINTER(_I), C.POINTER(_D), C.POINTER(_D), C.POINTER(_I),
                               C.POINTER(C.c_longlong), C.POINTER(_D), C.POINTER(_D), _P, _I]),
    "ttcr_fsm_loc_release": (_I, [_P]),
    "ttcr_fsm_dd_pairs": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_I), C.POINTER(_I),
                               C.POINTER(C.c_longlong)]),
    "ttcr_fsm_dd_apply": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P, _I]),
    "ttcr_fsm_dd_gn": (_I, [_P, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, C.POINTER(_D), _P, _I, _P, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "ttcr_fsm_dd_solve": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _D, C.POINTER(_D), _D, C.POINTER(_D), C.POINTER(_D), _P, _I, _I, _D, _I,
                               _I, _P, _I, _P, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_D), C.POINTER(_D), C.POINTER(_I)]),
    "ttcr_fsm_dd_release": (_I, [_P]),
    "ttcr_fsm_raytrace_multi_l": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I]),
    "ttcr_fsm_multi_l_size": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_get_multi_l": (_I, [_P, _P, _P, _P]),
    "ttcr_fsm_slot_m_size": (_I, [_P, _I, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_get_slot_m": (_I, [_P, _I, _P, _P, _P]),
    "ttcr_fsm_raytrace_l": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _I]),
    "ttcr_fsm_slot_l_size": (_I, [_P, _I, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ttcr_fsm_get_slot_l": (_I, [_P, _I, _P, _P, _P]),
}

_lib = None


def load():
    """Load libttcr_amd.so (built in-tree by ttcr_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -m ttcr_amd.build). "
                "ttcr_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
            fn.restype = res
            fn.argtypes = args
        # build provenance: the library in the tree must have been compiled from the sources in the tree (a tuning build named by
        # TTCR_AMD_LIB is exempt: it is never what the tests, smoke() or bench.py measure without saying so)
        if not os.environ.get("TTCR_AMD_LIB"):
            from . import build as _b

            have, want = lib.ttcr_fsm_build_id().decode(), _b.source_hash()
            if have != want:
                raise ImportError(f"{LIB_PATH} was built from other sources (build id {have}, the sources here hash to {want}): "
                                  "rebuild it (python -m ttcr_amd.build)")
        _lib = lib
    return _lib


def build_id():
    """16-hex-digit hash of the kernel sources + compiler flags the loaded library was compiled from (ttcr_fsm_build_id)."""
    return load().ttcr_fsm_build_id().decode()


def last_error():
    return load().ttcr_fsm_last_error().decode(errors="replace")


class UnsupportedError(NotImplementedError):
    pass


class DeviceError(RuntimeError):
    pass


def check(status):
    """Map a C status to the exception the reference's Python layer would raise."""
    if status == OK:
        return
    msg = last_error()
    if status == ERR_VALUE:
        raise ValueError(msg)
    if status == ERR_UNSUPPORTED:
        raise UnsupportedError(msg)
    if status == ERR_DEVICE:
        raise DeviceError(msg)
    raise RuntimeError(msg)  # std::runtime_error / length_error / logic_error via Cython `except +`
