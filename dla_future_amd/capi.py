"""ctypes binding of libdlaf_mi355x.so (include/dlaf_c/*.h + include/dlaf_mi355x/dlaf_mi355x.h)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class LibraryNotBuilt(RuntimeError):
    pass


def lib_path() -> str:
    # DLAF_MI355X_LIB: another build of the same library (diagnosis builds, e.g. tools/build_b2t_prof.sh)
    return os.environ.get("DLAF_MI355X_LIB") or os.path.join(_HERE, "lib", "libdlaf_mi355x.so")


class DLAFDescriptor(C.Structure):
    """struct DLAF_descriptor (include/dlaf_c/desc.h; reference desc.h:16-26)."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("mb", C.c_int), ("nb", C.c_int), ("isrc", C.c_int),
                ("jsrc", C.c_int), ("i", C.c_int), ("j", C.c_int), ("ld", C.c_int)]


class UpdateDesc(C.Structure):
    """struct dlaf_mi355x_update_desc (include/dlaf_mi355x/dlaf_mi355x.h): one launch of the grouped update kernel."""
    _fields_ = ([(n, C.c_long) for n in ("c_elems", "a_elems", "b_elems", "a2_elems", "b2_elems",
                                         "c_off", "a_off", "b_off", "a2_off", "b2_off")] +
                [("tile_layout", C.c_int), ("ltr", C.c_int), ("ltc", C.c_int),
                 ("c_tsr", C.c_long), ("c_tsc", C.c_long), ("ldc", C.c_int),
                 ("a_ts", C.c_long), ("lda", C.c_int),
                 ("b_ts", C.c_long), ("ldb", C.c_int), ("b_period", C.c_int), ("b_ts2", C.c_long), ("b_jl0", C.c_int)] +
                [(n, C.c_int) for n in ("il0", "il1", "jl0", "jl1", "nb", "K", "pr", "ri", "pc", "ci", "nt", "last_rows",
                                        "rect", "nt_c", "last_cols", "K1", "her2k", "info", "role")] +
                [("max_blocks", C.c_long), ("excl_rounds", C.c_int),
                 ("persistent", C.c_long), ("exclusive", C.c_long), ("bulk_slots", C.c_long),
                 ("second_below", C.c_int)])


class TrsmDesc(C.Structure):
    """struct dlaf_mi355x_trsm_desc (include/dlaf_mi355x/dlaf_mi355x.h): one launch of the panel TRSM."""
    _fields_ = ([(n, C.c_long) for n in ("b_elems", "l_elems", "w_elems", "b_off", "l_off", "w_off", "b_ts")] +
                [(n, C.c_int) for n in ("ldb", "il0", "il1", "pr", "ri", "nb", "nt", "last_rows", "ldl", "n", "upper",
                                        "prio", "info", "winv_source", "unit", "path", "vec", "info_out")])


class PotrfDesc(C.Structure):
    """struct dlaf_mi355x_potrf_desc (include/dlaf_mi355x/dlaf_mi355x.h): one factorization of one diagonal tile."""
    _fields_ = ([(n, C.c_long) for n in ("t_elems", "w_elems", "t_off", "w_off")] +
                [(n, C.c_int) for n in ("kb", "ld", "info", "info_base", "path", "sync_zeroed_by", "count_strips",
                                        "info_out", "t_before_changed", "w_before_changed")])


BCAST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t)
BARRIER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
# dlaf_mi355x_spectral_weights_{s,d}: (n, w, begin, end, g, user)
WEIGHTS_FN_S = C.CFUNCTYPE(None, C.c_long, C.POINTER(C.c_float), C.c_long, C.c_long, C.POINTER(C.c_float), C.c_void_p)
WEIGHTS_FN_D = C.CFUNCTYPE(None, C.c_long, C.POINTER(C.c_double), C.c_long, C.c_long, C.POINTER(C.c_double), C.c_void_p)

_TYPE_CHARS = {np.dtype(np.float32): "s", np.dtype(np.float64): "d", np.dtype(np.complex64): "c",
               np.dtype(np.complex128): "z"}


def type_char(dtype) -> str:
    try:
        return _TYPE_CHARS[np.dtype(dtype)]
    except KeyError:
        raise TypeError(f"unsupported element type {dtype}: expected float32/64 or complex64/128") from None


# every symbol the headers declare: name -> (restype, argtypes)
_vp, _i, _l, _ch = C.c_void_p, C.c_int, C.c_long, C.c_char
_IP = C.POINTER(C.c_int)
_i64 = C.c_int64
_LP = C.POINTER(C.c_long)
SIGNATURES = {
    # include/dlaf_c/init.h
    "dlaf_initialize": (None, [_i, C.POINTER(C.c_char_p), _i, C.POINTER(C.c_char_p)]),
    "dlaf_finalize": (None, []),
    # include/dlaf_c/grid.h
    "dlaf_free_grid": (None, [_i]),
    # include/dlaf_c/utils.h
    "make_dlaf_descriptor": (DLAFDescriptor, [_i, _i, _i, _i, _IP]),
    # include/dlaf_c/factorization/cholesky.h
    "dlaf_cholesky_factorization_s": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_cholesky_factorization_d": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_cholesky_factorization_c": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_cholesky_factorization_z": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_pspotrf": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_pdpotrf": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_pcpotrf": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_pzpotrf": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    # include/dlaf_mi355x/dlaf_mi355x.h
    "dlaf_mi355x_version": (C.c_char_p, []),
    "dlaf_mi355x_create_grid_single": (_i, []),
    "dlaf_mi355x_rccl_unique_id": (None, [_vp]),
    "dlaf_mi355x_create_grid_rccl": (_i, [_vp, _i, _i, _i, _i, _ch]),
    "dlaf_mi355x_create_grid_host": (_i, [_i, _i, _i, _i, _ch, BCAST_FN, BARRIER_FN, _vp]),
    "dlaf_mi355x_grid_host_bcast": (_i, [_i, _i, _i, _vp, C.c_size_t]),
    "dlaf_mi355x_grid_info": (_i, [_i, _IP, _IP, _IP, _IP]),
    "dlaf_mi355x_grid_barrier": (_i, [_i]),
    "dlaf_mi355x_grid_selftest": (_i, [_i, C.c_size_t]),
    "dlaf_mi355x_matrix_create": (_i, [_i, _ch, _ch, DLAFDescriptor, C.POINTER(_vp)]),
    "dlaf_mi355x_matrix_destroy": (None, [_vp]),
    "dlaf_mi355x_matrix_upload": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_matrix_download": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_matrix_copy": (_i, [_vp, _vp]),
    "dlaf_mi355x_matrix_fetch_tile": (_i, [_vp, _l, _l, _vp, _i]),
    "dlaf_mi355x_grid_on_free": (_i, [_i, _vp, _vp]),
    "dlaf_mi355x_grid_rekey": (_i, [_i, _i]),
    "dlaf_mi355x_grid_comm_log": (_i, [_i, _i]),
    "dlaf_mi355x_grid_comm_log_read": (_l, [_i, C.POINTER(C.c_long), _l]),
    "dlaf_mi355x_matrix_local_info": (_i, [_vp]),
    "dlaf_mi355x_potrf_trace": (_i, [C.POINTER(C.c_ulonglong)]),
    "dlaf_mi355x_update_launch_stats": (_i, [C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "dlaf_mi355x_cholesky_start": (_i, [_vp]),
    "dlaf_mi355x_cholesky_wait": (_i, [_vp]),
    "dlaf_mi355x_cholesky_factorization_device": (_i, [_vp]),
    "dlaf_mi355x_cholesky_residual": (_i, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_matrix_trsm_profile": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_matrix_profile": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_long),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_triangular_solver_s": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_triangular_solver_d": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_triangular_solver_c": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_triangular_solver_z": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_triangular_multiplication_s": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_triangular_multiplication_d": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_triangular_multiplication_c": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_triangular_multiplication_z": (_i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_pstrsm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdtrsm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pctrsm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pztrsm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pstrmm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdtrmm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pctrmm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pztrmm": (None, [_ch, _ch, _ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_hermitian_multiplication_s": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_multiplication_d": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_multiplication_c": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_multiplication_z": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_pssymm": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdsymm": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pchemm": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzhemm": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_general_multiplication_s": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_general_multiplication_d": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_general_multiplication_c": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_general_multiplication_z": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_k_update_s": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_k_update_d": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_k_update_c": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_k_update_z": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_2k_update_s": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_2k_update_d": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_2k_update_c": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_rank_2k_update_z": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_weighted_rank_k_update_s": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_weighted_rank_k_update_d": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_weighted_rank_k_update_c": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_weighted_rank_k_update_z": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_weighted_rank_k_update_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_function_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, WEIGHTS_FN_S, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_function_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, WEIGHTS_FN_D, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_function_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, WEIGHTS_FN_S, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_function_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, WEIGHTS_FN_D, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_function_device": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_power_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, C.c_double, C.c_double, _LP]),
    "dlaf_mi355x_hermitian_power_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, C.c_double, C.c_double, _LP]),
    "dlaf_mi355x_hermitian_power_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, C.c_double, C.c_double, _LP]),
    "dlaf_mi355x_hermitian_power_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, C.c_double, C.c_double, _LP]),
    "dlaf_mi355x_hermitian_power_device": (_i, [_vp, _vp, C.c_double, C.c_double, _LP]),
    "dlaf_mi355x_pssyrk": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdsyrk": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pcherk": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzherk": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pssyr2k": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdsyr2k": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pcher2k": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzher2k": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_general_addition_s": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_general_addition_d": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_general_addition_c": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_general_addition_z": (_i, [_i, _ch, _ch, _vp, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_complete_s": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_complete_d": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_complete_c": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_hermitian_complete_z": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_psgeadd": (None, [_ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pstradd": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pslacpy": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdgeadd": (None, [_ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdtradd": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdlacpy": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pcgeadd": (None, [_ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pctradd": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pclacpy": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzgeadd": (None, [_ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pztradd": (None, [_ch, _ch, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzlacpy": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pstran": (None, [_i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdtran": (None, [_i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pctranu": (None, [_i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pctranc": (None, [_i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pztranu": (None, [_i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pztranc": (None, [_i, _i, _vp, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_psgemm": (None, [_ch, _ch, _i, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdgemm": (None, [_ch, _ch, _i, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pcgemm": (None, [_ch, _ch, _i, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzgemm": (None, [_ch, _ch, _i, _i, _i, _vp, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pspotrs": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_pdpotrs": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_pcpotrs": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_pzpotrs": (None, [_ch, _i, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_solver_profile": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_multiplication_profile": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_addition_profile": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_gmatrix_create": (_i, [_i, _ch, DLAFDescriptor, C.POINTER(_vp)]),
    "dlaf_mi355x_gmatrix_destroy": (None, [_vp]),
    "dlaf_mi355x_gmatrix_upload": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_gmatrix_download": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_triangular_solver_device": (_i, [_ch, _ch, _ch, _ch, _vp, _vp, _vp]),
    "dlaf_mi355x_triangular_multiplication_device": (_i, [_ch, _ch, _ch, _ch, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_multiplication_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_general_multiplication_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_rank_k_update_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_rank_2k_update_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_general_addition_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_complete_device": (_i, [_ch, _ch, _vp]),
    "dlaf_mi355x_matrix_to_general": (_i, [_ch, _vp, _vp]),
    "dlaf_mi355x_matrix_from_general": (_i, [_vp, _vp]),
    "dlaf_mi355x_potrs_device": (_i, [_ch, _vp, _vp]),
    "dlaf_mi355x_generalized_to_standard_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_generalized_to_standard_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_generalized_to_standard_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_generalized_to_standard_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor]),
    "dlaf_mi355x_pshegst": (None, [_i, _ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _IP]),
    "dlaf_mi355x_pdhegst": (None, [_i, _ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _IP]),
    "dlaf_mi355x_pchegst": (None, [_i, _ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _IP]),
    "dlaf_mi355x_pzhegst": (None, [_i, _ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _IP]),
    "dlaf_mi355x_generalized_to_standard_device": (_i, [_vp, _vp]),
    "dlaf_mi355x_triangular_inverse_s": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_inverse_from_cholesky_factor_s": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_pstrtri": (None, [_ch, _ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_pspotri": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_triangular_inverse_d": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_inverse_from_cholesky_factor_d": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_pdtrtri": (None, [_ch, _ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_pdpotri": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_triangular_inverse_c": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_inverse_from_cholesky_factor_c": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_pctrtri": (None, [_ch, _ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_pcpotri": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_triangular_inverse_z": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_inverse_from_cholesky_factor_z": (_i, [_i, _ch, _vp, DLAFDescriptor]),
    "dlaf_mi355x_pztrtri": (None, [_ch, _ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_pzpotri": (None, [_ch, _i, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_triangular_inverse_device": (_i, [_ch, _ch, _vp]),
    "dlaf_mi355x_inverse_from_cholesky_factor_device": (_i, [_ch, _vp]),
    "dlaf_mi355x_inverse_profile": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_inverse_plan": (_i, [C.c_long, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_long)]),
    "dlaf_mi355x_inverse_step": (_i, [C.c_long, _i, _i, _i, _i, _i, _i, _i, C.c_long, C.POINTER(C.c_long)]),
    "dlaf_mi355x_general_norm_s": (_i, [_i, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_hermitian_norm_s": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_triangular_norm_s": (_i, [_i, _ch, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_pslange": (C.c_float, [_ch, _i, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pslansy": (C.c_float, [_ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pslantr": (C.c_float, [_ch, _ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_general_norm_d": (_i, [_i, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_hermitian_norm_d": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_triangular_norm_d": (_i, [_i, _ch, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_pdlange": (C.c_double, [_ch, _i, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdlansy": (C.c_double, [_ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pdlantr": (C.c_double, [_ch, _ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_general_norm_c": (_i, [_i, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_hermitian_norm_c": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_triangular_norm_c": (_i, [_i, _ch, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_pclange": (C.c_float, [_ch, _i, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pclanhe": (C.c_float, [_ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pclantr": (C.c_float, [_ch, _ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_general_norm_z": (_i, [_i, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_hermitian_norm_z": (_i, [_i, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_triangular_norm_z": (_i, [_i, _ch, _ch, _ch, _vp, DLAFDescriptor, C.POINTER(C.c_double)]),
    "dlaf_mi355x_pzlange": (C.c_double, [_ch, _i, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzlanhe": (C.c_double, [_ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_pzlantr": (C.c_double, [_ch, _ch, _ch, _i, _vp, _i, _i, _IP]),
    "dlaf_mi355x_matrix_norm": (_i, [_vp, _ch, _ch, _ch, C.POINTER(C.c_double)]),
    "dlaf_mi355x_general_matrix_norm": (_i, [_vp, _ch, C.POINTER(C.c_double)]),
    "dlaf_mi355x_gmatrix_device_tiles": (_i, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "dlaf_mi355x_norm_profile": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_reduction_to_band_s": (_i, [_i, _vp, DLAFDescriptor, _i, _vp]),
    "dlaf_mi355x_reduction_to_band_d": (_i, [_i, _vp, DLAFDescriptor, _i, _vp]),
    "dlaf_mi355x_reduction_to_band_c": (_i, [_i, _vp, DLAFDescriptor, _i, _vp]),
    "dlaf_mi355x_reduction_to_band_z": (_i, [_i, _vp, DLAFDescriptor, _i, _vp]),
    "dlaf_mi355x_reduction_to_band_device": (_i, [_vp, _i, _vp]),
    "dlaf_mi355x_bt_reduction_to_band_s": (_i, [_i, _i, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp]),
    "dlaf_mi355x_bt_reduction_to_band_d": (_i, [_i, _i, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp]),
    "dlaf_mi355x_bt_reduction_to_band_c": (_i, [_i, _i, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp]),
    "dlaf_mi355x_bt_reduction_to_band_z": (_i, [_i, _i, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp]),
    "dlaf_mi355x_bt_reduction_to_band_device": (_i, [_i, _vp, _vp, _vp]),
    "dlaf_mi355x_band_to_tridiagonal_s": (_i, [_i, _vp, DLAFDescriptor, _i, _vp, _vp, _vp, _i]),
    "dlaf_mi355x_bt_band_to_tridiagonal_s": (_i, [_i, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_band_to_tridiagonal_d": (_i, [_i, _vp, DLAFDescriptor, _i, _vp, _vp, _vp, _i]),
    "dlaf_mi355x_bt_band_to_tridiagonal_d": (_i, [_i, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_band_to_tridiagonal_c": (_i, [_i, _vp, DLAFDescriptor, _i, _vp, _vp, _vp, _i]),
    "dlaf_mi355x_bt_band_to_tridiagonal_c": (_i, [_i, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_band_to_tridiagonal_z": (_i, [_i, _vp, DLAFDescriptor, _i, _vp, _vp, _vp, _i]),
    "dlaf_mi355x_bt_band_to_tridiagonal_z": (_i, [_i, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_symmetric_eigensolver_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_symmetric_generalized_eigensolver_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_symmetric_generalized_eigensolver_factorized_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_symmetric_eigensolver_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_symmetric_generalized_eigensolver_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_symmetric_generalized_eigensolver_factorized_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_hermitian_eigensolver_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_hermitian_generalized_eigensolver_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_hermitian_generalized_eigensolver_factorized_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_hermitian_eigensolver_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_hermitian_generalized_eigensolver_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_hermitian_generalized_eigensolver_factorized_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor]),
    "dlaf_pssyevd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pdsyevd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pcheevd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pzheevd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pssygvd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pssygvd_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pdsygvd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pdsygvd_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pchegvd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pchegvd_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pzhegvd": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_pzhegvd_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _IP]),
    "dlaf_mi355x_tridiagonal_eigensolver_s": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i]),
    "dlaf_mi355x_tridiagonal_eigensolver_d": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i]),
    "dlaf_symmetric_eigensolver_partial_spectrum_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_symmetric_generalized_eigensolver_partial_spectrum_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_symmetric_eigensolver_partial_spectrum_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_symmetric_generalized_eigensolver_partial_spectrum_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_hermitian_eigensolver_partial_spectrum_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_hermitian_generalized_eigensolver_partial_spectrum_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_hermitian_eigensolver_partial_spectrum_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_hermitian_generalized_eigensolver_partial_spectrum_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, _i64, _i64]),
    "dlaf_pssyevd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pdsyevd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pcheevd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pzheevd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pssygvd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pssygvd_factorized_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pdsygvd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pdsygvd_factorized_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pchegvd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pchegvd_factorized_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pzhegvd_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_pzhegvd_factorized_partial_spectrum": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, _i64, _i64, _IP]),
    "dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_s": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _l, _l]),
    "dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_d": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _l, _l]),
    "dlaf_symmetric_eigenvalues_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_symmetric_generalized_eigenvalues_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_symmetric_generalized_eigenvalues_factorized_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_symmetric_eigensolver_partial_spectrum_by_value_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_float, C.c_float, _LP, _LP]),
    "dlaf_symmetric_generalized_eigensolver_partial_spectrum_by_value_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_float, C.c_float, _LP, _LP]),
    "dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_by_value_s": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_float, C.c_float, _LP, _LP]),
    "dlaf_pssyevd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pssygvd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pssygvd_eigenvalues_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pssyevd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_float, C.c_float, _IP, _IP]),
    "dlaf_pssygvd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_float, C.c_float, _IP, _IP]),
    "dlaf_pssygvd_factorized_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_float, C.c_float, _IP, _IP]),
    "dlaf_symmetric_eigenvalues_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_symmetric_generalized_eigenvalues_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_symmetric_generalized_eigenvalues_factorized_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_symmetric_eigensolver_partial_spectrum_by_value_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_double, C.c_double, _LP, _LP]),
    "dlaf_symmetric_generalized_eigensolver_partial_spectrum_by_value_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_double, C.c_double, _LP, _LP]),
    "dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_by_value_d": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_double, C.c_double, _LP, _LP]),
    "dlaf_pdsyevd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pdsygvd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pdsygvd_eigenvalues_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pdsyevd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_double, C.c_double, _IP, _IP]),
    "dlaf_pdsygvd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_double, C.c_double, _IP, _IP]),
    "dlaf_pdsygvd_factorized_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_double, C.c_double, _IP, _IP]),
    "dlaf_hermitian_eigenvalues_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_hermitian_generalized_eigenvalues_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_hermitian_generalized_eigenvalues_factorized_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_hermitian_eigensolver_partial_spectrum_by_value_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_float, C.c_float, _LP, _LP]),
    "dlaf_hermitian_generalized_eigensolver_partial_spectrum_by_value_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_float, C.c_float, _LP, _LP]),
    "dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_by_value_c": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_float, C.c_float, _LP, _LP]),
    "dlaf_pcheevd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pchegvd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pchegvd_eigenvalues_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pcheevd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_float, C.c_float, _IP, _IP]),
    "dlaf_pchegvd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_float, C.c_float, _IP, _IP]),
    "dlaf_pchegvd_factorized_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_float, C.c_float, _IP, _IP]),
    "dlaf_hermitian_eigenvalues_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_hermitian_generalized_eigenvalues_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_hermitian_generalized_eigenvalues_factorized_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _i64, _i64]),
    "dlaf_hermitian_eigensolver_partial_spectrum_by_value_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_double, C.c_double, _LP, _LP]),
    "dlaf_hermitian_generalized_eigensolver_partial_spectrum_by_value_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_double, C.c_double, _LP, _LP]),
    "dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_by_value_z": (_i, [_i, _ch, _vp, DLAFDescriptor, _vp, DLAFDescriptor, _vp, _vp, DLAFDescriptor, C.c_double, C.c_double, _LP, _LP]),
    "dlaf_pzheevd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pzhegvd_eigenvalues": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pzhegvd_eigenvalues_factorized": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _i64, _i64, _IP]),
    "dlaf_pzheevd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_double, C.c_double, _IP, _IP]),
    "dlaf_pzhegvd_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_double, C.c_double, _IP, _IP]),
    "dlaf_pzhegvd_factorized_partial_spectrum_by_value": (None, [_ch, _i, _vp, _i, _i, _IP, _vp, _i, _i, _IP, _vp, _vp, _i, _i, _IP, C.c_double, C.c_double, _IP, _IP]),
    "dlaf_mi355x_tridiagonal_eigenvalues_s": (_i, [_i, _vp, _vp, _vp, _l, _l]),
    "dlaf_mi355x_tridiagonal_sturm_count_s": (_i, [_i, _vp, _vp, _l, _vp, _vp]),
    "dlaf_mi355x_tridiagonal_eigenvalues_d": (_i, [_i, _vp, _vp, _vp, _l, _l]),
    "dlaf_mi355x_tridiagonal_sturm_count_d": (_i, [_i, _vp, _vp, _l, _vp, _vp]),
    "dlaf_mi355x_sturm_layout": (_i, [_IP]),
    "dlaf_mi355x_partial_spectrum_plan": (_i, [_l, _i, _i, _i, _i, _l, _l, C.POINTER(C.c_long)]),
    "dlaf_mi355x_eigensolver_profile": (_i, [C.POINTER(C.c_double)]),
    "dlaf_mi355x_get_band_size": (_i, [_i]),
    "dlaf_mi355x_red2band_panel_stats": (_i, [C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "dlaf_mi355x_workspace_pool_release": (C.c_long, []),
    "dlaf_mi355x_get_eigensolver_min_band": (_i, []),
    "dlaf_mi355x_set_eigensolver_min_band": (None, [_i]),
    "dlaf_mi355x_red2band_profile": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dlaf_mi355x_set_random_hpd": (_i, [_i, _ch, _vp, DLAFDescriptor, _i]),
    "dlaf_mi355x_tile_potrf": (_i, [_ch, _ch, _i, _vp, _i]),
    "dlaf_mi355x_tile_trsm": (_i, [_ch, _ch, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_tile_herk": (_i, [_ch, _ch, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_tile_gemm": (_i, [_ch, _ch, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_update_direct_s": (_i, [C.POINTER(UpdateDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_update_direct_d": (_i, [C.POINTER(UpdateDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_update_direct_c": (_i, [C.POINTER(UpdateDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_update_direct_z": (_i, [C.POINTER(UpdateDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_update_bulk_slots": (_l, [_ch]),
    "dlaf_mi355x_trsm_direct_s": (_i, [C.POINTER(TrsmDesc), _vp, _vp, _vp]),
    "dlaf_mi355x_trsm_direct_d": (_i, [C.POINTER(TrsmDesc), _vp, _vp, _vp]),
    "dlaf_mi355x_trsm_direct_c": (_i, [C.POINTER(TrsmDesc), _vp, _vp, _vp]),
    "dlaf_mi355x_trsm_direct_z": (_i, [C.POINTER(TrsmDesc), _vp, _vp, _vp]),
    "dlaf_mi355x_potrf_direct_s": (_i, [C.POINTER(PotrfDesc), _vp, _vp]),
    "dlaf_mi355x_potrf_direct_d": (_i, [C.POINTER(PotrfDesc), _vp, _vp]),
    "dlaf_mi355x_potrf_direct_c": (_i, [C.POINTER(PotrfDesc), _vp, _vp]),
    "dlaf_mi355x_potrf_direct_z": (_i, [C.POINTER(PotrfDesc), _vp, _vp]),
    "dlaf_mi355x_dist_owner": (_i, [_l, _i, _i]),
    "dlaf_mi355x_dist_local_tile": (_l, [_l, _i, _i, _i]),
    "dlaf_mi355x_dist_next_local_tile": (_l, [_l, _i, _i, _i]),
    "dlaf_mi355x_dist_global_tile": (_l, [_l, _i, _i, _i]),
    "dlaf_mi355x_dist_local_size": (_l, [_l, _i, _i, _i, _i]),
    "dlaf_mi355x_dist_local_tiles": (_l, [_l, _i, _i, _i, _i]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libdlaf_mi355x.so and type every entry point.  Raises LibraryNotBuilt when the HIP
    library is missing: there is deliberately no other implementation to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64 / librccl (same SONAMEs as /opt/rocm's).  Two copies in one
    # process abort at exit, so when torch is installed it must be loaded FIRST: our library then binds
    # to the runtime torch brought in.  DLAF_MI355X_NO_TORCH=1 skips this (pure C / numpy users).
    if os.environ.get("DLAF_MI355X_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = lib_path()
    if not os.path.exists(path):
        raise LibraryNotBuilt(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); dla_future_amd has no CPU fallback")
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        f = getattr(L, name)  # AttributeError here = header/library drift, which must be loud
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def version() -> str:
    return lib().dlaf_mi355x_version().decode()
