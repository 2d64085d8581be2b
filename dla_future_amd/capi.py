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
_DP = C.POINTER(C.c_double)
_D = DLAFDescriptor
_A = [_vp, _i, _i, _IP]  # a matrix in a ScaLAPACK argument list: a, ia, ja, desca


class _PerType(tuple):
    """One ctypes type per element type, in the order s, d, c, z, where a signature depends on it."""


_real = _PerType((C.c_float, C.c_double, C.c_float, C.c_double))
_weights = _PerType((WEIGHTS_FN_S, WEIGHTS_FN_D, WEIGHTS_FN_S, WEIGHTS_FN_D))


def _family(names, res, args, types="sdcz"):
    """The entries of one routine for every element type: `names` is a pattern with {t}, and with {sy} / {symmetric} for
    the sy / he and symmetric / hermitian spellings, or the names themselves where they follow no pattern."""
    if isinstance(names, str):
        names = [names.format(t=t, sy="sy" if t in "sd" else "he", symmetric="symmetric" if t in "sd" else "hermitian")
                 for t in types]

    def pick(x, k):
        return x[k] if isinstance(x, _PerType) else x

    return {name: (pick(res, k), [pick(x, k) for x in args]) for k, name in enumerate(names)}


SIGNATURES = {
    # include/dlaf_c/init.h
    "dlaf_initialize": (None, [_i, C.POINTER(C.c_char_p), _i, C.POINTER(C.c_char_p)]),
    "dlaf_finalize": (None, []),
    # include/dlaf_c/grid.h
    "dlaf_free_grid": (None, [_i]),
    # include/dlaf_c/utils.h
    "make_dlaf_descriptor": (_D, [_i, _i, _i, _i, _IP]),
    # include/dlaf_mi355x/dlaf_mi355x.h: the entries that exist once
    "dlaf_mi355x_version": (C.c_char_p, []),
    "dlaf_mi355x_create_grid_single": (_i, []),
    "dlaf_mi355x_rccl_unique_id": (None, [_vp]),
    "dlaf_mi355x_create_grid_rccl": (_i, [_vp, _i, _i, _i, _i, _ch]),
    "dlaf_mi355x_create_grid_host": (_i, [_i, _i, _i, _i, _ch, BCAST_FN, BARRIER_FN, _vp]),
    "dlaf_mi355x_grid_host_bcast": (_i, [_i, _i, _i, _vp, C.c_size_t]),
    "dlaf_mi355x_grid_info": (_i, [_i, _IP, _IP, _IP, _IP]),
    "dlaf_mi355x_grid_barrier": (_i, [_i]),
    "dlaf_mi355x_grid_selftest": (_i, [_i, C.c_size_t]),
    "dlaf_mi355x_grid_on_free": (_i, [_i, _vp, _vp]),
    "dlaf_mi355x_grid_rekey": (_i, [_i, _i]),
    "dlaf_mi355x_grid_comm_log": (_i, [_i, _i]),
    "dlaf_mi355x_grid_comm_log_read": (_l, [_i, _LP, _l]),
    "dlaf_mi355x_matrix_create": (_i, [_i, _ch, _ch, _D, C.POINTER(_vp)]),
    "dlaf_mi355x_matrix_destroy": (None, [_vp]),
    "dlaf_mi355x_matrix_upload": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_matrix_download": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_matrix_copy": (_i, [_vp, _vp]),
    "dlaf_mi355x_matrix_fetch_tile": (_i, [_vp, _l, _l, _vp, _i]),
    "dlaf_mi355x_matrix_local_info": (_i, [_vp]),
    "dlaf_mi355x_matrix_to_general": (_i, [_ch, _vp, _vp]),
    "dlaf_mi355x_matrix_from_general": (_i, [_vp, _vp]),
    "dlaf_mi355x_matrix_trsm_profile": (_i, [_vp, _i, _DP, _DP, _DP]),
    "dlaf_mi355x_matrix_profile": (_i, [_vp, _i, _DP, _LP, _DP, _DP]),
    "dlaf_mi355x_matrix_norm": (_i, [_vp, _ch, _ch, _ch, _DP]),
    "dlaf_mi355x_gmatrix_create": (_i, [_i, _ch, _D, C.POINTER(_vp)]),
    "dlaf_mi355x_gmatrix_destroy": (None, [_vp]),
    "dlaf_mi355x_gmatrix_upload": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_gmatrix_download": (_i, [_vp, _vp, _i]),
    "dlaf_mi355x_gmatrix_device_tiles": (_i, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "dlaf_mi355x_general_matrix_norm": (_i, [_vp, _ch, _DP]),
    "dlaf_mi355x_potrf_trace": (_i, [C.POINTER(C.c_ulonglong)]),
    "dlaf_mi355x_update_launch_stats": (_i, [_LP, _LP]),
    "dlaf_mi355x_workspace_pool_release": (_l, []),
    "dlaf_mi355x_set_random_hpd": (_i, [_i, _ch, _vp, _D, _i]),
    "dlaf_mi355x_cholesky_start": (_i, [_vp]),
    "dlaf_mi355x_cholesky_wait": (_i, [_vp]),
    "dlaf_mi355x_cholesky_factorization_device": (_i, [_vp]),
    "dlaf_mi355x_cholesky_residual": (_i, [_vp, _vp, _DP, _DP]),
    "dlaf_mi355x_potrs_device": (_i, [_ch, _vp, _vp]),
    "dlaf_mi355x_triangular_solver_device": (_i, [_ch, _ch, _ch, _ch, _vp, _vp, _vp]),
    "dlaf_mi355x_triangular_multiplication_device": (_i, [_ch, _ch, _ch, _ch, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_multiplication_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_general_multiplication_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_rank_k_update_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_rank_2k_update_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_weighted_rank_k_update_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_function_device": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_power_device": (_i, [_vp, _vp, C.c_double, C.c_double, _LP]),
    "dlaf_mi355x_general_addition_device": (_i, [_ch, _ch, _vp, _vp, _vp, _vp]),
    "dlaf_mi355x_hermitian_complete_device": (_i, [_ch, _ch, _vp]),
    "dlaf_mi355x_generalized_to_standard_device": (_i, [_vp, _vp]),
    "dlaf_mi355x_triangular_inverse_device": (_i, [_ch, _ch, _vp]),
    "dlaf_mi355x_inverse_from_cholesky_factor_device": (_i, [_ch, _vp]),
    "dlaf_mi355x_inverse_plan": (_i, [_l, _i, _i, _i, _i, _i, _i, _i, _LP]),
    "dlaf_mi355x_inverse_step": (_i, [_l, _i, _i, _i, _i, _i, _i, _i, _l, _LP]),
    "dlaf_mi355x_reduction_to_band_device": (_i, [_vp, _i, _vp]),
    "dlaf_mi355x_bt_reduction_to_band_device": (_i, [_i, _vp, _vp, _vp]),
    "dlaf_mi355x_solver_profile": (_i, [_DP, _DP]),
    "dlaf_mi355x_multiplication_profile": (_i, [_DP, _DP]),
    "dlaf_mi355x_addition_profile": (_i, [_DP, _DP]),
    "dlaf_mi355x_inverse_profile": (_i, [_DP, _DP]),
    "dlaf_mi355x_norm_profile": (_i, [_DP, _DP]),
    "dlaf_mi355x_red2band_profile": (_i, [_DP, _DP]),
    "dlaf_mi355x_eigensolver_profile": (_i, [_DP]),
    "dlaf_mi355x_sturm_layout": (_i, [_IP]),
    "dlaf_mi355x_partial_spectrum_plan": (_i, [_l, _i, _i, _i, _i, _l, _l, _LP]),
    "dlaf_mi355x_get_band_size": (_i, [_i]),
    "dlaf_mi355x_red2band_panel_stats": (_i, [_LP, _LP]),
    "dlaf_mi355x_get_eigensolver_min_band": (_i, []),
    "dlaf_mi355x_set_eigensolver_min_band": (None, [_i]),
    "dlaf_mi355x_tile_potrf": (_i, [_ch, _ch, _i, _vp, _i]),
    "dlaf_mi355x_tile_trsm": (_i, [_ch, _ch, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_tile_herk": (_i, [_ch, _ch, _i, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_tile_gemm": (_i, [_ch, _ch, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i]),
    "dlaf_mi355x_update_bulk_slots": (_l, [_ch]),
    "dlaf_mi355x_dist_owner": (_i, [_l, _i, _i]),
    "dlaf_mi355x_dist_local_tile": (_l, [_l, _i, _i, _i]),
    "dlaf_mi355x_dist_next_local_tile": (_l, [_l, _i, _i, _i]),
    "dlaf_mi355x_dist_global_tile": (_l, [_l, _i, _i, _i]),
    "dlaf_mi355x_dist_local_size": (_l, [_l, _i, _i, _i, _i]),
    "dlaf_mi355x_dist_local_tiles": (_l, [_l, _i, _i, _i, _i]),
}

# the entries that exist per element type, each family stated once: (names, restype, argtypes[, types])
_FAMILIES = [
    # factorization, solver, multiplication (include/dlaf_c/factorization/cholesky.h, dlaf_mi355x.h)
    ("dlaf_cholesky_factorization_{t}", _i, [_i, _ch, _vp, _D]),
    ("dlaf_p{t}potrf", None, [_ch, _i, *_A, _IP]),
    ("dlaf_mi355x_p{t}potrs", None, [_ch, _i, _i, *_A, *_A, _IP]),
    ("dlaf_mi355x_triangular_solver_{t}", _i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, _D, _vp, _D]),
    ("dlaf_mi355x_triangular_multiplication_{t}", _i, [_i, _ch, _ch, _ch, _ch, _vp, _vp, _D, _vp, _D]),
    ("dlaf_mi355x_p{t}trsm", None, [_ch, _ch, _ch, _ch, _i, _i, _vp, *_A, *_A]),
    ("dlaf_mi355x_p{t}trmm", None, [_ch, _ch, _ch, _ch, _i, _i, _vp, *_A, *_A]),
    ("dlaf_mi355x_hermitian_multiplication_{t}", _i, [_i, _ch, _ch, _vp, _vp, _D, _vp, _D, _vp, _vp, _D]),
    (["dlaf_mi355x_pssymm", "dlaf_mi355x_pdsymm", "dlaf_mi355x_pchemm", "dlaf_mi355x_pzhemm"], None,
     [_ch, _ch, _i, _i, _vp, *_A, *_A, _vp, *_A]),
    ("dlaf_mi355x_general_multiplication_{t}", _i, [_i, _ch, _ch, _vp, _vp, _D, _vp, _D, _vp, _vp, _D]),
    ("dlaf_mi355x_p{t}gemm", None, [_ch, _ch, _i, _i, _i, _vp, *_A, *_A, _vp, *_A]),
    # rank updates and matrix functions
    ("dlaf_mi355x_hermitian_rank_k_update_{t}", _i, [_i, _ch, _ch, _vp, _vp, _D, _vp, _vp, _D]),
    ("dlaf_mi355x_hermitian_rank_2k_update_{t}", _i, [_i, _ch, _ch, _vp, _vp, _D, _vp, _D, _vp, _vp, _D]),
    (["dlaf_mi355x_pssyrk", "dlaf_mi355x_pdsyrk", "dlaf_mi355x_pcherk", "dlaf_mi355x_pzherk"], None,
     [_ch, _ch, _i, _i, _vp, *_A, _vp, *_A]),
    (["dlaf_mi355x_pssyr2k", "dlaf_mi355x_pdsyr2k", "dlaf_mi355x_pcher2k", "dlaf_mi355x_pzher2k"], None,
     [_ch, _ch, _i, _i, _vp, *_A, *_A, _vp, *_A]),
    ("dlaf_mi355x_hermitian_weighted_rank_k_update_{t}", _i, [_i, _ch, _ch, _vp, _vp, _D, _vp, _vp, _vp, _D]),
    ("dlaf_mi355x_hermitian_function_{t}", _i, [_i, _ch, _vp, _D, _vp, _weights, _vp, _vp, _vp, _vp]),
    ("dlaf_mi355x_hermitian_power_{t}", _i, [_i, _ch, _vp, _D, _vp, C.c_double, C.c_double, _LP]),
    # addition, transposition, copy, completion
    ("dlaf_mi355x_general_addition_{t}", _i, [_i, _ch, _ch, _vp, _vp, _D, _vp, _vp, _D]),
    ("dlaf_mi355x_hermitian_complete_{t}", _i, [_i, _ch, _ch, _vp, _D]),
    ("dlaf_mi355x_p{t}geadd", None, [_ch, _i, _i, _vp, *_A, _vp, *_A]),
    ("dlaf_mi355x_p{t}tradd", None, [_ch, _ch, _i, _i, _vp, *_A, _vp, *_A]),
    ("dlaf_mi355x_p{t}lacpy", None, [_ch, _i, _i, *_A, *_A]),
    (["dlaf_mi355x_pstran", "dlaf_mi355x_pdtran", "dlaf_mi355x_pctranu", "dlaf_mi355x_pctranc", "dlaf_mi355x_pztranu",
      "dlaf_mi355x_pztranc"], None, [_i, _i, _vp, *_A, _vp, *_A]),
    # gen_to_std, inverses, norms
    ("dlaf_mi355x_generalized_to_standard_{t}", _i, [_i, _ch, _vp, _D, _vp, _D]),
    ("dlaf_mi355x_p{t}hegst", None, [_i, _ch, _i, *_A, *_A, _vp, _IP]),
    ("dlaf_mi355x_triangular_inverse_{t}", _i, [_i, _ch, _ch, _vp, _D]),
    ("dlaf_mi355x_inverse_from_cholesky_factor_{t}", _i, [_i, _ch, _vp, _D]),
    ("dlaf_mi355x_p{t}trtri", None, [_ch, _ch, _i, *_A, _IP]),
    ("dlaf_mi355x_p{t}potri", None, [_ch, _i, *_A, _IP]),
    ("dlaf_mi355x_general_norm_{t}", _i, [_i, _ch, _vp, _D, _DP]),
    ("dlaf_mi355x_hermitian_norm_{t}", _i, [_i, _ch, _ch, _vp, _D, _DP]),
    ("dlaf_mi355x_triangular_norm_{t}", _i, [_i, _ch, _ch, _ch, _vp, _D, _DP]),
    ("dlaf_mi355x_p{t}lange", _real, [_ch, _i, _i, *_A]),
    ("dlaf_mi355x_p{t}lan{sy}", _real, [_ch, _ch, _i, *_A]),
    ("dlaf_mi355x_p{t}lantr", _real, [_ch, _ch, _ch, _i, *_A]),
    # the eigensolver stages
    ("dlaf_mi355x_reduction_to_band_{t}", _i, [_i, _vp, _D, _i, _vp]),
    ("dlaf_mi355x_bt_reduction_to_band_{t}", _i, [_i, _i, _vp, _D, _vp, _D, _vp]),
    ("dlaf_mi355x_band_to_tridiagonal_{t}", _i, [_i, _vp, _D, _i, _vp, _vp, _vp, _i]),
    ("dlaf_mi355x_bt_band_to_tridiagonal_{t}", _i, [_i, _i, _i, _vp, _i, _vp, _i]),
    ("dlaf_mi355x_tridiagonal_eigensolver_{t}", _i, [_i, _i, _vp, _vp, _vp, _vp, _i], "sd"),
    ("dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_{t}", _i, [_i, _i, _vp, _vp, _vp, _vp, _i, _l, _l], "sd"),
    ("dlaf_mi355x_tridiagonal_eigenvalues_{t}", _i, [_i, _vp, _vp, _vp, _l, _l], "sd"),
    ("dlaf_mi355x_tridiagonal_sturm_count_{t}", _i, [_i, _vp, _vp, _l, _vp, _vp], "sd"),
    # the direct doors of the kernels
    ("dlaf_mi355x_update_direct_{t}", _i, [C.POINTER(UpdateDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    ("dlaf_mi355x_trsm_direct_{t}", _i, [C.POINTER(TrsmDesc), _vp, _vp, _vp]),
    ("dlaf_mi355x_potrf_direct_{t}", _i, [C.POINTER(PotrfDesc), _vp, _vp]),
]

# the eigensolver drivers (include/dlaf_c/eigensolver/*.h and their partial-spectrum / eigenvalues-only forms): the
# standard problem takes A, the generalized one A and B ("", "_factorized"); every driver exists in three selections
_EVD = [_vp, _D, _vp, _vp, _D]                    # a, desca, w, z, descz
_GVD = [_vp, _D, _vp, _D, _vp, _vp, _D]           # a, desca, b, descb, w, z, descz
_PEVD = [*_A, _vp, *_A]                           # a, ia, ja, desca, w, z, iz, jz, descz
_PGVD = [*_A, *_A, _vp, *_A]                      # a, ..., b, ..., w, z, ...
for _sel, _c, _p in (("", [], [_IP]), ("_partial_spectrum", [_i64, _i64], [_i64, _i64, _IP]),
                     ("_partial_spectrum_by_value", [_real, _real, _LP, _LP], [_real, _real, _IP, _IP])):
    _FAMILIES.append(("dlaf_{symmetric}_eigensolver" + _sel + "_{t}", _i, [_i, _ch, *_EVD, *_c]))
    _FAMILIES.append(("dlaf_p{t}{sy}evd" + _sel, None, [_ch, _i, *_PEVD, *_p]))
    for _fac in ("", "_factorized"):
        _FAMILIES.append(("dlaf_{symmetric}_generalized_eigensolver" + _fac + _sel + "_{t}", _i, [_i, _ch, *_GVD, *_c]))
        _FAMILIES.append(("dlaf_p{t}{sy}gvd" + _fac + _sel, None, [_ch, _i, *_PGVD, *_p]))
_FAMILIES += [
    ("dlaf_{symmetric}_eigenvalues_{t}", _i, [_i, _ch, _vp, _D, _vp, _i64, _i64]),
    ("dlaf_p{t}{sy}evd_eigenvalues", None, [_ch, _i, *_A, _vp, _i64, _i64, _IP]),
]
for _fac in ("", "_factorized"):
    _FAMILIES.append(("dlaf_{symmetric}_generalized_eigenvalues" + _fac + "_{t}", _i,
                      [_i, _ch, _vp, _D, _vp, _D, _vp, _i64, _i64]))
    _FAMILIES.append(("dlaf_p{t}{sy}gvd_eigenvalues" + _fac, None, [_ch, _i, *_A, *_A, _vp, _i64, _i64, _IP]))

for _f in _FAMILIES:
    _entries = _family(*_f)
    assert not set(_entries) & set(SIGNATURES), set(_entries) & set(SIGNATURES)  # a family stated twice
    SIGNATURES.update(_entries)

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
