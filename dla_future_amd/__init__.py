"""dla_future_amd -- MI355X-native tiled distributed Cholesky behind the DLA-Future interface.

The product is the C-ABI shared library ``dla_future_amd/lib/libdlaf_mi355x.so`` (hand-written
gfx950 HIP kernels + a thin C++ host over HIP streams/events and RCCL).  This package is the
Python doorway onto that ABI, mirroring the reference's operator surface for the path:

    dlaf_initialize / dlaf_finalize                    include/dlaf_c/init.h
    dlaf_create_grid* / dlaf_free_grid                 include/dlaf_c/grid.h
    dlaf_cholesky_factorization_{s,d,c,z}              include/dlaf_c/factorization/cholesky.h:32-47
    dlaf_p{s,d,c,z}potrf                               include/dlaf_c/factorization/cholesky.h:74-87
    dlaf::cholesky_factorization(uplo, Matrix&)        include/dlaf/factorization/cholesky.h:39-79
    dlaf::triangular_solver(side, uplo, op, diag, ...)  include/dlaf/solver/triangular.h:41-177 (next row)
    dlaf::triangular_multiplication(side, uplo, ...)   include/dlaf/multiplication/triangular.h
    dlaf::hermitian_multiplication(side, uplo, ...)    include/dlaf/multiplication/hermitian.h
    dlaf::multiplication::internal::generalMatrix(...) include/dlaf/multiplication/general.h (p?gemm)
    hermitian_rank_k_update / hermitian_rank_2k_update BLAS xSYRK / xHERK, xSYR2K / xHER2K (p?syrk, p?herk, p?syr2k, p?her2k)
    hermitian_weighted_rank_k_update                   "xHERK with weights": C = alpha A D A^H + beta C, D a real diagonal
    hermitian_function / hermitian_power               f(A) = Z f(W) Z^H of a Hermitian matrix (S^(-1/2), projectors, ...)
    general_addition / hermitian_complete              PBLAS p?geadd, p?tradd, p?tran / p?tranu / p?tranc, ScaLAPACK p?lacpy
    dlaf::triangular_inverse(uplo, diag, A)            LAPACK xTRTRI / p?trtri (upstream: after the reference snapshot)
    dlaf::inverse_from_cholesky_factor(uplo, A)        LAPACK xPOTRI / p?potri
    dlaf::auxiliary::max_norm(grid, rank, uplo, A)     include/dlaf/auxiliary/norm.h (+ one / inf / Frobenius: p?lange, p?lanhe, p?lantr)
    generalized_to_standard(grid, uplo, A, B)          include/dlaf/eigensolver/gen_to_std.h:50,:101
    reduction_to_band / bt_reduction_to_band           include/dlaf/eigensolver/reduction_to_band.h:40-122, bt_reduction_to_band.h

One module per owner, named after the host sources (csrc/host/*.cpp): grid, device_matrix, cholesky, solver,
multiplication, rank_update, addition, inverse, norm, gen_to_std, eigensolver, matrix_function, distribution, and direct
(the tile operations and the one-launch doors of the kernels).  capi holds the ctypes signature table, _abi the few lines
every wrapper shares.  Everything public is re-exported here.

There is no CPU fallback: importing works anywhere, every compute call needs the HIP library
and a GPU and fails loudly otherwise.
"""
from .capi import (DLAFDescriptor, LibraryNotBuilt, lib, lib_path, type_char, version)  # noqa: F401
from ._abi import make_descriptor  # noqa: F401
from .grid import Grid, finalize, initialize  # noqa: F401
from .device_matrix import DeviceMatrix, GeneralDeviceMatrix  # noqa: F401
from .cholesky import (cholesky_factorization, potrf_trace, potrs_device, pxpotrf, pxpotrs, release_workspace_pool,  # noqa: F401
                       set_random_hermitian_positive_definite, update_launch_stats)
from .solver import pxtrsm, solver_profile, triangular_solver, triangular_solver_device  # noqa: F401
from .multiplication import (general_multiplication, general_multiplication_device, hermitian_multiplication,  # noqa: F401
                             hermitian_multiplication_device, multiplication_profile, pxgemm, pxhemm, pxtrmm,
                             triangular_multiplication, triangular_multiplication_device)
from .rank_update import (hermitian_rank_2k_update, hermitian_rank_2k_update_device, hermitian_rank_k_update,  # noqa: F401
                          hermitian_rank_k_update_device, pxher2k, pxherk)
from .addition import (addition_profile, general_addition, general_addition_device, hermitian_complete,  # noqa: F401
                       hermitian_complete_device, pxgeadd, pxlacpy, pxtradd, pxtran)
from .inverse import inverse_from_cholesky_factor, inverse_profile, pxpotri, pxtrtri, triangular_inverse  # noqa: F401
from .norm import matrix_norm, matrix_norm_device, norm_profile, pxlange, pxlanhe, pxlantr  # noqa: F401
from .gen_to_std import generalized_to_standard, pxhegst  # noqa: F401
from .direct import (potrf_direct, tile_gemm, tile_herk, tile_potrf, tile_trsm, trsm_direct, update_bulk_slots,  # noqa: F401
                     update_direct)
from . import distribution  # noqa: F401
from .eigensolver import (band_to_tridiagonal, bt_band_to_tridiagonal, bt_reduction_to_band,  # noqa: F401
                          bt_reduction_to_band_device, eigensolver_min_band, eigensolver_profile, get_band_size, hermitian_eigensolver,
                          hermitian_generalized_eigensolver, red2band_panel_stats, red2band_profile, reduction_to_band,
                          reduction_to_band_device, tridiagonal_eigensolver, pxheevd_partial_spectrum,
                          partial_spectrum_plan, hermitian_eigenvalues, hermitian_generalized_eigenvalues,
                          pxheevd_eigenvalues, pxheevd_partial_spectrum_by_value, pxhegvd_eigenvalues,
                          pxhegvd_partial_spectrum_by_value, sturm_layout, tridiagonal_eigenvalues,
                          tridiagonal_sturm_count)
from .matrix_function import (hermitian_function, hermitian_function_device, hermitian_power,  # noqa: F401
                              hermitian_power_device, hermitian_weighted_rank_k_update,
                              hermitian_weighted_rank_k_update_device)

__all__ = ["hermitian_function", "hermitian_function_device", "hermitian_power", "hermitian_power_device",
           "hermitian_weighted_rank_k_update", "hermitian_weighted_rank_k_update_device",
           "band_to_tridiagonal", "bt_band_to_tridiagonal", "eigensolver_profile", "hermitian_eigensolver",
           "hermitian_generalized_eigensolver", "tridiagonal_eigensolver", "bt_reduction_to_band", "bt_reduction_to_band_device", "get_band_size", "eigensolver_min_band", "red2band_profile",
           "reduction_to_band", "reduction_to_band_device", "DLAFDescriptor", "DeviceMatrix", "GeneralDeviceMatrix", "Grid", "LibraryNotBuilt", "cholesky_factorization", "distribution",
           "finalize", "generalized_to_standard", "initialize", "lib", "lib_path", "make_descriptor", "pxhegst", "pxpotrf", "pxpotrs", "pxtrsm",
           "set_random_hermitian_positive_definite", "solver_profile", "tile_gemm", "tile_herk", "tile_potrf", "tile_trsm",
           "triangular_solver", "triangular_solver_device", "potrs_device", "triangular_inverse",
           "inverse_from_cholesky_factor", "pxtrtri", "pxpotri", "inverse_profile", "type_char", "version",
           "triangular_multiplication", "triangular_multiplication_device", "pxtrmm", "multiplication_profile",
           "hermitian_multiplication", "hermitian_multiplication_device", "pxhemm", "general_multiplication",
           "general_multiplication_device", "pxgemm", "hermitian_rank_k_update", "hermitian_rank_2k_update",
           "hermitian_rank_k_update_device", "hermitian_rank_2k_update_device", "pxherk", "pxher2k", "general_addition",
           "hermitian_complete", "pxgeadd", "pxtradd", "pxtran", "pxlacpy", "general_addition_device",
           "hermitian_complete_device", "addition_profile", "update_direct",
           "update_bulk_slots",
           "trsm_direct", "potrf_direct", "pxheevd_partial_spectrum", "partial_spectrum_plan", "hermitian_eigenvalues",
           "hermitian_generalized_eigenvalues", "pxheevd_eigenvalues", "pxheevd_partial_spectrum_by_value", "pxhegvd_eigenvalues",
           "pxhegvd_partial_spectrum_by_value", "sturm_layout",
           "tridiagonal_eigenvalues", "tridiagonal_sturm_count", "matrix_norm",
           "matrix_norm_device", "pxlange", "pxlanhe", "pxlantr", "norm_profile"]
