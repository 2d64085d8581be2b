// direct.hpp -- the entries the tests reach single kernels through: one tile with host operands (tile_ops.cpp), one
// launch with every field given by the caller (update_direct.cpp, trsm_direct.cpp, potrf_direct.cpp; the descriptors are
// declared in dlaf_mi355x/dlaf_mi355x.h).
#pragma once

struct dlaf_mi355x_update_desc;
struct dlaf_mi355x_trsm_desc;
struct dlaf_mi355x_potrf_desc;

namespace dlaf_mi355x {

// single-tile operations with host operands (tests of the tile kernels through the C ABI)
template <class T>
int tile_potrf(char uplo, int n, T* a, int lda);
template <class T>
void tile_trsm(char uplo, int m, int n, const T* a, int lda, T* b, int ldb);
template <class T>
void tile_herk(char uplo, int n, int k, const T* a, int lda, T* c, int ldc);
template <class T>
void tile_gemm(char uplo, int m, int n, int k, const T* a, int lda, const T* b, int ldb, T* c, int ldc);
// one launch of the grouped update kernel, every field given by the caller (update_direct.cpp)
template <class T>
int update_direct(::dlaf_mi355x_update_desc& d, void* c, const void* a, const void* b, const void* a2, const void* b2,
                  void* c_again);
// one launch of the panel TRSM and the preparation of its inverted diagonal blocks, every field given by the caller
// (trsm_direct.cpp)
template <class T>
int trsm_direct(::dlaf_mi355x_trsm_desc& d, void* b, const void* l, void* winv);
// one factorization of one diagonal tile on either path, every field given by the caller (potrf_direct.cpp)
template <class T>
int potrf_direct(::dlaf_mi355x_potrf_desc& d, void* tile, void* winv);

}  // namespace dlaf_mi355x
