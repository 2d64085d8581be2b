// gemm_forms.hpp -- how the general multiplication kernel (kernels_gemm.hip) reads op(A) and op(B) from tiles AS STORED:
// the mapping from (op, leading dimension, block origin) to the operand description gemm_acc takes (gemm_general.hpp:
// OpDesc -- pointer, row stride, k stride, conjugation flag), and the choice of the slab loader of a block.  Plain
// C++ and nothing from HIP, so that a host program can sweep both against a brute-force model
// (tests/gemm_forms/sweep.cpp); the kernel includes the same definitions.
//
// gemm_acc computes  acc(m, n) += sum_k a(m, k) * conj(b(n, k))  when neither operand is flagged; a set flag stores the
// conjugate of that operand into LDS instead.  So with a(m, k) = op(A)(m0 + m, k) and b(n, k) = op(B)(k, n0 + n):
//      opA  N : the stored m x k tile, rows contiguous          flag 0     loader mode 0
//           T : the stored k x m tile, k contiguous             flag 0     loader mode 1
//           C : the same, conjugated while it is staged         flag 1     loader mode 1
//      opB  N : the stored k x n tile, k contiguous             flag 1 (undoes gemm_acc's conj)     mode 1
//           T : the stored n x k tile, rows contiguous          flag 1                              mode 0
//           C : the same; gemm_acc's own conj is the op         flag 0                              mode 0
// (the flags HEMM sets for its j < l and j > l tiles, kernels_hemm.hip, are the N and C rows of opB).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DLAF_GEMM_FORMS_FN __host__ __device__ inline
#else
#define DLAF_GEMM_FORMS_FN inline
#endif

namespace dlaf_mi355x {

// element (r, k) of a block's operand sits off + r * rs + k * ks elements from the origin of its tile
struct GemmForm {
  long off, rs, ks;
  int conj;   // OpDesc::conj
  int vmode;  // the vector loader of this form (OpSlab mode): 0 rows contiguous, 1 k contiguous
};

DLAF_GEMM_FORMS_FN bool gemm_op_is_n(char op) {
  return op == 'N' || op == 'n';
}
DLAF_GEMM_FORMS_FN bool gemm_op_is_c(char op) {
  return op == 'C' || op == 'c';
}

// a(r, k) = op(A)(m0 + r, k) of one tile with leading dimension ld
DLAF_GEMM_FORMS_FN GemmForm gemm_form_a(char op, int ld, int m0) {
  if (gemm_op_is_n(op))
    return {(long) m0, 1, (long) ld, 0, 0};
  return {(long) m0 * ld, (long) ld, 1, gemm_op_is_c(op) ? 1 : 0, 1};
}

// b(r, k) with a(m, k) * [flag ? b(n, k) : conj(b(n, k))] = a(m, k) * op(B)(k, n0 + n)
DLAF_GEMM_FORMS_FN GemmForm gemm_form_b(char op, int ld, int n0) {
  if (gemm_op_is_n(op))
    return {(long) n0 * ld, (long) ld, 1, 1, 1};
  return {(long) n0, 1, (long) ld, gemm_op_is_c(op) ? 0 : 1, 0};
}

// The slab loader of one operand of one block and one k tile: the form's vector loader when every promise it relies on
// holds -- the block's first element and every column (ld) of the tile on a 16-byte boundary, a whole block of rows, a
// whole number of BK slabs -- and the bounds-checked element loader (mode 2) otherwise.
template <int ELEM_BYTES>
DLAF_GEMM_FORMS_FN int gemm_loader_mode(const GemmForm& f, const void* tile, int ld, int rows_valid, int rows_block,
                                        int K, int BK) {
  const std::uintptr_t first = reinterpret_cast<std::uintptr_t>(tile) + (std::uintptr_t) (f.off * ELEM_BYTES);
  const bool aligned = first % 16 == 0 && ((long) ld * ELEM_BYTES) % 16 == 0;
  return (aligned && rows_valid == rows_block && K > 0 && K % BK == 0) ? f.vmode : 2;
}

}  // namespace dlaf_mi355x
