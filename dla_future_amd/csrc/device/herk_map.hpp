// herk_map.hpp -- the index arithmetic of the Hermitian rank-k / rank-2k update kernel (kernels_herk.hip): which blocks
// of which tiles of the LOWER triangle of a view run, which of their elements are stored, which of those sit on the
// diagonal, and how trans maps onto the operand forms of gemm_forms.hpp.  Plain C++ and nothing from HIP, so that a host
// program can sweep all of it against a brute-force model (tests/herk_map/sweep.cpp); the kernel includes the same
// definitions.
//
// The view V is n x n in nb x nb tiles, block-cyclic: local tile (il, jl) is global tile (gi, gj) = (il pr + ri,
// jl pc + ci).  A tile is cut into BM x BN blocks (block (bm, bn) starts at (m0, n0) = (bm BM, bn BN) of its tile) and a
// workgroup owns one block.  BM != BN (complex double: 128 x 64) makes blocks of a diagonal tile that straddle the
// diagonal without being "on" it: rows 0 - 127 x columns 64 - 127 lies partly below it and runs, masked.
//
// Operands: the update of the view is  V(i, j) = alpha sum_k x(i, k) conj(y(j, k)) [+ ...] + beta V(i, j)  with x the
// row operand and y the column operand, both tiles of A AS STORED:
//      trans N : A is n x k, a stored nb x K tile per operand           the form pair (N, C) of gemm_forms.hpp
//      trans C : A is k x n, a stored K x nb tile per operand           the form pair (C, N)
// conj_view: V is the plain transpose of the caller's upper-stored C, whose lower triangle is conj(C)'s; its update
// is the same with conj(A) for A, i.e. both conjugation flags flipped.  (Real types ignore the flags.)
#pragma once
#include "gemm_forms.hpp"

namespace dlaf_mi355x {

DLAF_GEMM_FORMS_FN bool herk_trans_is_n(char trans) {
  return trans == 'N' || trans == 'n';
}

// x(r, k) = the row operand of block row m0; y(r, k) = the column operand of block column n0 (ld: the tile's)
DLAF_GEMM_FORMS_FN GemmForm herk_form_x(char trans, int conj_view, int ld, int m0) {
  GemmForm f = gemm_form_a(herk_trans_is_n(trans) ? 'N' : 'C', ld, m0);
  f.conj ^= conj_view ? 1 : 0;
  return f;
}
DLAF_GEMM_FORMS_FN GemmForm herk_form_y(char trans, int conj_view, int ld, int n0) {
  GemmForm f = gemm_form_b(herk_trans_is_n(trans) ? 'C' : 'N', ld, n0);
  f.conj ^= conj_view ? 1 : 0;
  return f;
}
// the vector loader both forms of a trans share (OpSlab mode): 0 rows contiguous (trans N), 1 k contiguous (trans C)
DLAF_GEMM_FORMS_FN int herk_vector_mode(char trans) {
  return herk_trans_is_n(trans) ? 0 : 1;
}

// global tile (gi, gj) holds a part of the lower triangle
DLAF_GEMM_FORMS_FN bool herk_tile_runs(int gi, int gj) {
  return gi >= gj;
}
// the block at (m0, n0) of that tile with mrows x ncols valid elements (both > 0) holds an element of the triangle:
// every block of a tile below the diagonal; in a diagonal tile those whose last row reaches their first column
DLAF_GEMM_FORMS_FN bool herk_block_runs(int gi, int gj, int m0, int mrows, int n0, int ncols) {
  if (gi < gj || mrows <= 0 || ncols <= 0)
    return false;
  return gi > gj || m0 + mrows - 1 >= n0;
}
// element (r, c) of tile (gi, gj), a tile that runs, belongs to the lower triangle / sits on the diagonal
DLAF_GEMM_FORMS_FN bool herk_element_stored(int gi, int gj, int r, int c) {
  return gi > gj || (gi == gj && r >= c);
}
DLAF_GEMM_FORMS_FN bool herk_element_diagonal(int gi, int gj, int r, int c) {
  return gi == gj && r == c;
}

// Local tile `idx` of an operand panel: tiles next to each other (period 1), or grouped into `period` classes by the
// process they came from (the transposed panel of a process grid: class idx % period at base + class * ts2, its
// members idx / period next to each other) -- the addressing of the Cholesky's transposed panel.
DLAF_GEMM_FORMS_FN long herk_panel_offset(int idx, int period, long ts, long ts2) {
  return period <= 1 ? (long) idx * ts : (long) (idx % period) * ts2 + (long) (idx / period) * ts;
}

// The weighted update (hermitian_weighted_rank_k_update: x scaled by a real weight per k between its global load and its
// LDS image): which weights of a slab a thread of the slab loader needs, and which of them each of its registers takes.
// OpSlab::load (gemm_general.hpp) gives thread t of `threads` the pieces idx = t + threads q: a 16-byte load of ve
// elements into registers [q ve, (q + 1) ve) in modes 0 and 1, the single element of register q in mode 2.
//   mode 0: the ve elements of a piece are ve rows of ONE k = idx / (rows / ve)         slot q,  one weight per piece
//   mode 1: ve consecutive k of one row from (idx % (bk / ve)) ve; `threads` is a multiple of bk / ve, so every piece
//           of a thread covers the SAME ve k                                            slot e,  ve weights per thread
//   mode 2: k = idx / rows                                                              slot q,  one weight per element
// herk_weight_slots: how many weights a thread holds; herk_weight_k: the k (inside the slab) of its slot s;
// herk_weight_slot: the slot register r takes.  tests/herk_weight_map/sweep.cpp sweeps the three against the loader's
// own enumeration.
DLAF_GEMM_FORMS_FN int herk_weight_slots(int mode, int rows, int bk, int ve, int threads) {
  return mode == 1 ? ve : (mode == 0 ? rows * bk / (threads * ve) : rows * bk / threads);
}
DLAF_GEMM_FORMS_FN int herk_weight_k(int mode, int t, int s, int rows, int bk, int ve, int threads) {
  if (mode == 0)
    return (t + threads * s) / (rows / ve);
  if (mode == 1)
    return (t % (bk / ve)) * ve + s;
  return (t + threads * s) / rows;
}
DLAF_GEMM_FORMS_FN int herk_weight_slot(int mode, int r, int ve) {
  return mode == 0 ? r / ve : (mode == 1 ? r % ve : r);
}

}  // namespace dlaf_mi355x
