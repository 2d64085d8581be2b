// launch_args.hpp -- the arguments of the update / panel kernels, built from the matrix they act on.  M is a
// DeviceMatrix<T> or a TileMatrix<T> (tiles, tile_elems, ltr, ltc, nb, rows, cols); everything that follows from M --
// the tile strides, the block-cyclic geometry, the ragged last tile -- is filled here and nowhere else, every other
// field keeps the default of its struct (device_api.hpp).  Which one for which launch:
//   update_args        C(il, jl) -= a(il) b(jl)^H on and below the diagonal (herk / gemm by global tile index)
//   rect_update_args   the same over every tile of the rectangle (an m x n right-hand side, a panel against 0.5 D)
//   panel_args         TRSM / TRMM of local rows [il0, il1) of one local tile column against a diagonal tile
//   tile_batch_args    TRSM / TRMM of a batch of independent tiles that belong to no matrix
// What is particular to a launch is set on the result: a2 / b2 / K1 / her2k, b_period / b_ts2 / b_jl0, operands that
// are not in tile layout (a_ts, lda, ldb), winv / info / prio / upper / unit of the panel kernels.
#pragma once
#include "../device/device_api.hpp"

namespace dlaf_mi355x {

// local tile rows [il0, il1) x local tile columns [jl0, jl1) of m; a: one tile (nb x K) per local row from il0 on,
// b: the tile of local column jl at b + (jl - jl0) * b_ts
template <class M, class T>
UpdateArgs<T> update_args(const M& m, long il0, long il1, long jl0, long jl1, const T* a, const T* b, long b_ts, int K,
                          const int* info) {
  UpdateArgs<T> ua{};
  ua.c = m.tiles;
  ua.c_tsr = (long) m.tile_elems;
  ua.c_tsc = (long) (m.tile_elems * m.ltr);
  ua.ldc = m.nb;
  ua.a = a;
  ua.a_ts = (long) m.tile_elems;
  ua.lda = m.nb;
  ua.b = b;
  ua.b_ts = b_ts;
  ua.ldb = m.nb;
  ua.il0 = (int) il0;
  ua.il1 = (int) il1;
  ua.jl0 = (int) jl0;
  ua.jl1 = (int) jl1;
  ua.nb = m.nb;
  ua.K = K;
  ua.pr = m.rows.P;
  ua.ri = m.rows.shift();
  ua.pc = m.cols.P;
  ua.ci = m.cols.shift();
  ua.nt = (int) m.rows.nt();
  ua.last_rows = m.rows.last_extent();
  ua.info = info;
  return ua;
}

template <class M, class T>
UpdateArgs<T> rect_update_args(const M& m, long il0, long il1, long jl0, long jl1, const T* a, const T* b, long b_ts,
                               int K, const int* info) {
  UpdateArgs<T> ua = update_args(m, il0, il1, jl0, jl1, a, b, b_ts, K, info);
  ua.rect = 1;
  ua.nt_c = (int) m.cols.nt();
  ua.last_cols = m.cols.last_extent();
  return ua;
}

// Args = TrsmArgs<T> or TrmmArgs<T>: local tile rows [il0, il1) of local tile column klc of m against the diagonal tile
// l (ld nb) of order n
template <class Args, class M, class T>
Args panel_args(const M& m, long il0, long il1, long klc, const T* l, int n) {
  Args ta{};
  ta.b = m.tile(il0, klc);
  ta.b_ts = (long) m.tile_elems;
  ta.ldb = m.nb;
  ta.il0 = (int) il0;
  ta.il1 = (int) il1;
  ta.pr = m.rows.P;
  ta.ri = m.rows.shift();
  ta.nb = m.nb;
  ta.nt = (int) m.rows.nt();
  ta.last_rows = m.rows.last_extent();
  ta.l = l;
  ta.ldl = m.nb;
  ta.n = n;
  return ta;
}

// `ntiles` independent tiles of rows_each x n at b, b + b_ts, ... (ld each) against l (ldl); none of them is "the
// last global tile"
template <class Args, class T>
Args tile_batch_args(T* b, long b_ts, int ld, long ntiles, int rows_each, const T* l, int ldl, int n) {
  Args ta{};
  ta.b = b;
  ta.b_ts = b_ts;
  ta.ldb = ld;
  ta.il0 = 0;
  ta.il1 = (int) ntiles;
  ta.pr = 1;
  ta.ri = 0;
  ta.nb = rows_each;
  ta.nt = (int) ntiles + 1;
  ta.last_rows = rows_each;
  ta.l = l;
  ta.ldl = ldl;
  ta.n = n;
  return ta;
}

// the tile sq x sq (ld sq) at c, alone: C -= a b^H with a, b of K columns (ld sq).  below_diagonal: the tile takes the
// place of global tile (1, 0) of a 3 x 3 grid -- a plain gemm --, otherwise it is the only diagonal tile (herk, lower)
template <class T>
UpdateArgs<T> single_tile_update_args(T* c, const T* a, const T* b, int sq, int K, bool below_diagonal, const int* info) {
  UpdateArgs<T> ua{};
  ua.c = c;
  ua.ldc = sq;
  ua.a = a;
  ua.lda = sq;
  ua.b = b;
  ua.ldb = sq;
  // every tile stride stays 0: the tile index does not move a base
  ua.il0 = below_diagonal ? 1 : 0;
  ua.il1 = ua.il0 + 1;
  ua.jl0 = 0;
  ua.jl1 = 1;
  ua.nb = sq;
  ua.K = K;
  ua.pr = ua.pc = 1;
  ua.ri = ua.ci = 0;
  ua.nt = below_diagonal ? 3 : 1;
  ua.last_rows = sq;
  ua.info = info;
  return ua;
}

// the relayout between m's tiles and a column-major array cm (ld_cm) of the caller's local part; what is particular
// to a relayout is set on the result (full, rev_rows / rev_cols, conj, scale / alpha, jl_first / jl_count)
template <class M, class T>
LayoutArgs<T> layout_args(const M& m, T* cm, long ld_cm) {
  LayoutArgs<T> a;
  a.tiles = m.tiles;
  a.cm = cm;
  a.ld_cm = ld_cm;
  a.ltr = (int) m.ltr;
  a.ltc = (int) m.ltc;
  a.nb = m.nb;
  a.rows = m.rows.local_size();
  a.cols = m.cols.local_size();
  a.pr = m.rows.P;
  a.ri = m.rows.shift();
  a.pc = m.cols.P;
  a.ci = m.cols.shift();
  a.transpose = m.transposed ? 1 : 0;
  return a;
}

// Source (caller-side) local extents: rows/cols of the UNtransposed distribution.
template <class M>
void source_extents(const M& m, long& srows, long& scols) {
  srows = m.transposed ? m.cols.local_size() : m.rows.local_size();
  scols = m.transposed ? m.rows.local_size() : m.cols.local_size();
}

}  // namespace dlaf_mi355x
