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

}  // namespace dlaf_mi355x
