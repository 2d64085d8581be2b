// geadd_map.hpp -- the index arithmetic of the addition / transposition kernel (kernels_geadd.hip): the work-unit
// decomposition, which units run for a uplo mask and which of their elements are written, the choice between the
// 16-byte and the element path, the source tile and source element of a destination element, and the LDS image of the
// transposing form.  Plain C++ and nothing from HIP, so that a host program can sweep all of it against a brute-force
// model (tests/geadd_map/sweep.cpp); the kernel and the host (addition.cpp) include the same definitions.
//
// The destination D is the local part of a block-cyclic matrix in tile layout: tile (il, jl) is global tile (gi, gj) =
// (il pr + ri, jl pc + ci), nb x nb with leading dimension nb, `rows` x `cols` local elements (the last local tile
// ragged).  A tile is cut into B x B sub-blocks, B = geadd_block(sizeof(T)); a WORK UNIT -- one workgroup -- owns the
// sub-block (bi, bj) of one tile: rows [bi B, ..) x columns [bj B, ..).  Tiles and sub-blocks are square and start at
// multiples of their size in both directions, so a sub-block lies on the global diagonal (gi == gj and bi == bj) or
// wholly on one side of it.
//
// The source of destination element (r, c) of tile (il, jl) is element (r, c) of the source tile (straight form) or
// element (c, r) of it (transposing form); the source tile sits at
//      (il - il0) a_tsi + geadd_panel_offset(jl, a_period, a_ts, a_ts2)
// which covers a tile matrix as stored (straight: a_tsi = tile, a_ts = tile column; transposing on one process: the
// two swapped, the source tile of (il, jl) is (jl, il)) and one tile row of D fed from the panel buffer that
// bcast_transposed_panel_whole fills on a process grid (il0 = that row, a_tsi = 0, the classes at a_ts2).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DLAF_GEADD_FN __host__ __device__ __forceinline__
#else
#define DLAF_GEADD_FN inline
#endif

namespace dlaf_mi355x {

constexpr int kGeaddThreads = 256;

// the uplo part in GLOBAL element coordinates (row gr, column gc)
constexpr int kGeaddAll = 0;       // every element
constexpr int kGeaddLowerEq = 1;   // gr >= gc   (uplo L)
constexpr int kGeaddUpperEq = 2;   // gr <= gc   (uplo U)
constexpr int kGeaddLower = 3;     // gr >  gc
constexpr int kGeaddUpper = 4;     // gr <  gc

// what a launch does with an element: decided ONCE per launch on the host (geadd_arith), a template argument of the
// kernel, so that a copy carries no multiply
constexpr int kGeaddCopy = 0;      // alpha = 1, beta = 0:  D = op(A)            -- a move of the bits
constexpr int kGeaddScale = 1;     //            beta = 0:  D = alpha op(A)      -- D is not read
constexpr int kGeaddAxpby = 2;     //                       D = beta D + alpha op(A)
constexpr int kGeaddScaleC = 3;    // alpha = 0:            D = beta D           -- A is not referenced
constexpr int kGeaddZero = 4;      // alpha = 0, beta = 0:  D = 0                -- neither is read
DLAF_GEADD_FN int geadd_arith(bool alpha_zero, bool alpha_one, bool beta_zero) {
  if (alpha_zero)
    return beta_zero ? kGeaddZero : kGeaddScaleC;
  if (beta_zero)
    return alpha_one ? kGeaddCopy : kGeaddScale;
  return kGeaddAxpby;
}
DLAF_GEADD_FN constexpr bool geadd_reads_a(int arith) {
  return arith == kGeaddCopy || arith == kGeaddScale || arith == kGeaddAxpby;
}
DLAF_GEADD_FN constexpr bool geadd_reads_c(int arith) {
  return arith == kGeaddAxpby || arith == kGeaddScaleC;
}

// side of a sub-block in elements: 64 for the 4- and 8-byte types, 32 for complex double -- 16, 32, 32 and 16 KiB of
// LDS per workgroup of the transposing form, 4 to 8 workgroups on a compute unit
DLAF_GEADD_FN constexpr int geadd_block(int elem_bytes) {
  return elem_bytes >= 16 ? 32 : 64;
}

// elements per global access: 16 bytes' worth when the tile bases and every tile column of both operands are 16-byte
// aligned (every tile stride is a multiple of nb nb elements, so the column rule covers them), otherwise 1
DLAF_GEADD_FN int geadd_vector_elems(int elem_bytes, int nb, unsigned long long a_base, unsigned long long c_base) {
  if (elem_bytes >= 16)
    return 1;
  const bool aligned = a_base % 16 == 0 && c_base % 16 == 0 && ((long) nb * elem_bytes) % 16 == 0;
  return aligned ? 16 / elem_bytes : 1;
}

struct GeaddGeom {
  int ltr, ltc, nb;    // local tiles of D, tile size = leading dimension of every tile
  long rows, cols;     // local element extents of D
  int pr, ri, pc, ci;  // gi = il pr + ri, gj = jl pc + ci
  int il0, nil;        // the local tile rows [il0, il0 + nil) a launch covers (every local tile column)
};

DLAF_GEADD_FN bool geadd_element_in(int mask, long gr, long gc) {
  switch (mask) {
    case kGeaddLowerEq: return gr >= gc;
    case kGeaddUpperEq: return gr <= gc;
    case kGeaddLower: return gr > gc;
    case kGeaddUpper: return gr < gc;
    default: return true;
  }
}

// the rectangle of global rows [gr0, gr0 + nr) x columns [gc0, gc0 + nc), nr, nc > 0, against the part:
// 0 no element inside, 1 every element inside, 2 the diagonal crosses it (element mask)
constexpr int kGeaddDead = 0, kGeaddWhole = 1, kGeaddCrossed = 2;
DLAF_GEADD_FN int geadd_rect_class(int mask, long gr0, int nr, long gc0, int nc) {
  const long gr1 = gr0 + nr - 1, gc1 = gc0 + nc - 1;
  switch (mask) {
    case kGeaddLowerEq: return gr0 >= gc1 ? kGeaddWhole : gr1 < gc0 ? kGeaddDead : kGeaddCrossed;
    case kGeaddUpperEq: return gr1 <= gc0 ? kGeaddWhole : gr0 > gc1 ? kGeaddDead : kGeaddCrossed;
    case kGeaddLower: return gr0 > gc1 ? kGeaddWhole : gr1 <= gc0 ? kGeaddDead : kGeaddCrossed;
    case kGeaddUpper: return gr1 < gc0 ? kGeaddWhole : gr0 >= gc1 ? kGeaddDead : kGeaddCrossed;
    default: return kGeaddWhole;
  }
}

DLAF_GEADD_FN int geadd_tile_rows(const GeaddGeom& g, int il) {
  const long left = g.rows - (long) il * g.nb;
  return (int) (left < g.nb ? (left > 0 ? left : 0) : g.nb);
}
DLAF_GEADD_FN int geadd_tile_cols(const GeaddGeom& g, int jl) {
  const long left = g.cols - (long) jl * g.nb;
  return (int) (left < g.nb ? (left > 0 ? left : 0) : g.nb);
}
DLAF_GEADD_FN int geadd_sub_blocks(int nb, int B) {
  return (nb + B - 1) / B;
}

// the work unit (sub-block (bi, bj) of local tile (il, jl)): its first row / column inside the tile, its valid extent,
// the global element coordinates of its origin, and its class (kGeaddDead: the workgroup leaves at once)
struct GeaddUnit {
  int r0, c0, nr, nc;
  long gr0, gc0;
  int cls;
};
DLAF_GEADD_FN GeaddUnit geadd_unit(const GeaddGeom& g, int mask, int B, int il, int jl, int bi, int bj) {
  GeaddUnit u;
  u.r0 = bi * B;
  u.c0 = bj * B;
  const int tr = geadd_tile_rows(g, il), tc = geadd_tile_cols(g, jl);
  u.nr = tr - u.r0 < B ? tr - u.r0 : B;
  u.nc = tc - u.c0 < B ? tc - u.c0 : B;
  u.gr0 = ((long) il * g.pr + g.ri) * g.nb + u.r0;
  u.gc0 = ((long) jl * g.pc + g.ci) * g.nb + u.c0;
  u.cls = (u.nr <= 0 || u.nc <= 0) ? kGeaddDead : geadd_rect_class(mask, u.gr0, u.nr, u.gc0, u.nc);
  return u;
}

// the ve elements of rows [r, r + ve) of global column gc, first global row gr, in a unit of class cls whose valid rows
// end before rend: true when all of them are valid and inside the part (one 16-byte store), false: element by element.
// (Along a column the part is an interval, so the first and the last element decide.)
DLAF_GEADD_FN bool geadd_vector_whole(int mask, int cls, int ve, int r, int rend, long gr, long gc) {
  if (r + ve > rend)
    return false;
  return cls != kGeaddCrossed || (geadd_element_in(mask, gr, gc) && geadd_element_in(mask, gr + ve - 1, gc));
}
// element e of such a vector is written on the element path
DLAF_GEADD_FN bool geadd_element_written(int mask, int cls, int r, int e, int rend, long gr, long gc) {
  return r + e < rend && (cls == kGeaddWhole || geadd_element_in(mask, gr + e, gc));
}

// Local tile `idx` of a panel: tiles next to each other (period <= 1), or grouped into `period` classes by the process
// they came from -- the layout bcast_transposed_panel_whole leaves: class idx % period at ts2, its members idx / period
// next to each other
DLAF_GEADD_FN long geadd_panel_offset(int idx, int period, long ts, long ts2) {
  return period <= 1 ? (long) idx * ts : (long) (idx % period) * ts2 + (long) (idx / period) * ts;
}
DLAF_GEADD_FN long geadd_src_tile_offset(const GeaddGeom& g, int il, int jl, long a_tsi, int a_period, long a_ts,
                                         long a_ts2) {
  return (long) (il - g.il0) * a_tsi + geadd_panel_offset(jl, a_period, a_ts, a_ts2);
}
// the element of the source tile that destination element (r, c) takes
DLAF_GEADD_FN long geadd_src_elem(bool trans, int r, int c, int nb) {
  return trans ? (long) c + (long) r * nb : (long) r + (long) c * nb;
}

// Thread t's q-th access of a unit is vector v = t + q kGeaddThreads of the B B / ve vectors of the sub-block: ve
// consecutive rows from geadd_vec_row in column geadd_vec_col -- consecutive lanes walk down a tile column, so a wave's
// access is made of contiguous runs of B elements.  Both sides of the transposing form use this map, each in the
// coordinates of its own tile.
DLAF_GEADD_FN int geadd_vec_row(int ve, int B, int v) {
  return ve * (v % (B / ve));
}
DLAF_GEADD_FN int geadd_vec_col(int ve, int B, int v) {
  return v / (B / ve);
}

// LDS image of the SOURCE sub-block in the transposing form: column sc of the block is B elements = B / ve slots of ve
// elements (16 bytes on the vector path), unpadded, and the slot of rows [sr, sr + ve) is XOR-swizzled with the
// column's slot index.  The load side writes whole slots (one 16-byte ds_write per global vector), the store side
// gathers the ve elements of a destination vector from ve consecutive columns.  Element index into the image:
DLAF_GEADD_FN int geadd_lds_index(int ve, int B, int sr, int sc) {
  const int slots = B / ve;
  return sc * B + (((sr / ve) ^ ((sc / ve) % slots)) * ve) + sr % ve;
}

}  // namespace dlaf_mi355x
