// norm_split.hpp -- the work split and the partial-buffer layout of the norm kernels (kernels_norm.hip), in plain C++
// so that the host (norm.cpp), the kernels and a stand-alone host sweep (tests/norm_split/sweep.cpp) share ONE copy.
//
// The operand is the local part of a block-cyclic matrix in tile layout (tile (il, jl) at (il + jl*ltr) nb^2, ld nb,
// global tile gi = il*pr + ri, gj = jl*pc + ci).  A WORK UNIT -- one workgroup of pass 1 -- is
//   (tile (il, jl), row slab sl, column chunk ch):  rows [sl*slab_rows, ..) x columns [ch*cw, ..) of the tile.
// A slab is what the 64 lanes of a wave cover with kNormSlabLoads loads of `ve` elements (16 bytes on the aligned
// path), a chunk is `cw` whole columns that the four waves of the workgroup deal out among themselves.  A unit is
// LIVE when its tile is referenced (every tile of a general matrix; gi >= gj for the Hermitian and the triangular
// structure) and its first row and first column lie inside the tile's extent.  Every live unit writes ALL its slots
// (zeros where the diagonal masks everything), a unit that is not live writes its scalar slot only, and pass 2 reads
// the slots of live units only: every slot has exactly one writer and nothing is read that was not written.
//   scalars   wg_index(unit) * kNormScalars          max, NaN flag, and the three sum-of-squares accumulators
//   colp      (il*nsl + sl) * ldc + jl*nb + c        partial sum of column c over the slab's rows        ldc = ltc*nb
//   rowp      (jl*nch + ch) * ldr + il*nb + r        partial sum of row r over the chunk's columns      ldr = ltr*nb
#pragma once

#if defined(__HIPCC__)
#define DLAF_NORM_FN __host__ __device__ __forceinline__
#else
#define DLAF_NORM_FN inline
#endif

namespace dlaf_mi355x {

constexpr int kNormSlabLoads = 4;   // loads per lane and column of a slab
constexpr int kNormWaves = 4;       // waves per workgroup
constexpr int kNormLanes = 64;
constexpr int kNormScalars = 5;     // max, nan, big, med, sml
constexpr int kNormMinChunk = 32;   // columns of the narrowest chunk
constexpr long kNormTargetUnits = 8192;  // chunks are halved until there are this many units (or kNormMinChunk is hit)

struct NormSplit {
  int ve;         // elements per load: 16 / sizeof(T) on the aligned path, 1 otherwise
  int slab_rows;  // kNormSlabLoads * 64 * ve
  int nsl;        // slabs per tile
  int cw;         // columns per chunk
  int nch;        // chunks per tile
};

// the local operand: extents of the local part, its place in the grid, and which tiles are referenced
struct NormGeom {
  int ltr, ltc, nb;
  long rows, cols;     // local element extents
  int pr, ri, pc, ci;  // gi = il*pr + ri, gj = jl*pc + ci
  int structure;       // 0 general, 1 Hermitian (lower triangle of the view stored), 2 triangular (the same storage)
};

DLAF_NORM_FN bool norm_tile_referenced(const NormGeom& g, int il, int jl) {
  return g.structure == 0 || (long) il * g.pr + g.ri >= (long) jl * g.pc + g.ci;
}
DLAF_NORM_FN int norm_tile_rows(const NormGeom& g, int il) {
  const long left = g.rows - (long) il * g.nb;
  return (int) (left < g.nb ? (left > 0 ? left : 0) : g.nb);
}
DLAF_NORM_FN int norm_tile_cols(const NormGeom& g, int jl) {
  const long left = g.cols - (long) jl * g.nb;
  return (int) (left < g.nb ? (left > 0 ? left : 0) : g.nb);
}
inline long norm_referenced_tiles(const NormGeom& g) {
  long t = 0;
  for (int jl = 0; jl < g.ltc; ++jl)
    for (int il = 0; il < g.ltr; ++il)
      if (norm_tile_referenced(g, il, jl) && norm_tile_rows(g, il) > 0 && norm_tile_cols(g, jl) > 0)
        ++t;
  return t;
}

// elem_bytes = sizeof(T); aligned16: the tiles' base and every tile column are 16-byte aligned
inline NormSplit norm_split(int nb, int elem_bytes, bool aligned16, long referenced_tiles) {
  NormSplit s;
  s.ve = (aligned16 && elem_bytes < 16) ? 16 / elem_bytes : 1;
  s.slab_rows = kNormSlabLoads * kNormLanes * s.ve;
  s.nsl = (nb + s.slab_rows - 1) / s.slab_rows;
  s.cw = nb;
  while (s.cw > kNormMinChunk && referenced_tiles * s.nsl * ((nb + s.cw - 1) / s.cw) < kNormTargetUnits)
    s.cw = (s.cw + 1) / 2;
  if (s.cw < 1)
    s.cw = 1;
  s.nch = (nb + s.cw - 1) / s.cw;
  return s;
}
inline bool norm_aligned16(const void* tiles, int nb, int elem_bytes) {
  return ((unsigned long long) tiles) % 16 == 0 && ((long) nb * elem_bytes) % 16 == 0;
}

// the tile row that load q of `lane` holds in element e of slab sl; wave w of a unit takes the chunk's columns
// ch*cw + w, ch*cw + w + kNormWaves, ...
DLAF_NORM_FN int norm_row_of(const NormSplit& s, int sl, int q, int lane, int e) {
  return sl * s.slab_rows + (q * kNormLanes + lane) * s.ve + e;
}

DLAF_NORM_FN bool norm_unit_live(const NormGeom& g, const NormSplit& s, int il, int jl, int sl, int ch) {
  return norm_tile_referenced(g, il, jl) && sl * s.slab_rows < norm_tile_rows(g, il) && ch * s.cw < norm_tile_cols(g, jl);
}
// units are numbered like the launch: x = sl + nsl*ch, y = il, z = jl
DLAF_NORM_FN long norm_unit_index(const NormGeom& g, const NormSplit& s, int il, int jl, int sl, int ch) {
  return (long) (sl + s.nsl * ch) + (long) s.nsl * s.nch * ((long) il + (long) g.ltr * jl);
}
DLAF_NORM_FN long norm_unit_count(const NormGeom& g, const NormSplit& s) {
  return (long) s.nsl * s.nch * g.ltr * g.ltc;
}
DLAF_NORM_FN long norm_colp_slot(const NormGeom& g, const NormSplit& s, int il, int sl, int jl, int c) {
  return ((long) il * s.nsl + sl) * ((long) g.ltc * g.nb) + (long) jl * g.nb + c;
}
DLAF_NORM_FN long norm_rowp_slot(const NormGeom& g, const NormSplit& s, int jl, int ch, int il, int r) {
  return ((long) jl * s.nch + ch) * ((long) g.ltr * g.nb) + (long) il * g.nb + r;
}
DLAF_NORM_FN long norm_colp_elems(const NormGeom& g, const NormSplit& s) {
  return (long) g.ltr * s.nsl * g.ltc * g.nb;
}
DLAF_NORM_FN long norm_rowp_elems(const NormGeom& g, const NormSplit& s) {
  return (long) g.ltc * s.nch * g.ltr * g.nb;
}

}  // namespace dlaf_mi355x
