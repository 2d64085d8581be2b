// api_checks.hpp -- the argument checks of the C API (c_api.cpp, c_api_host.cpp, c_api_device.cpp) in one vocabulary.
// Host only: no HIP header, usable from a plain g++ program (tests/api_checks/sweep.cpp sweeps the predicates against a
// brute-force model).  The predicates answer; the require_* helpers terminate through fatal() (runtime.cpp) before
// anything touches the GPU, the way upstream's asserts do.  who names the routine in a message; nullptr: no prefix.
#pragma once
#include <cstring>
#include <initializer_list>
#include <string>

#include <dlaf_c/desc.h>

#include "host_operand.hpp"

namespace dlaf_mi355x {

[[noreturn]] void fatal(const char* fmt, ...);

#pragma GCC visibility push(hidden)  // helpers of the C API's own files: the library exports none of them

// ---- letters (NUL is in no set)
inline bool in_set(char c, const char* set) {
  return c != 0 && std::strchr(set, c) != nullptr;
}
inline bool is_uplo(char c) { return in_set(c, "LlUu"); }
inline bool is_lower(char c) { return in_set(c, "Ll"); }
inline bool is_upper(char c) { return in_set(c, "Uu"); }
inline bool is_side(char c) { return in_set(c, "LlRr"); }
inline bool is_left(char c) { return in_set(c, "Ll"); }
inline bool is_op(char c) { return in_set(c, "NnTtCc"); }
inline bool is_diag(char c) { return in_set(c, "NnUu"); }

// ---- source process inside the grid (GridT: anything with nprow, npcol; the library passes its Grid)
inline bool source_in_grid(int nprow, int npcol, int isrc, int jsrc) {
  return isrc >= 0 && isrc < nprow && jsrc >= 0 && jsrc < npcol;
}
template <class GridT>
bool source_in_grid(const GridT& g, const DLAF_descriptor& d) {
  return source_in_grid(g.nprow, g.npcol, d.isrc, d.jsrc);
}
template <class GridT>
void require_sources(const char* who, const GridT& g, std::initializer_list<const DLAF_descriptor*> descs) {
  for (const DLAF_descriptor* d : descs)
    if (!source_in_grid(g, *d))
      fatal("[dlaf_mi355x] %s%ssource rank (%d,%d) outside the %d x %d grid\n", who ? who : "", who ? ": " : "", d->isrc,
            d->jsrc, g.nprow, g.npcol);
}

// ---- descriptors
inline void require_uplo(char uplo) {
  if (!is_uplo(uplo))
    fatal("[dlaf_mi355x] uplo must be 'L' or 'U', got '%c'\n", uplo);
}
// square matrix, square blocks, no offsets: the preconditions of dlaf::cholesky_factorization
// (include/dlaf/factorization/cholesky.h:39-79) and of its C wrapper (src/c_api/factorization/cholesky.h:37-38), which
// gen_to_std, the inverses, reduction_to_band (reduction_to_band.h:103-106), band_to_tridiagonal
// (band_to_tridiag.h:76-80) and the eigensolvers share
inline void require_square_desc(const DLAF_descriptor& d) {
  if (d.i != 0 || d.j != 0)
    fatal("[dlaf_mi355x] sub-matrices are not supported: i = %d, j = %d must be 0\n", d.i, d.j);
  if (d.m != d.n)
    fatal("[dlaf_mi355x] Cholesky needs a square matrix: %d x %d\n", d.m, d.n);
  if (d.mb != d.nb || d.nb < 1)
    fatal("[dlaf_mi355x] Cholesky needs square blocks: %d x %d\n", d.mb, d.nb);
  if (d.m < 0)
    fatal("[dlaf_mi355x] negative matrix size %d\n", d.m);
}
// the eigensolvers' B and Z: described like A, without offsets (eigensolver.h:44-45 upstream)
inline void require_like(const char* who, const DLAF_descriptor& da, std::initializer_list<const DLAF_descriptor*> others) {
  for (const DLAF_descriptor* d : others) {
    if (d->i != 0 || d->j != 0)
      fatal("[dlaf_mi355x] %s: sub-matrix offsets must be 0\n", who);
    if (d->m != da.m || d->n != da.n || d->mb != da.mb || d->nb != da.nb)
      fatal("[dlaf_mi355x] %s: B and Z must have A's size %d x %d and block %d x %d\n", who, da.m, da.n, da.mb, da.nb);
  }
}
// reduction_to_band.h:108-109, band_to_tridiag.h:78-80
inline void require_band(const char* who, int band, int nb) {
  if (band < 2 || nb % band != 0)
    fatal("[dlaf_mi355x] %s: band_size %d must be >= 2 and divide the block size %d\n", who, band, nb);
}

// ---- the Level-3 families: one judgement each for the descriptor entries, the p? entries and the resident ones.  Every
// operand as an OperandDesc (host_operand.hpp) of the matrix AS STORED; a HostOperand is one.
inline OperandDesc operand_desc(const DLAF_descriptor& d) {
  return {d.m, d.n, d.mb, d.nb, d.isrc, d.jsrc};
}
inline bool is_notrans(char c) { return in_set(c, "Nn"); }

// ---- triangular solver / multiplication  B = alpha op(A)^-1 B, alpha op(A) B (side L) / the same from the right: a the
// triangular matrix, b the m x n matrix that is overwritten; a_stored: the triangle a resident A holds (0: A is a host
// array).  Terminates unless: the four letters are letters; A is square with one square block; A's order is B's rows
// (side L) / columns (side R); B's block along the triangular dimension is A's (util_matrix.h:123-143; the other one is
// free: the device tiles stay square, the free dimension is re-cut locally, tile_matrix.hpp create_rhs); every source
// inside the grid; a resident A holds the uplo triangle; A and a non-empty B start on the same process along the
// triangular dimension.
template <class GridT>
void require_triangular(const char* who, const GridT& g, char side, char uplo, char op, char diag, const OperandDesc& a,
                        const OperandDesc& b, char a_stored = 0) {
  if (!is_side(side) || !is_uplo(uplo) || !is_op(op) || !is_diag(diag))
    fatal("[dlaf_mi355x] %s: bad side/uplo/op/diag '%c' '%c' '%c' '%c'\n", who, side, uplo, op, diag);
  if (a.m != a.n || a.mb != a.nb || a.nb < 1)
    fatal("[dlaf_mi355x] %s: A must be square with square blocks (%ld x %ld, %d x %d)\n", who, a.m, a.n, a.mb, a.nb);
  const bool left = is_left(side);
  if (b.m < 0 || b.n < 0 || a.m != (left ? b.m : b.n))
    fatal("[dlaf_mi355x] %s: A is %ld x %ld, B is %ld x %ld (side %c)\n", who, a.m, a.n, b.m, b.n, side);
  if ((left ? b.mb : b.nb) != a.nb || b.mb < 1 || b.nb < 1)
    fatal("[dlaf_mi355x] %s: B's blocks (%d x %d) do not match A's (%d x %d) for side %c\n", who, b.mb, b.nb, a.mb, a.nb,
          side);
  for (const OperandDesc* o : {&a, &b})
    if (!source_in_grid(g.nprow, g.npcol, o->isrc, o->jsrc))
      fatal("[dlaf_mi355x] source rank (%d,%d) outside the %d x %d grid\n", o->isrc, o->jsrc, g.nprow, g.npcol);
  if (a_stored != 0 && is_upper(a_stored) != is_upper(uplo))
    fatal("[dlaf_mi355x] %s: uplo '%c' but the resident matrix holds its '%c' triangle\n", who, uplo, a_stored);
  if (b.m > 0 && b.n > 0 && (left ? (a.isrc != b.isrc) : (a.jsrc != b.jsrc)))
    fatal("[dlaf_mi355x] %s: A and B must share the source process along the triangular dimension\n", who);
}

// ---- Hermitian multiplication  C = beta C + alpha A B (side L) / beta C + alpha B A (side R), A Hermitian in its uplo
// triangle (dlaf::hermitian_multiplication, include/dlaf/multiplication/hermitian.h, and this build's own conditions, the
// solver's); a_stored as above.  Terminates unless: side and uplo are letters; A is square with one square block; B has
// C's shape and blocks; A's order is C's rows (side L) / columns (side R) and C's block along that dimension is A's;
// every source inside the grid; a resident A holds the uplo triangle; B starts on C's process, and A on a non-empty C's
// along A's dimension.
template <class GridT>
void require_hermitian_multiplication(const char* who, const GridT& g, char side, char uplo, const OperandDesc& a,
                                      const OperandDesc& b, const OperandDesc& c, char a_stored = 0) {
  if (!is_side(side) || !is_uplo(uplo))
    fatal("[dlaf_mi355x] %s: bad side/uplo '%c' '%c'\n", who, side, uplo);
  if (a.m != a.n || a.mb != a.nb || a.nb < 1)
    fatal("[dlaf_mi355x] %s: A must be square with square blocks (%ld x %ld, %d x %d)\n", who, a.m, a.n, a.mb, a.nb);
  const bool left = is_left(side);
  if (c.m < 0 || c.n < 0 || b.m != c.m || b.n != c.n || b.mb != c.mb || b.nb != c.nb)
    fatal("[dlaf_mi355x] %s: B (%ld x %ld, blocks %d x %d) and C (%ld x %ld, blocks %d x %d) differ\n", who, b.m, b.n, b.mb,
          b.nb, c.m, c.n, c.mb, c.nb);
  if (a.m != (left ? c.m : c.n))
    fatal("[dlaf_mi355x] %s: A is %ld x %ld, B and C are %ld x %ld (side %c)\n", who, a.m, a.n, c.m, c.n, side);
  if ((left ? c.mb : c.nb) != a.nb || c.mb < 1 || c.nb < 1)
    fatal("[dlaf_mi355x] %s: the blocks of B and C (%d x %d) do not match A's (%d x %d) for side %c\n", who, c.mb, c.nb,
          a.mb, a.nb, side);
  for (const OperandDesc* o : {&a, &b, &c})
    if (!source_in_grid(g.nprow, g.npcol, o->isrc, o->jsrc))
      fatal("[dlaf_mi355x] %s: source rank (%d,%d) outside the %d x %d grid\n", who, o->isrc, o->jsrc, g.nprow, g.npcol);
  if (a_stored != 0 && is_upper(a_stored) != is_upper(uplo))
    fatal("[dlaf_mi355x] %s: uplo '%c' but the resident matrix holds its '%c' triangle\n", who, uplo, a_stored);
  if (b.isrc != c.isrc || b.jsrc != c.jsrc)
    fatal("[dlaf_mi355x] %s: B and C must share the source process ((%d,%d) vs (%d,%d))\n", who, b.isrc, b.jsrc, c.isrc,
          c.jsrc);
  if (c.m > 0 && c.n > 0 && (left ? (a.isrc != c.isrc) : (a.jsrc != c.jsrc)))
    fatal("[dlaf_mi355x] %s: A must share the source process of B and C along A's dimension\n", who);
}

// ---- general multiplication  C = beta C + alpha op(A) op(B)
// Terminates unless: both ops are letters; one square block for the three matrices; op(A) is m x k, op(B) k x n for C's
// m x n; every source inside the grid; on a grid of more than one process both ops are 'N' (the transposed forms need
// the two-hop transposed-panel broadcast, which is not built), A starts on C's process row and B on C's process column.
template <class GridT>
void require_general_multiplication(const char* who, const GridT& g, char opa, char opb, const OperandDesc& a,
                                    const OperandDesc& b, const OperandDesc& c) {
  if (!is_op(opa) || !is_op(opb))
    fatal("[dlaf_mi355x] %s: bad opa/opb '%c' '%c'\n", who, opa, opb);
  if (a.mb != a.nb || b.mb != b.nb || c.mb != c.nb || a.nb != c.nb || b.nb != c.nb || c.nb < 1)
    fatal("[dlaf_mi355x] %s: A, B and C need one square block (A %d x %d, B %d x %d, C %d x %d)\n", who, a.mb, a.nb,
          b.mb, b.nb, c.mb, c.nb);
  const long am = is_notrans(opa) ? a.m : a.n, ak = is_notrans(opa) ? a.n : a.m;
  const long bk = is_notrans(opb) ? b.m : b.n, bn = is_notrans(opb) ? b.n : b.m;
  if (c.m < 0 || c.n < 0 || ak < 0 || am != c.m || bn != c.n || ak != bk)
    fatal("[dlaf_mi355x] %s: op(A) is %ld x %ld (op '%c'), op(B) is %ld x %ld (op '%c'), C is %ld x %ld\n", who, am, ak,
          opa, bk, bn, opb, c.m, c.n);
  for (const OperandDesc* o : {&a, &b, &c})
    if (!source_in_grid(g.nprow, g.npcol, o->isrc, o->jsrc))
      fatal("[dlaf_mi355x] %s: source rank (%d,%d) outside the %d x %d grid\n", who, o->isrc, o->jsrc, g.nprow, g.npcol);
  if (g.nprow * g.npcol > 1 && (!is_notrans(opa) || !is_notrans(opb)))
    fatal("[dlaf_mi355x] %s: opa '%c', opb '%c' on a %d x %d grid: only 'N' 'N' is built on more than one process\n", who,
          opa, opb, g.nprow, g.npcol);
  if (a.isrc != c.isrc)
    fatal("[dlaf_mi355x] %s: A must start on C's process row (source row %d vs %d)\n", who, a.isrc, c.isrc);
  if (b.jsrc != c.jsrc)
    fatal("[dlaf_mi355x] %s: B must start on C's process column (source column %d vs %d)\n", who, b.jsrc, c.jsrc);
}

// ---- Hermitian rank-k / rank-2k update of the uplo triangle of C: one judgement for the descriptor entries, the p?
// entries and the resident ones.  a (and b, rank-2k; nullptr: rank-k) as stored; c_stored: the triangle a resident C
// holds (0: C is a host array).  Terminates unless: uplo and trans are letters, and trans is not 'T' on a complex type
// (that is the complex-symmetric p{c,z}syrk, which is not built); C is square; A is n x k (trans N) or k x n; B has A's
// shape, blocks and source; one square block for all; every source inside the grid; a resident C holds the uplo
// triangle; on a grid of more than one process trans is 'N' (the transposed forms need the two-hop transposed-panel
// broadcast of A's ROWS, which is not built) and A starts on C's process row.
template <class GridT>
void require_rank_update(const char* who, const GridT& g, bool complex_type, char uplo, char trans, const OperandDesc& a,
                         const OperandDesc* b, const OperandDesc& c, char c_stored = 0) {
  if (!is_uplo(uplo) || !is_op(trans))
    fatal("[dlaf_mi355x] %s: bad uplo/trans '%c' '%c'\n", who, uplo, trans);
  if (complex_type && in_set(trans, "Tt"))
    fatal("[dlaf_mi355x] %s: trans '%c' on a complex type (the complex-symmetric update) is not built; use 'N' or 'C'\n",
          who, trans);
  if (c.m != c.n || c.n < 0)
    fatal("[dlaf_mi355x] %s: C must be square (%ld x %ld)\n", who, c.m, c.n);
  const bool tn = is_notrans(trans);
  const long an = tn ? a.m : a.n, ak = tn ? a.n : a.m;
  if (an != c.n || ak < 0)
    fatal("[dlaf_mi355x] %s: A is %ld x %ld (trans '%c'), C is %ld x %ld\n", who, a.m, a.n, trans, c.m, c.n);
  if (b && (b->m != a.m || b->n != a.n || b->mb != a.mb || b->nb != a.nb || b->isrc != a.isrc || b->jsrc != a.jsrc))
    fatal("[dlaf_mi355x] %s: A (%ld x %ld, block %d x %d, source %d,%d) and B (%ld x %ld, block %d x %d, source %d,%d) "
          "differ\n", who, a.m, a.n, a.mb, a.nb, a.isrc, a.jsrc, b->m, b->n, b->mb, b->nb, b->isrc, b->jsrc);
  if (a.mb != a.nb || c.mb != c.nb || a.nb != c.nb || c.nb < 1)
    fatal("[dlaf_mi355x] %s: the operands need one square block (A %d x %d, C %d x %d)\n", who, a.mb, a.nb, c.mb, c.nb);
  for (const OperandDesc* o : {&a, &c})
    if (!source_in_grid(g.nprow, g.npcol, o->isrc, o->jsrc))
      fatal("[dlaf_mi355x] %s: source rank (%d,%d) outside the %d x %d grid\n", who, o->isrc, o->jsrc, g.nprow, g.npcol);
  if (c_stored != 0 && is_upper(c_stored) != is_upper(uplo))
    fatal("[dlaf_mi355x] %s: uplo '%c' but the resident matrix holds its '%c' triangle\n", who, uplo, c_stored);
  if (g.nprow * g.npcol > 1 && !tn)
    fatal("[dlaf_mi355x] %s: trans '%c' on a %d x %d grid: only 'N' is built on more than one process\n", who, trans,
          g.nprow, g.npcol);
  if (tn && a.isrc != c.isrc)
    fatal("[dlaf_mi355x] %s: A must start on C's process row (source row %d vs %d)\n", who, a.isrc, c.isrc);
}

// ---- the weighted rank-k update  C = alpha A D A^H + beta C: require_rank_update's tests (b: none) under its own
// name, and the weights: d null while they would be read (k > 0 and alpha != 0).  Their values are not judged.
template <class GridT>
void require_weighted_rank_update(const GridT& g, bool complex_type, char uplo, char trans, bool alpha_is_zero,
                                  const OperandDesc& a, const void* d, const OperandDesc& c, char c_stored = 0) {
  const char* who = "hermitian weighted rank-k update";
  require_rank_update(who, g, complex_type, uplo, trans, a, nullptr, c, c_stored);
  const long k = is_notrans(trans) ? a.n : a.m;
  if (!d && k > 0 && !alpha_is_zero)
    fatal("[dlaf_mi355x] %s: the weights d are null (k = %ld, alpha != 0)\n", who, k);
}
// ---- functions of a Hermitian matrix: uplo 'L' (the eigensolver's); a square matrix in square blocks with its source
// inside the grid; at most one selection; hermitian_power: threshold >= 0
template <class GridT>
void require_hermitian_function(const char* who, const GridT& g, char uplo, const OperandDesc& a, bool by_index,
                                bool by_value) {
  if (uplo != 'L' && uplo != 'l')
    fatal("[dlaf_mi355x] %s: uplo = %c is not implemented (neither by the eigensolver)\n", who, uplo);
  if (a.m != a.n || a.n < 0)
    fatal("[dlaf_mi355x] %s: the matrix must be square (%ld x %ld)\n", who, a.m, a.n);
  if (a.mb != a.nb || a.nb < 1)
    fatal("[dlaf_mi355x] %s: the matrix needs a square block (%d x %d)\n", who, a.mb, a.nb);
  if (!source_in_grid(g.nprow, g.npcol, a.isrc, a.jsrc))
    fatal("[dlaf_mi355x] %s: source rank (%d,%d) outside the %d x %d grid\n", who, a.isrc, a.jsrc, g.nprow, g.npcol);
  if (by_index && by_value)
    fatal("[dlaf_mi355x] %s: two selections at once: give an index range or a value interval, not both\n", who);
}
inline void require_power_threshold(const char* who, double threshold) {
  if (!(threshold >= 0))
    fatal("[dlaf_mi355x] %s: threshold %g < 0: eigenvalues at or below the threshold are dropped, and a negative one "
          "has no real power\n", who, threshold);
}

// ---- general addition  C = beta C + alpha op(A) on the uplo part, hermitian_complete and the resident conversions: one
// judgement for the descriptor entries, the p? entries and the resident ones.  a, c as stored; same_storage: A and C are
// the same array / handle.  Terminates unless: uplo is A, L or U and op a letter; one square block for both; C is m x n
// and A m x n (op N) or n x m; every source inside the grid; for op N A starts on C's source process (the launch is
// local: both must hold the same elements); the same storage twice only with op N.
inline bool is_part(char c) { return in_set(c, "AaLlUu"); }
template <class GridT>
void require_general_addition(const char* who, const GridT& g, char uplo, char op, const OperandDesc& a,
                              const OperandDesc& c, bool same_storage) {
  if (!is_part(uplo) || !is_op(op))
    fatal("[dlaf_mi355x] %s: bad uplo/op '%c' '%c' (uplo is 'A', 'L' or 'U')\n", who, uplo, op);
  if (a.mb != a.nb || c.mb != c.nb || a.nb != c.nb || c.nb < 1)
    fatal("[dlaf_mi355x] %s: A and C need one square block (A %d x %d, C %d x %d)\n", who, a.mb, a.nb, c.mb, c.nb);
  const bool tn = is_notrans(op);
  if (c.m < 0 || c.n < 0 || (tn ? a.m : a.n) != c.m || (tn ? a.n : a.m) != c.n)
    fatal("[dlaf_mi355x] %s: A is %ld x %ld (op '%c'), C is %ld x %ld\n", who, a.m, a.n, op, c.m, c.n);
  for (const OperandDesc* o : {&a, &c})
    if (!source_in_grid(g.nprow, g.npcol, o->isrc, o->jsrc))
      fatal("[dlaf_mi355x] %s: source rank (%d,%d) outside the %d x %d grid\n", who, o->isrc, o->jsrc, g.nprow, g.npcol);
  if (tn && (a.isrc != c.isrc || a.jsrc != c.jsrc))
    fatal("[dlaf_mi355x] %s: op 'N' needs A on C's source process (source %d,%d vs %d,%d)\n", who, a.isrc, a.jsrc, c.isrc,
          c.jsrc);
  if (same_storage && !tn)
    fatal("[dlaf_mi355x] %s: A and C are the same matrix, which only op 'N' accepts (op '%c')\n", who, op);
}
template <class GridT>
void require_hermitian_complete(const char* who, const GridT& g, char uplo, char kind, const OperandDesc& a) {
  if (!is_uplo(uplo) || !in_set(kind, "HhSs"))
    fatal("[dlaf_mi355x] %s: bad uplo/kind '%c' '%c' (kind is 'H' or 'S')\n", who, uplo, kind);
  if (a.m != a.n || a.n < 0)
    fatal("[dlaf_mi355x] %s: the matrix must be square (%ld x %ld)\n", who, a.m, a.n);
  if (a.mb != a.nb || a.nb < 1)
    fatal("[dlaf_mi355x] %s: the matrix needs a square block (%d x %d)\n", who, a.mb, a.nb);
  if (!source_in_grid(g.nprow, g.npcol, a.isrc, a.jsrc))
    fatal("[dlaf_mi355x] %s: source rank (%d,%d) outside the %d x %d grid\n", who, a.isrc, a.jsrc, g.nprow, g.npcol);
}
// d: the DeviceMatrix as an n x n operand of the caller's matrix; kinds: the letters the direction takes ("" : none)
inline void require_matrix_conversion(const char* who, char kind, const char* kinds, const OperandDesc& d,
                                      const OperandDesc& g) {
  if (kinds[0] != 0 && !in_set(kind, kinds))
    fatal("[dlaf_mi355x] %s: bad kind '%c' (one of %s)\n", who, kind, kinds);
  if (g.m != d.m || g.n != d.n || g.mb != d.mb || g.nb != d.nb || g.isrc != d.isrc || g.jsrc != d.jsrc)
    fatal("[dlaf_mi355x] %s: the matrix (%ld x %ld, block %d, source %d,%d) and the general matrix (%ld x %ld, block %d x "
          "%d, source %d,%d) differ\n", who, d.m, d.n, d.nb, d.isrc, d.jsrc, g.m, g.n, g.mb, g.nb, g.isrc, g.jsrc);
}

// ---- the prologue of a ScaLAPACK argument list: every operand as (name letter, desc, row offset, column offset)
struct ScalapackOperand {
  char name;
  const int* desc;
  int i, j;
};
// "ia, ja, ib, jb": the offsets the call takes
inline std::string offset_names(std::initializer_list<ScalapackOperand> ops) {
  std::string s;
  for (const ScalapackOperand& o : ops) {
    const char l = (char) (o.name | 0x20);
    s += std::string(s.empty() ? "" : ", ") + 'i' + l + ", j" + l;
  }
  return s;
}
// "A", "A and B", "A, B and Z"
inline std::string operand_names(std::initializer_list<ScalapackOperand> ops) {
  std::string s;
  size_t k = 0;
  for (const ScalapackOperand& o : ops)
    s += std::string(k++ == 0 ? "" : k == ops.size() ? " and " : ", ") + o.name;
  return s;
}
// dtype 1 (src/c_api/factorization/cholesky.h:65-75), all offsets 1, one context; returns the context
inline int require_scalapack_args(std::initializer_list<ScalapackOperand> ops, const char* who = nullptr) {
  const std::string pre = who ? std::string(who) + ": " : "";
  for (const ScalapackOperand& o : ops)
    if (o.desc[0] != 1)
      fatal("[dlaf_mi355x] %sdesc[0] (dtype) must be 1\n", pre.c_str());
  for (const ScalapackOperand& o : ops)
    if (o.i != 1 || o.j != 1)
      fatal("[dlaf_mi355x] %s%s must be 1\n", pre.c_str(), offset_names(ops).c_str());
  const int ctx = ops.begin()->desc[1];
  std::string all;
  for (const ScalapackOperand& o : ops)
    all += (all.empty() ? "" : ", ") + std::to_string(o.desc[1]);
  for (const ScalapackOperand& o : ops)
    if (o.desc[1] != ctx)
      fatal("[dlaf_mi355x] %s%s live on different contexts (%s)\n", pre.c_str(), operand_names(ops).c_str(), all.c_str());
  return ctx;
}

#pragma GCC visibility pop
}  // namespace dlaf_mi355x
