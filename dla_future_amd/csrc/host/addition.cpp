// addition.cpp -- C = beta C + alpha op(A) on the uplo part of an m x n matrix (PBLAS p?geadd / p?tradd, p?tran / p?tranu /
// p?tranc, ScaLAPACK p?lacpy), the completion of a Hermitian / symmetric matrix from one triangle, and the resident
// conversions between a DeviceMatrix (one triangle) and a general resident matrix, all on one memory-bound kernel
// (kernels_geadd.hip; index arithmetic: geadd_map.hpp).
//
// Semantics.  uplo A: every element, L: i >= j, U: i <= j (for m != n the trapezoids of xLACPY).  Outside the uplo part
// C stays bit for bit, and so do the padding rows of its leading dimension.  A is only read.  beta == 0: C is not read
// (NaNs in it do not survive).  alpha == 0: A is not referenced (NaNs in it reach nothing); with beta == 1 nothing at all
// is touched.  alpha == 1 and beta == 0 with op N or T: the result is a BIT COPY of the source elements -- signed zeros,
// denormals and NaN payloads are moved, not multiplied (op C flips the sign bit of the imaginary part and nothing else).
// m == 0 or n == 0 returns before the GPU is touched.  hermitian_complete writes the OTHER triangle from the uplo one:
// kind H conjugates the mirror and stores the diagonal's imaginary parts as exactly 0 (the convention of
// hermitian_rank_k_update), kind S transposes plainly and leaves the diagonal alone bit for bit.
//
// Reference: the reference has no such algorithm; its matrix::copy (matrix/copy.h) is the alpha = 1, beta = 0, op N case.
//
// One process: ONE launch over every local tile, whatever the op.  op N on a grid is the same launch on the local part:
// A starts on C's source process (the entries check), so both hold the same elements and no byte moves.  op T / C and
// hermitian_complete on a P x Q grid walk the tile columns k of A (n x m for an m x n C); for each k
//   column k of A         along the process rows from the owner column (bcast_view_column): the tiles A(j, k) of my
//                         local tile rows j of A
//   its transposed panel  down the process columns, one broadcast per root process row (bcast_transposed_panel_whole,
//                         have = A's rows, want = C's columns): the tiles A(j, k) of my local tile COLUMNS j of C
//   one launch            on the process row that owns tile row k of C, over that row, reading the panel buffer
// on s_comm one step ahead, into rings of kBuf buffers.  Each tile so reaches P + Q processes and one of them consumes
// it: the price of having broadcasts only (transport.hpp has no point-to-point), accepted here.
// hermitian_complete is the same walk with A = C: the columns go in DESCENDING order for uplo L and ascending for uplo U,
// so that the tile row a step writes holds no tile of a column that is still to be broadcast.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../device/geadd_map.hpp"
#include "drivers.hpp"
#include "sweep.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

double g_add_ms = 0, g_add_bytes = 0;

bool op_is_n(char op) {
  return op == 'N' || op == 'n';
}
bool op_is_c(char op) {
  return op == 'C' || op == 'c';
}
int mask_of_uplo(char uplo) {
  return (uplo == 'L' || uplo == 'l') ? kGeaddLowerEq : (uplo == 'U' || uplo == 'u') ? kGeaddUpperEq : kGeaddAll;
}
// elements of the part of an m x n matrix
double part_elements(int mask, long m, long n) {
  auto lower_eq = [](long r, long c) {
    const long k = std::min(r, c);
    return (double) k * (double) r - (double) k * (double) (k - 1) / 2;
  };
  const double diag = (double) std::min(m, n);
  switch (mask) {
    case kGeaddLowerEq: return lower_eq(m, n);
    case kGeaddUpperEq: return lower_eq(n, m);
    case kGeaddLower: return lower_eq(m, n) - diag;
    case kGeaddUpper: return lower_eq(n, m) - diag;
    default: return (double) m * (double) n;
  }
}

// the launch arguments every field of which follows from the destination D (a TileMatrix or a DeviceMatrix: its VIEW)
template <class T, class M>
GeaddArgs<T> dest_args(const M& d) {
  GeaddArgs<T> a{};
  a.c = d.tiles;
  a.c_tsr = (long) d.tile_elems;
  a.c_tsc = (long) (d.tile_elems * d.ltr);
  a.g.ltr = (int) d.ltr;
  a.g.ltc = (int) d.ltc;
  a.g.nb = d.nb;
  a.g.rows = d.rows.local_size();
  a.g.cols = d.cols.local_size();
  a.g.pr = d.rows.P;
  a.g.ri = d.rows.shift();
  a.g.pc = d.cols.P;
  a.g.ci = d.cols.shift();
  a.g.il0 = 0;
  a.g.nil = (int) d.ltr;
  a.alpha = a.beta = T{};
  return a;
}
template <class T>
void set_scalars(GeaddArgs<T>& a, T alpha, T beta) {
  a.alpha = alpha;
  a.beta = beta;
  a.arith = geadd_arith(is_zero(alpha), is_one(alpha), is_zero(beta));
}
// the source tiles as stored, read straight (tile (il, jl)) or transposed (tile (jl, il)); sltr: local tile rows of it
template <class T>
void set_local_source(GeaddArgs<T>& a, const T* src, long sltr, size_t te, bool trans) {
  a.a = src;
  a.trans = trans ? 1 : 0;
  a.a_tsi = (long) (trans ? te * sltr : te);
  a.a_ts = (long) (trans ? te : te * sltr);
  a.a_ts2 = 0;
  a.a_period = 1;
}
template <class T>
void launch(GeaddArgs<T>& a, hipStream_t s) {
  a.ve = geadd_vector_elems((int) sizeof(T), a.g.nb, (unsigned long long) a.a, (unsigned long long) a.c);
  launch_geadd(a, s);
}

// The walk over the tile columns of A on a grid (header): C's tile row k = op(column k of A); proto: the launch
// arguments of C with mask, conj, diag_real and the scalars set.  A and C may be the same matrix (descending: see the
// header).  Everything is issued on sw's streams; the caller closes the window.
template <class T>
void transposed_walk(Sweep& sw, TileMatrix<T>& C, TileMatrix<T>& A, GeaddArgs<T> proto, bool descending) {
  Transport* tr = grid_transport(*C.grid);
  const size_t te = C.tile_elems;
  const long nkt = A.cols.nt();
  const Axis& have = A.rows;
  const Axis& want = C.cols;
  StepPipeline pipe(nkt);
  // the transposed panel travels when A's rows are spread; else every tile of the column panel is here
  Ring<T> arow((size_t) A.ltr * te, A.cols.P > 1), acol((size_t) (want.local_tiles() + have.P) * te, have.P > 1);
  std::vector<Panel<T>> panel((size_t) nkt);
  auto column_of = [&](long s) { return descending ? nkt - 1 - s : s; };
  auto fetch = [&](long s, int buf) {
    panel[(size_t) s] =
        bcast_column_and_transposed_panel(tr, A, column_of(s), have, want, arow[buf], acol[buf], sw.s_comm).col;
  };
  proto.trans = 1;
  proto.a_tsi = 0;
  proto.g.nil = 1;
  auto apply = [&](long s) {
    const long k = column_of(s);
    if (C.rows.mine(k) && C.ltc > 0) {
      const Panel<T>& p = panel[(size_t) s];
      GeaddArgs<T> a = proto;
      a.g.il0 = (int) C.rows.local_of(k);
      a.a = p.base;
      a.a_ts = p.ts;
      a.a_ts2 = p.ts2;
      a.a_period = p.period;
      launch(a, sw.s_main);
    }
  };
  pipe.run(sw, fetch, apply);
}

void set_profile(double ms, int mask, long m, long n, size_t elem, int arith, bool in_place_half) {
  g_add_ms = ms;
  const double e = part_elements(mask, m, n) * (double) elem;
  g_add_bytes = e * ((geadd_reads_a(arith) ? 1 : 0) + 1 + (geadd_reads_c(arith) && !in_place_half ? 1 : 0));
}

// C = beta C + alpha op(A) on resident tiles; A null: alpha == 0
template <class T>
void addition_canonical(TileMatrix<T>& C, TileMatrix<T>* A, char op, int mask, T alpha, T beta) {
  Grid* g = C.grid;
  const bool dist = g->nranks > 1;
  GeaddArgs<T> a = dest_args<T>(C);
  set_scalars(a, A ? alpha : T{}, beta);
  a.mask = mask;
  a.conj = op_is_c(op) ? 1 : 0;
  const bool trans = A && !op_is_n(op);
  Sweep sw(false, false);
  if (!trans || !dist) {
    sw.begin(false);
    if (A)
      set_local_source(a, A->tiles, A->ltr, C.tile_elems, trans);
    if (C.ltr > 0 && C.ltc > 0)
      launch(a, sw.s_main);
  }
  else {
    transposed_walk(sw, C, *A, a, false);
  }
  set_profile(sw.finish(), mask, C.rows.n, C.cols.n, sizeof(T), a.arith, false);
}

// the other triangle of the square G from the `upper_stored ? upper : lower` one, in place
template <class T>
void complete_canonical(TileMatrix<T>& G, bool upper_stored, bool herm) {
  GeaddArgs<T> a = dest_args<T>(G);
  a.arith = kGeaddCopy;
  // H writes the diagonal too (imaginary part 0), S leaves it alone
  a.mask = herm ? (upper_stored ? kGeaddLowerEq : kGeaddUpperEq) : (upper_stored ? kGeaddLower : kGeaddUpper);
  a.conj = herm ? 1 : 0;
  a.diag_real = herm ? 1 : 0;
  Sweep sw(false, false);
  if (G.grid->nranks == 1) {
    sw.begin(false);
    set_local_source(a, G.tiles, G.ltr, G.tile_elems, true);
    if (G.ltr > 0 && G.ltc > 0)
      launch(a, sw.s_main);
  }
  else {
    transposed_walk(sw, G, G, a, !upper_stored);
  }
  set_profile(sw.finish(), kGeaddLower, G.rows.n, G.cols.n, sizeof(T), kGeaddCopy, true);
}

}  // namespace

void addition_last_profile(double* ms, double* bytes) {
  *ms = g_add_ms;
  *bytes = g_add_bytes;
}

template <class T>
int general_addition_host(Grid* g, char uplo, char op, T alpha, HostOperand<const T> a, T beta, HostOperand<T> c) {
  if (c.m == 0 || c.n == 0)
    return 0;
  const bool use_a = !is_zero(alpha);
  if (!use_a && is_one(beta))
    return 0;  // quick return: nothing is touched
  (void) checked_transport(*g);
  const int mask = mask_of_uplo(uplo);
  ScratchStream s;  // before the matrices: destroyed after them
  TileMatrix<T> Ad, Cd;
  Cd.create(g, false, c.m, c.n, c.nb, c.isrc, c.jsrc);
  if (use_a) {
    Ad.create(g, false, a.m, a.n, c.nb, a.isrc, a.jsrc);
    Ad.upload(a.p, a.ld, false, false, T{}, s);
  }
  // beta = 0: the part of C is not read; what lies outside the part travels there and back unchanged
  if (!is_zero(beta) || mask != kGeaddAll)
    Cd.upload(c.p, c.ld, false, false, T{}, s);
  s.sync();
  addition_canonical<T>(Cd, use_a ? &Ad : nullptr, op, mask, alpha, beta);
  Cd.download(c.p, c.ld, false, s);
  s.sync();
  return 0;
}

// The same on two RESIDENT general matrices (arguments judged by the entry, c_api_device.cpp); a == c: op N in place.
int general_addition_device(char uplo, char op, const void* alpha, MatrixBase* a, const void* beta, MatrixBase* c) {
  if (!a || !c || a->type != c->type)
    fatal("[dlaf_mi355x] general addition: operands of different element types\n");
  return dispatch_type(c->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto& A = static_cast<GeneralMatrix<T>&>(*a);
    auto& C = static_cast<GeneralMatrix<T>&>(*c);
    if (A.m.grid != C.m.grid)
      fatal("[dlaf_mi355x] general addition: the operands live on different grids\n");
    if (C.rows_g == 0 || C.cols_g == 0)
      return 0;
    const T al = *static_cast<const T*>(alpha), be = *static_cast<const T*>(beta);
    const bool use_a = !is_zero(al);
    if (!use_a && is_one(be))
      return 0;
    addition_canonical<T>(C.m, use_a ? &A.m : nullptr, op, mask_of_uplo(uplo), al, be);
    return 0;
  });
}

template <class T>
int hermitian_complete_host(Grid* g, char uplo, char kind, HostOperand<T> a) {
  if (a.n == 0)
    return 0;
  (void) checked_transport(*g);
  ScratchStream s;  // before the matrices: destroyed after them
  TileMatrix<T> Ad;
  Ad.create(g, false, a.n, a.n, a.nb, a.isrc, a.jsrc);
  Ad.upload(a.p, a.ld, false, false, T{}, s);
  s.sync();
  complete_canonical<T>(Ad, uplo_is_upper(uplo), kind == 'H' || kind == 'h');
  Ad.download(a.p, a.ld, false, s);
  s.sync();
  return 0;
}

int hermitian_complete_device(char uplo, char kind, MatrixBase* a) {
  if (!a)
    fatal("[dlaf_mi355x] hermitian complete: no matrix\n");
  return dispatch_type(a->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto& A = static_cast<GeneralMatrix<T>&>(*a);
    if (A.rows_g == 0)
      return 0;
    complete_canonical<T>(A.m, uplo_is_upper(uplo), kind == 'H' || kind == 'h');
    return 0;
  });
}

// DeviceMatrix <-> general resident matrix (same grid, order, block and source process: the entry checks).  A
// DeviceMatrix created with uplo U holds the plain transposed view; a transposed view of a block-cyclic matrix stays on
// its process, so both directions are local launches on every grid -- transposing ones for uplo U.
namespace {
template <class T>
void triangle_between(DeviceMatrix<T>& D, GeneralMatrix<T>& G, bool to_general, hipStream_t s) {
  const size_t te = D.tile_elems;
  if (to_general) {
    GeaddArgs<T> a = dest_args<T>(G.m);
    a.arith = kGeaddCopy;
    a.mask = D.transposed ? kGeaddUpperEq : kGeaddLowerEq;
    set_local_source(a, D.tiles, D.ltr, te, D.transposed);
    if (G.m.ltr > 0 && G.m.ltc > 0)
      launch(a, s);
  }
  else {
    // in the coordinates of D's view the stored triangle is always the lower one
    GeaddArgs<T> a = dest_args<T>(D);
    a.arith = kGeaddCopy;
    a.mask = kGeaddLowerEq;
    set_local_source(a, G.m.tiles, G.m.ltr, te, D.transposed);
    if (D.ltr > 0 && D.ltc > 0)
      launch(a, s);
  }
}
}  // namespace

int matrix_to_general(char kind, MatrixBase* m, MatrixBase* gm) {
  return dispatch_type(m->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto& D = static_cast<DeviceMatrix<T>&>(*m);
    auto& G = static_cast<GeneralMatrix<T>&>(*gm);
    if (D.n == 0)
      return 0;
    const bool tri = kind == 'T' || kind == 't';
    double ms = 0;
    {
      Sweep sw(false, false);
      sw.begin(false);
      triangle_between(D, G, true, sw.s_main);
      if (tri) {
        // exact zeros in the other triangle
        GeaddArgs<T> z = dest_args<T>(G.m);
        z.arith = kGeaddZero;
        z.mask = D.transposed ? kGeaddLower : kGeaddUpper;
        if (G.m.ltr > 0 && G.m.ltc > 0)
          launch(z, sw.s_main);
      }
      ms = sw.finish();
    }
    if (!tri) {
      complete_canonical<T>(G.m, D.transposed, kind == 'H' || kind == 'h');
      ms += g_add_ms;
    }
    // the triangle read and written, the other one written (and, completing, the first read once more)
    g_add_ms = ms;
    g_add_bytes = (double) D.n * (double) D.n * sizeof(T) * (tri ? 1.5 : 2.0);
    return 0;
  });
}

int matrix_from_general(MatrixBase* m, MatrixBase* gm) {
  return dispatch_type(m->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto& D = static_cast<DeviceMatrix<T>&>(*m);
    auto& G = static_cast<GeneralMatrix<T>&>(*gm);
    if (D.n == 0)
      return 0;
    Sweep sw(false, false);
    sw.begin(false);
    triangle_between(D, G, false, sw.s_main);
    g_add_ms = sw.finish();
    g_add_bytes = (double) D.n * (double) D.n * sizeof(T);
    return 0;
  });
}

#define DLAF_ADDITION_INST(T)                                                                               \
  template int general_addition_host<T>(Grid*, char, char, T, HostOperand<const T>, T, HostOperand<T>);     \
  template int hermitian_complete_host<T>(Grid*, char, char, HostOperand<T>);
DLAF_ADDITION_INST(float)
DLAF_ADDITION_INST(double)
DLAF_ADDITION_INST(cfloat)
DLAF_ADDITION_INST(cdouble)
#undef DLAF_ADDITION_INST

}  // namespace dlaf_mi355x
