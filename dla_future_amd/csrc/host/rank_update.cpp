// rank_update.cpp -- the Hermitian rank-k and rank-2k updates (xSYRK / xHERK, xSYR2K / xHER2K) of the uplo triangle
// of C on a kernel that keeps a block of C in its accumulators over the k dimension (kernels_herk.hip):
//        herk  : C = alpha A A^H + beta C (trans N)            alpha A^H A + beta C (trans C)
//        her2k : C = alpha A B^H + conj(alpha) B A^H + beta C  alpha A^H B + conj(alpha) B^H A + beta C
//        weighted herk : C = alpha A D A^H + beta C (trans N)    alpha A^H D A + beta C (trans C),  D a real diagonal
// alpha of herk and every beta are real.  BLAS semantics: the other triangle of C is never referenced; the imaginary
// part of C's diagonal is ignored on entry and exactly 0 on exit; beta == 0: C is not read; alpha == 0 or k == 0: A and
// B are not referenced; then with beta == 1 nothing at all is touched.
//
// Reference: the herk / her2k tile calls of dlaf::cholesky_factorization and generalized_to_standard
// (factorization/cholesky/impl.h, eigensolver/gen_to_std/impl.h), which the reference never exposes as an algorithm.
//
// C is a DeviceMatrix (the operand of factorize(), gen_to_std and the eigensolvers): uplo U holds the plain transposed
// view, whose lower triangle is conj(C)'s -- the kernel updates it with conj(A), conj(B) and conj(alpha) (conj_view).
// One process: ONE launch over all the k tiles, both trans.  A grid (trans N only: the entries refuse the rest) runs
// SUMMA, one step per k tile l, nothing reduced:
//   column l of A        along the process rows from the owner column (bcast_view_column): the tiles A(i, l) of my
//                        local tile rows i of C
//   its transposed panel down the process columns, one broadcast per root process row
//                        (bcast_transposed_panel_whole): the tiles A(j, l) of my local tile columns j of C
//   (her2k: the same for B)
//   one launch with nk = 1 (first: l == 0)
// all of it on s_comm one step ahead, into rings of kBuf buffers.  A (and B) start on C's process row (the entries check).
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../device/herk_map.hpp"
#include "drivers.hpp"
#include "sweep.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

// Ad (and Bd, her2k; null: herk): the operands AS STORED, n x k (trans N) or k x n; nkt: the k tiles to multiply
// (0: k == 0 or alpha == 0 -- the triangle becomes beta C, Ad, Bd and d_host are not touched).
// d_host (herk only; null: the plain update): the k real weights of the weighted update C = alpha A D A^H + beta C, a
// HOST array, the same on every rank; uploaded once (k reals) into a pool workspace, the kernel multiplies them into the
// row operand on its way to LDS (launch_rank_k_weighted).  One process: one launch, the pointer at weight 0; a grid: the
// pointer advanced by l nb at step l.
template <class T>
void rank_update_canonical(DeviceMatrix<T>& C, TileMatrix<T>* Ad, TileMatrix<T>* Bd, const real_t<T>* d_host, bool trans_n,
                           long k, long nkt, T alpha, real_t<T> beta) {
  Grid* g = C.grid;
  Transport* tr = grid_transport(*g);
  const bool dist = g->nranks > 1;
  const bool two = Bd != nullptr;
  const size_t te = C.tile_elems;

  RankKArgs<T> ra;
  ra.c = C.tiles;
  ra.c_tsr = (long) te;
  ra.c_tsc = (long) (te * C.ltr);
  ra.x = ra.y = nullptr;
  ra.x_ts = ra.y_ts = ra.ks = 0;
  ra.trans = trans_n ? 'N' : 'C';
  ra.conj_view = C.transposed ? 1 : 0;
  ra.nk = 0;
  ra.k_last = 0;
  ra.ltr = (int) C.ltr;
  ra.ltc = (int) C.ltc;
  ra.nb = C.nb;
  ra.pr = C.rows.P;
  ra.ri = C.rows.shift();
  ra.pc = C.cols.P;
  ra.ci = C.cols.shift();
  ra.nt = (int) C.nt;
  ra.last = C.rows.last_extent();
  ra.alpha = alpha;
  ra.beta = beta;
  const bool work = C.ltr > 0 && C.ltc > 0;

  Sweep sw(false, false);
  const hipStream_t s_main = sw.s_main, s_comm = sw.s_comm;
  const bool weighted = d_host != nullptr && nkt > 0;
  PoolScope ws;
  const real_t<T>* dw = nullptr;
  if (weighted) {
    real_t<T>* w = ws.get<real_t<T>>((size_t) k);
    DLAF_HIP_CHECK(hipMemcpyAsync(w, d_host, (size_t) k * sizeof(real_t<T>), hipMemcpyHostToDevice, s_main));
    dw = w;
  }
  auto launch = [&] {
    if (weighted)
      launch_rank_k_weighted(ra, s_main);
    else
      launch_rank_k(ra, s_main);
  };
  if (nkt == 0 || !dist) {
    sw.begin(false);
    if (nkt > 0) {
      // tile (i, t) of a stored n x k matrix: rows next to each other; tile (t, i) of a stored k x n one: columns
      ra.x = ra.y = Ad->tiles;
      ra.x_ts = ra.y_ts = (long) (trans_n ? te : te * Ad->ltr);
      ra.ks = (long) (trans_n ? te * Ad->ltr : te);
      if (two)
        ra.x2 = ra.y2 = Bd->tiles;
      ra.nk = (int) nkt;
      ra.k_last = (trans_n ? Ad->cols : Ad->rows).last_extent();
      ra.kw = dw;
    }
    if (work)
      launch();
  }
  else {
    // in terms of the caller's C: its tile rows are spread like A's (the same axis), its tile columns over the
    // process columns
    const Axis& srow = Ad->rows;
    const Axis& scol = C.transposed ? C.rows : C.cols;
    const Axis& ka = Ad->cols;
    const bool hop = srow.P > 1;  // the transposed panel travels; else every tile of the column panel is here
    StepPipeline pipe(nkt);
    const size_t rp = (size_t) Ad->ltr * te, cp = (size_t) (scol.local_tiles() + srow.P) * te;
    Ring<T> arow(rp, ka.P > 1), acol(cp, hop), brow(rp, two && ka.P > 1), bcol(cp, two && hop);
    struct StepOperands {
      PanelPair<T> a, b;
    };
    std::vector<StepOperands> sop((size_t) nkt);
    auto fetch = [&](long l, int buf) {
      StepOperands& o = sop[(size_t) l];
      o.a = bcast_column_and_transposed_panel(tr, *Ad, l, srow, scol, arow[buf], acol[buf], s_comm);
      if (two)
        o.b = bcast_column_and_transposed_panel(tr, *Bd, l, srow, scol, brow[buf], bcol[buf], s_comm);
    };
    auto apply = [&](long l) {
      if (work) {
        const StepOperands& o = sop[(size_t) l];
        // the view's rows are C's rows (uplo L) or C's columns (uplo U: the transposed view)
        const Panel<T>& px = C.transposed ? o.a.col : o.a.row;
        const Panel<T>& py = C.transposed ? o.a.row : o.a.col;
        ra.x = px.base;
        ra.x_ts = px.ts;
        ra.x_ts2 = px.ts2;
        ra.x_period = px.period;
        ra.y = py.base;
        ra.y_ts = py.ts;
        ra.y_ts2 = py.ts2;
        ra.y_period = py.period;
        if (two) {
          ra.x2 = (C.transposed ? o.b.col : o.b.row).base;
          ra.y2 = (C.transposed ? o.b.row : o.b.col).base;
        }
        ra.ks = 0;
        ra.nk = 1;
        ra.k_last = ka.tile_extent(l);
        ra.first = l == 0 ? 1 : 0;
        ra.kw = weighted ? dw + l * C.nb : nullptr;
        launch();
      }
    };
    pipe.run(sw, fetch, apply);
  }
  const double ms = sw.finish();
  ws.release();
  // whole-grid algorithmic flops: k n (n + 1) per product (x4 complex)
  multiplication_set_profile(ms, (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (two ? 2.0 : 1.0) * (double) k * (double) C.n *
                                     (double) (C.n + 1));
}

}  // namespace

template <class T>
int hermitian_rank_update_host(Grid* g, char uplo, char trans, T alpha, HostOperand<const T> a,
                               const HostOperand<const T>* b, real_t<T> beta, HostOperand<T> c, const real_t<T>* d) {
  if (c.n == 0)
    return 0;
  const bool tn = herk_trans_is_n(trans);
  const long k = tn ? a.n : a.m;
  const int nb = c.nb;
  const bool product = k > 0 && !is_zero(alpha);
  if (!product && beta == real_t<T>(1))
    return 0;  // quick return: C is untouched, the imaginary parts of its diagonal included
  (void) checked_transport(*g);
  ScratchStream s;  // before the matrices: destroyed after them
  DeviceMatrix<T> Cd;
  Cd.create(g, uplo, c.n, nb, c.isrc, c.jsrc);
  TileMatrix<T> Ad, Bd;
  if (product) {
    Ad.create(g, false, a.m, a.n, nb, a.isrc, a.jsrc);
    Ad.upload(a.p, a.ld, false, false, T{}, s);
    if (b) {
      Bd.create(g, false, b->m, b->n, nb, b->isrc, b->jsrc);
      Bd.upload(b->p, b->ld, false, false, T{}, s);
    }
    s.sync();
  }
  const bool read_c = beta != real_t<T>(0);  // beta = 0: C is not read
  if (read_c)
    Cd.upload(c.p, c.ld);
  rank_update_canonical<T>(Cd, product ? &Ad : nullptr, (product && b) ? &Bd : nullptr, product ? d : nullptr, tn, k,
                           product ? (k + nb - 1) / nb : 0, alpha, beta);
  Cd.download(c.p, c.ld, read_c);
  return 0;
}

// The same on RESIDENT operands (arguments judged by the entry, c_api_device.cpp): C a DeviceMatrix whose stored triangle
// is uplo, A (and B; null: herk) general resident matrices.  alpha: real_t<T> for herk, T for her2k; beta: real_t<T>.
int hermitian_rank_update_device(char trans, const void* alpha, MatrixBase* a, MatrixBase* b, const void* beta,
                                 MatrixBase* c, const void* d) {
  const char* who = b ? "hermitian rank-2k update" : (d ? "hermitian weighted rank-k update" : "hermitian rank-k update");
  if (!a || !c || a->type != c->type || (b && b->type != c->type))
    fatal("[dlaf_mi355x] %s: operands of different element types\n", who);
  return dispatch_type(c->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    using R = real_t<T>;
    auto& A = static_cast<GeneralMatrix<T>&>(*a);
    auto* B = b ? &static_cast<GeneralMatrix<T>&>(*b) : nullptr;
    auto& C = static_cast<DeviceMatrix<T>&>(*c);
    if (A.m.grid != C.grid || (B && B->m.grid != C.grid))
      fatal("[dlaf_mi355x] %s: the operands live on different grids\n", who);
    if (C.n == 0)
      return 0;
    T al{};
    if (b)
      al = *static_cast<const T*>(alpha);
    else if constexpr (TypeInfo<T>::is_complex)
      al = T{*static_cast<const R*>(alpha), R(0)};
    else
      al = *static_cast<const R*>(alpha);
    const R be = *static_cast<const R*>(beta);
    const bool tn = herk_trans_is_n(trans);
    const long k = tn ? A.cols_g : A.rows_g;
    const bool product = k > 0 && !is_zero(al);
    if (!product && be == R(1))
      return 0;
    rank_update_canonical<T>(C, product ? &A.m : nullptr, (product && B) ? &B->m : nullptr,
                             product ? static_cast<const R*>(d) : nullptr, tn, k, product ? (k + C.nb - 1) / C.nb : 0, al,
                             be);
    return 0;
  });
}

// The weighted update on a resident C and the resident A `a` of which only the leading k columns (trans N) are
// multiplied -- the eigenvector matrix of a partial spectrum behind matrix_function.cpp, whose own k is all of them.
template <class T>
void hermitian_weighted_update_resident(DeviceMatrix<T>& C, TileMatrix<T>& A, const real_t<T>* d_host, long k, T alpha,
                                        real_t<T> beta) {
  const bool product = k > 0 && !is_zero(alpha);
  rank_update_canonical<T>(C, product ? &A : nullptr, nullptr, product ? d_host : nullptr, true, k,
                           product ? (k + C.nb - 1) / C.nb : 0, alpha, beta);
}

#define DLAF_RANK_UPDATE_INST(T)                                                                                     \
  template int hermitian_rank_update_host<T>(Grid*, char, char, T, HostOperand<const T>, const HostOperand<const T>*, \
                                             real_t<T>, HostOperand<T>, const real_t<T>*);                            \
  template void hermitian_weighted_update_resident<T>(DeviceMatrix<T>&, TileMatrix<T>&, const real_t<T>*, long, T,    \
                                                      real_t<T>);
DLAF_RANK_UPDATE_INST(float)
DLAF_RANK_UPDATE_INST(double)
DLAF_RANK_UPDATE_INST(cfloat)
DLAF_RANK_UPDATE_INST(cdouble)
#undef DLAF_RANK_UPDATE_INST

}  // namespace dlaf_mi355x
