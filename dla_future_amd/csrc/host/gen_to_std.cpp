// gen_to_std.cpp -- reduction of the Hermitian generalized eigenproblem to standard form,
//        A  <-  L^-1 A L^-H   (uplo = L)         A  <-  U^-H A U^-1   (uplo = U),
// with the Cholesky factor of B (LAPACK xHEGST itype 1).
//
// Reference: dlaf::eigensolver::internal::generalized_to_standard (include/dlaf/eigensolver/gen_to_std.h:50,
// :101), GenToStd::call_L local (eigensolver/gen_to_std/impl.h:222-283) and distributed (:286-...), tile ops
// hegst (lapack/tile.h:209-218), trsm, hemm, her2k, gemm (blas/tile.h).  Per step k the reference issues
//   (1) hegst of the diagonal tile, (2) panel trsm + hemm, (3) her2k / 2 gemm on every trailing tile,
//   (4) hemm on the panel again, (5) a left triangular solve of the panel with the trailing part of L,
// one tile task at a time.
//
// MI355X design -- the kernels of the Cholesky path, grouped launches, two phases:
//   Phase I, step k = (1)-(4):
//     * the diagonal tile goes through two passes of the panel-TRSM kernel on its full Hermitian image
//       (D <- D L^-H, then the same on D^H: L^-1 D L^-H = ((D L^-H)^H L^-H)^H);
//     * panel: TRSM kernel, then "hemm" as one rectangular update launch against 0.5 * D (full image);
//     * trailing matrix: ONE two-segment update launch per step,
//           C -= [A_ik | L_ik] [L_jk | A_jk]^H  =  A_ik L_jk^H + L_ik A_jk^H      (K = 2 nb),
//       the her2k of the diagonal tiles being the same product under the triangle mask;
//   Phase II = (5) for ALL columns at once.  Step (5) of column k reads only L and column k after its step
//     (4), and nothing reads column k afterwards, so it can be deferred; deferred, it is the block forward
//     substitution  L X = strictly-block-lower(A)  swept by tile ROWS:
//           R_j <- L_jj^-1 R_j (R_j = tile row j left of the diagonal),   A(i, :) -= L_ij R_j  for i > j,
//     i.e. per row j one panel TRSM on the transposed tiles of R_j and one rectangular update over all the
//     rows below -- the launch shapes of the Cholesky trailing update instead of a chain of tile solves.
//   uplo = U runs on the transposed view like the Cholesky (B^T = L'^-1 A^T L'^-H with L' = U^T).
// Communication per step (process grids): L_kk (+ inverse blocks, + 0.5 D) down the owning process column,
// the A and L column panels along process rows, their transposed panels down process columns (one broadcast
// per root row each); Phase II: L_jj along the process row, the solved row down process columns, the L
// column panel along process rows.  One process: the diagonal tile / panel chain of step k+1 (Phase II: the solve of
// row j+1) runs on a side stream beside the trailing update of step k, which takes the next column (row) first; on a
// grid everything is stream-ordered on one stream.
#include <algorithm>
#include <cstdlib>

#include "drivers.hpp"
#include "launch_args.hpp"
#include "pool.hpp"
#include "sweep.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

// One process: lookahead.  The chain diagonal tile -> panel of step k+1 runs on a side stream beside the trailing
// update of step k, which takes column k+1 first and leaves `side_slots` workgroup slots free afterwards (the
// Cholesky's "sidecar" order, cholesky.cpp).  On a grid everything stays on one stream (the single panel workspaces
// are reused step by step).  Measured on MI355X (tools/run_hegst.sh, profiles/r03_gen_to_std_lookahead_ab.txt): NO
// gain -- fp64 N=16384 nb=512 44.8 (lookahead) vs 46.9 TFlop/s (one stream), N=32768 nb=1024 60.5 vs 61.3, z
// N=16384 nb=512 53.4 vs 52.7: on 32 slots the chain (two single-tile solves, panel solve, hemm) takes about as
// long as the trailing update it runs beside, and the update loses the slots.  The stage is bound by the nb = 512
// update rate and by 126 latency-bound solves of ~86 us per run (rocprofv3: update 84 %, TRSM 11 %).  So: opt-in,
// DLAF_MI355X_HEGST_LOOKAHEAD=1.
bool want_lookahead(bool dist) {
  const char* e = std::getenv("DLAF_MI355X_HEGST_LOOKAHEAD");
  return !dist && (e ? std::atoi(e) != 0 : false);
}

// One reduction of A with the factor L: its streams, workspaces and events, the operations the two phases are built
// of, and the phases.  Step k's diagonal tile / panel chain (Phase II: row j's solve) is issued on sp, everything
// else on s; sp == s unless the lookahead is on.
template <class T>
struct GenToStd {
  DeviceMatrix<T>& A;
  DeviceMatrix<T>& L;
  Transport* const tr;
  const bool dist;
  const Axis &rows, &cols;
  const long nt, ltr, ltc;
  const int nb;
  const size_t te, wel;
  // uplo == 'U' runs on the transposed view: its process rows are the caller's process columns
  const CommAxis ax_row, ax_col;
  int* const info;
  const bool lookahead;
  const long side_slots;  // workgroup slots the bulk launches leave to the side stream
  const hipStream_t s;
  hipStream_t sp;
  // workspaces: [L_kk | inverse diagonal blocks | 0.5 D] travel together down the process column; two of them and
  // two row buffers because the panel work of step k+1 runs beside the trailing update of step k (one process)
  DevBuf<T> dws2[2], dfull, xt, pA, pL, pAT, pLT, Tw2[2];
  DevBuf<unsigned> counters;
  Events ev_panel, ev_la;

  GenToStd(DeviceMatrix<T>& A_, DeviceMatrix<T>& L_, Transport* tr_)
      : A(A_), L(L_), tr(tr_), dist(A_.grid->nranks > 1), rows(A_.rows), cols(A_.cols), nt(A_.nt), ltr(A_.ltr),
        ltc(A_.ltc), nb(A_.nb), te(A_.tile_elems), wel(A_.winv_elems()),
        ax_row(A_.transposed ? CommAxis::Col : CommAxis::Row), ax_col(A_.transposed ? CommAxis::Row : CommAxis::Col),
        info(A_.info), lookahead(want_lookahead(dist)), side_slots(lookahead ? 32 : 0), s(A_.s_high), sp(A_.s_high),
        dfull(te), xt(te), pA((size_t) ltr * te), pL((size_t) ltr * te), pAT((size_t) (ltc + rows.P) * te),
        pLT((size_t) (ltc + rows.P) * te), counters(16), ev_panel((size_t) nt + 1), ev_la((size_t) nt + 1) {
    for (int i = 0; i < 2; ++i) {
      dws2[i].alloc(2 * te + wel);
      Tw2[i].alloc((size_t) std::max<long>(ltc, 1) * te);
    }
    if (lookahead) {
      int lo = 0, hi = 0;
      DLAF_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      DLAF_HIP_CHECK(hipStreamCreateWithPriority(&sp, hipStreamNonBlocking, hi));
    }
  }
  GenToStd(const GenToStd&) = delete;
  GenToStd& operator=(const GenToStd&) = delete;
  ~GenToStd() {
    if (sp != s)
      (void) hipStreamDestroy(sp);
  }

  // [L_kk | inverse blocks | 0.5 D] of step k (Phase II: of row k, without the last)
  T* Lkk(long k) const { return dws2[k & 1].p; }
  T* Wkk(long k) const { return dws2[k & 1].p + te; }
  T* Hs(long k) const { return dws2[k & 1].p + te + wel; }

  void after(hipStream_t waiter, hipEvent_t ev, hipStream_t recorder) {
    DLAF_HIP_CHECK(hipEventRecord(ev, recorder));
    if (waiter != recorder)
      DLAF_HIP_CHECK(hipStreamWaitEvent(waiter, ev, 0));
  }

  // X = B l^-H for `ntiles` tiles of rows_each x n at b, b + te, ...
  void trsm_tiles(T* b, long ntiles, int rows_each, const T* l, const T* w, int n, hipStream_t st) {
    if (ntiles <= 0)
      return;
    auto ta = tile_batch_args<TrsmArgs<T>>(b, (long) te, nb, ntiles, rows_each, l, nb, n);
    ta.winv = w;
    ta.info = info;
    ta.prio = (st != s) ? 1 : 0;
    launch_trsm(ta, st);
  }
  // reserve > 0: persistent form that leaves that many workgroup slots to the side stream
  void launch(const UpdateArgs<T>& ua, hipStream_t st, long reserve) {
    if (reserve > 0)
      launch_update(ua, st, 3, std::max<long>(8, A.bulk_slots - reserve), counters.p, false);
    else
      launch_update(ua, st, 3);
  }
  // C(il, jl) -= a(il) b(jl)^H over local tile rows [il0, il1) x local tile columns [jl0, jl1), every tile
  void rect_update(long il0, long il1, long jl0, long jl1, const T* a, const T* b, long b_ts, int K, hipStream_t st,
                   long reserve = 0) {
    if (il0 >= il1 || jl0 >= jl1 || K <= 0)
      return;
    launch(rect_update_args(A, il0, il1, jl0, jl1, a, b, b_ts, K, info), st, reserve);
  }

  // ================================================================================== Phase I
  // (1) diagonal tile: D <- L_kk^-1 D L_kk^-H  (lapack/tile.h:209-218 hegst)
  void diag_step(long k, hipStream_t st) {
    const int kb = rows.tile_extent(k);
    if (rows.rank == rows.owner(k) && cols.rank == cols.owner(k)) {
      const long klc = cols.local_of(k);
      T* akk = A.tile(rows.local_of(k), klc);
      DLAF_HIP_CHECK(hipMemcpyAsync(Lkk(k), L.tile(rows.local_of(k), klc), te * sizeof(T), hipMemcpyDeviceToDevice, st));
      launch_invert_diag_blocks(Lkk(k), nb, kb, Wkk(k), info, st, false, false);
      launch_tile_xform(dfull.p, (long) nb, 0, akk, (long) nb, 0, kb, kb, 1, 1, 1.0, st);    // full Hermitian image
      trsm_tiles(dfull.p, 1, kb, Lkk(k), Wkk(k), kb, st);                                    // D L^-H
      launch_tile_xform(xt.p, (long) nb, 0, dfull.p, (long) nb, 0, kb, kb, 1, 0, 1.0, st);   // (D L^-H)^H
      trsm_tiles(xt.p, 1, kb, Lkk(k), Wkk(k), kb, st);                                       // (L^-1 D L^-H)^H
      launch_tile_xform(akk, (long) nb, 0, xt.p, (long) nb, 0, kb, kb, 1, 2, 1.0, st);       // lower triangle back
      launch_tile_xform(Hs(k), (long) nb, 0, akk, (long) nb, 0, kb, kb, 1, 1, 0.5, st);      // 0.5 D, full image
    }
  }
  // (2) panel: A_ik <- A_ik L_kk^-H, then A_ik -= 0.5 L_ik D  (impl.h:236-240)
  void panel_step(long k, hipStream_t st) {
    const int kb = rows.tile_extent(k);
    const bool in_col = cols.rank == cols.owner(k);
    const long il_n = rows.next_local(k + 1);
    if (in_col && rows.P > 1)
      tr->bcast(ax_col, rows.owner(k), rows.rank, Lkk(k), Lkk(k), (2 * te + wel) * sizeof(T), st);
    if (in_col && il_n < ltr) {
      const long klc = cols.local_of(k);
      auto ta = panel_args<TrsmArgs<T>>(A, il_n, ltr, klc, Lkk(k), kb);
      ta.winv = Wkk(k);
      ta.info = info;
      ta.prio = (st != s) ? 1 : 0;
      launch_trsm(ta, st);
      rect_update(il_n, ltr, klc, klc + 1, L.tile(il_n, klc), Hs(k), 0, kb, st);
    }
  }

  // the operands of step k's trailing update
  struct Panels {
    long il_n, jl_n;       // first local row / column beyond k
    T *colA, *colL;        // column panels of A and L: the tile of local row il at + (il - il_n) * te
    const T *rowA, *rowL;  // their transposed panels: the tile of local column jl
    long b_ts, b_ts2;
    int b_period;
  };
  // panels of A and L along process rows, their transposes down process columns
  Panels fetch_panels(long k) {
    Panels p;
    const int own_c = cols.owner(k);
    const bool in_col = cols.rank == own_c;
    p.il_n = rows.next_local(k + 1);
    p.jl_n = cols.next_local(k + 1);
    const long klc = in_col ? cols.local_of(k) : -1;
    p.colA = in_col ? A.tile(p.il_n < ltr ? p.il_n : 0, klc) : pA.p;
    p.colL = in_col ? L.tile(p.il_n < ltr ? p.il_n : 0, klc) : pL.p;
    if (cols.P > 1 && p.il_n < ltr) {
      tr->bcast(ax_row, own_c, cols.rank, p.colA, p.colA, (size_t) (ltr - p.il_n) * te * sizeof(T), s);
      tr->bcast(ax_row, own_c, cols.rank, p.colL, p.colL, (size_t) (ltr - p.il_n) * te * sizeof(T), s);
    }
    p.b_ts = (long) te;
    p.b_ts2 = 0;
    p.b_period = 1;
    if (rows.P > 1) {
      A.bcast_transposed_panel(tr, ax_col, p.colA, p.il_n, p.jl_n, pAT.p, s, p.b_period, p.b_ts2);
      A.bcast_transposed_panel(tr, ax_col, p.colL, p.il_n, p.jl_n, pLT.p, s, p.b_period, p.b_ts2);
      p.rowA = pAT.p;
      p.rowL = pLT.p;
    }
    else {
      const long off = (cols.global_of(p.jl_n) - p.il_n) * (long) te;
      p.rowA = p.colA + off;
      p.rowL = p.colL + off;
      p.b_ts = (long) te * cols.P;
    }
    return p;
  }
  // (3) trailing matrix, local tile columns [j0, j1): C -= A_ik L_jk^H + L_ik A_jk^H  (her2k on the diagonal tiles)
  void trailing(const Panels& p, int kb, long j0, long j1, long reserve) {
    if (p.il_n >= ltr || j0 >= j1)
      return;
    const long il0 = std::max(p.il_n, rows.next_local(cols.global_of(j0)));
    if (il0 >= ltr)
      return;
    UpdateArgs<T> ua = update_args(A, il0, ltr, j0, j1, p.colA + (size_t) (il0 - p.il_n) * te, p.rowL, p.b_ts, 2 * kb, info);
    ua.a2 = p.colL + (size_t) (il0 - p.il_n) * te;
    ua.b2 = p.rowA;
    ua.b_period = p.b_period;
    ua.b_ts2 = p.b_ts2;
    ua.b_jl0 = (int) p.jl_n;
    ua.K1 = kb;
    ua.her2k = 1;
    launch(ua, s, reserve);
  }

  void phase_one() {
    diag_step(0, sp);
    if (nt > 1)
      panel_step(0, sp);
    after(s, ev_panel[0], sp);
    for (long k = 0; k + 1 < nt; ++k) {
      if (tr)
        tr->mark(k);
      const int kb = rows.tile_extent(k);
      const bool in_col = cols.rank == cols.owner(k);
      const Panels p = fetch_panels(k);
      // column k+1 first: what the diagonal tile and the panel of step k+1 need
      const long j_la = cols.mine(k + 1) ? p.jl_n + 1 : p.jl_n;
      trailing(p, kb, p.jl_n, j_la, 0);
      after(sp, ev_la[k], s);
      diag_step(k + 1, sp);
      if (k + 2 < nt)
        panel_step(k + 1, sp);
      trailing(p, kb, j_la, ltc, side_slots);
      // ---- (4) panel again: A_ik -= 0.5 L_ik D  (impl.h:263-266) -----------------------------------------
      if (in_col && p.il_n < ltr) {
        const long klc = cols.local_of(k);
        rect_update(p.il_n, ltr, klc, klc + 1, L.tile(p.il_n, klc), Hs(k), 0, kb, s);
      }
      after(s, ev_panel[k + 1], sp);
      if (dist)
        DLAF_HIP_CHECK(hipStreamSynchronize(s));  // single panel workspaces: reused by the next step
    }
  }

  // ================================================================================== Phase II
  // (5) for every column at once: L X = strictly-block-lower(A), swept by tile rows (impl.h:268-280).  Row j:
  // R_j <- L_jj^-1 R_j through the adjoint tiles Tw2[j & 1]; the rows below take it from there.
  void row_step(long j, hipStream_t st) {
    const int kbj = rows.tile_extent(j);
    const int own_r = rows.owner(j), own_c = cols.owner(j);
    const bool in_row = rows.rank == own_r, in_col = cols.rank == own_c;
    const long ncl = cols.next_local(j);  // local tile columns left of the diagonal
    T* Tw = Tw2[j & 1].p;
    if (in_row && in_col) {
      DLAF_HIP_CHECK(hipMemcpyAsync(Lkk(j), L.tile(rows.local_of(j), cols.local_of(j)), te * sizeof(T),
                                    hipMemcpyDeviceToDevice, st));
      launch_invert_diag_blocks(Lkk(j), nb, kbj, Wkk(j), info, st, false, false);
    }
    if (in_row && cols.P > 1)
      tr->bcast(ax_row, own_c, cols.rank, Lkk(j), Lkk(j), (te + wel) * sizeof(T), st);
    if (in_row && ncl > 0) {
      const long lr = rows.local_of(j);
      // R_j^H tile by tile: T_c = A(j, c)^H (nb x kbj);  T_c <- T_c L_jj^-H;  A(j, c) = T_c^H
      launch_tile_xform(Tw, (long) nb, (long) te, A.tile(lr, 0), (long) nb, (long) (te * ltr), kbj, nb, (int) ncl, 0, 1.0, st);
      trsm_tiles(Tw, ncl, nb, Lkk(j), Wkk(j), kbj, st);
      launch_tile_xform(A.tile(lr, 0), (long) nb, (long) (te * ltr), Tw, (long) nb, (long) te, nb, kbj, (int) ncl, 0, 1.0, st);
    }
  }

  void phase_two() {
    if (nt > 1) {
      after(sp, ev_la[nt - 1], s);  // Phase I is complete on both streams
      row_step(1, sp);
      after(s, ev_panel[nt], sp);
    }
    for (long j = 1; j < nt; ++j) {
      if (tr)
        tr->mark(nt + j);
      const int kbj = rows.tile_extent(j);
      const int own_r = rows.owner(j), own_c = cols.owner(j);
      const bool in_col = cols.rank == own_c;
      const long il_n = rows.next_local(j + 1);
      const long ncl = cols.next_local(j);
      T* Tw = Tw2[j & 1].p;
      if (rows.P > 1 && ncl > 0)
        tr->bcast(ax_col, own_r, rows.rank, Tw, Tw, (size_t) ncl * te * sizeof(T), s);
      T* colL = in_col ? L.tile(il_n < ltr ? il_n : 0, cols.local_of(j)) : pL.p;
      if (cols.P > 1 && il_n < ltr)
        tr->bcast(ax_row, own_c, cols.rank, colL, colL, (size_t) (ltr - il_n) * te * sizeof(T), s);
      // A(i, c) -= L_ij T_c^H = L_ij A(j, c)  for the rows below j, the columns left of j: row j+1 first (the next
      // row to be solved), the others beside that solve
      const long il_la = (j + 1 < nt && rows.mine(j + 1)) ? il_n + 1 : il_n;
      rect_update(il_n, il_la, 0, ncl, colL, Tw, (long) te, kbj, s);
      if (j + 1 < nt) {
        after(sp, ev_la[j], s);
        row_step(j + 1, sp);
      }
      rect_update(il_la, ltr, 0, ncl, colL + (size_t) (il_la - il_n) * te, Tw, (long) te, kbj, s, side_slots);
      if (j + 1 < nt)
        after(s, ev_panel[j + 1], sp);
      if (dist)
        DLAF_HIP_CHECK(hipStreamSynchronize(s));
    }
  }

  // waits for both streams; this process's own status word
  int finish() {
    int h = 0;
    DLAF_HIP_CHECK(hipMemcpyAsync(&h, info, sizeof(int), hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    if (sp != s)
      DLAF_HIP_CHECK(hipStreamSynchronize(sp));
    return h;
  }
};

}  // namespace

template <class T>
int gen_to_std_device(DeviceMatrix<T>& A, DeviceMatrix<T>& L) {
  if (A.grid != L.grid || A.n != L.n || A.nb != L.nb || A.ltr != L.ltr || A.ltc != L.ltc || A.transposed != L.transposed)
    fatal("[dlaf_mi355x] gen_to_std: A and the Cholesky factor differ in shape, uplo or distribution\n");
  Transport* tr = checked_transport(*A.grid);
  // work enqueued on the factor's streams (a cholesky_start without a wait) must be done before it is read here
  for (hipStream_t ls : {L.s_high, L.s_low, L.s_comm})
    if (ls != nullptr && ls != A.s_high)
      DLAF_HIP_CHECK(hipStreamSynchronize(ls));
  DLAF_HIP_CHECK(hipMemsetAsync(A.info, 0, sizeof(int), A.s_high));
  if (A.nt == 0)
    return 0;
  int h = 0;
  {
    GenToStd<T> g(A, L, tr);
    g.phase_one();
    g.phase_two();
    h = g.finish();
  }
  // the same value on every rank, as DeviceMatrix::wait() makes it for the factorization
  return agree_on_info(*A.grid, h);
}

// Host entry: a, l = this process's local column-major parts of A and of the Cholesky factor of B
template <class T>
int gen_to_std_host(Grid* g, char uplo, HostOperand<T> a, HostOperand<const T> l) {
  DeviceMatrix<T> A, Lm;
  A.create(g, uplo, a.n, a.nb, a.isrc, a.jsrc);
  Lm.create(g, uplo, l.n, l.nb, l.isrc, l.jsrc);
  A.upload(a.p, a.ld);
  Lm.upload(l.p, l.ld);
  const int r = gen_to_std_device(A, Lm);
  A.download(a.p, a.ld, true);
  return r;
}

#define INST(T)                                                     \
  template int gen_to_std_device<T>(DeviceMatrix<T>&, DeviceMatrix<T>&); \
  template int gen_to_std_host<T>(Grid*, char, HostOperand<T>, HostOperand<const T>);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
