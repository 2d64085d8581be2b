// solver.cpp -- distributed triangular solve  op(A) X = alpha B  /  X op(A) = alpha B  on the tile kernels
// of the Cholesky path.
//
// Reference: dlaf::triangular_solver (include/dlaf/solver/triangular.h:41-177) and its eight hand-written
// variants call_{L,R}{L,U}{N,T} (solver/triangular/impl.h), each with its own tile loop and communication
// pattern (broadcasts for the NoTrans variants, reductions for the transposed ones).
//
// MI355X design: ONE device algorithm, the one the Cholesky kernels already implement,
//
//        X * T^H = B        T triangular (lower: swept forward, upper: swept backward)
//
//   step k:  X(:,k)  = B(:,k) * T_kk^-H                  panel TRSM kernel (inverted diagonal blocks)
//            B(:,j) -= X(:,k) * T(j,k)^H   for j beyond k   grouped NT update kernel, rectangular mode
//
// and every side / uplo / op / diag / alpha combination is mapped onto it when the operands are laid out
// on the device (the relayout kernel transposes, conjugates and scales on the way):
//
//   Right, op = C :  X A^H = aB            T = A            B_dev = a B
//   Right, op = N :  X A   = aB            T = A^H          B_dev = a B
//   Right, op = T :  X A^T = aB            T = conj(A)      B_dev = a B
//   Left,  op = N :  A X   = aB  <=>  X^H A^H   = (aB)^H    T = A            B_dev = (a B)^H
//   Left,  op = C :  A^H X = aB  <=>  X^H A     = (aB)^H    T = A^H          B_dev = (a B)^H
//   Left,  op = T :  A^T X = aB  <=>  X^H conj(A) = (aB)^H  T = A^T          B_dev = (a B)^H
//
// A transposed view of a block-cyclic matrix needs no communication: tile (i,j) of the view is tile (j,i)
// of the caller's matrix and stays on the same process, with the roles of process rows and columns swapped
// (the same device the Cholesky uses for uplo = U).  Two communication shapes remain, depending on whether
// T's rows are spread over the same grid dimension as B_dev's columns ("aligned": one broadcast of T's
// column panel) or over the other one ("crossed": the Cholesky's panel + transposed-panel pair).  T's
// panels depend on A only, so they are broadcast one step ahead of the sweep.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "drivers.hpp"
#include "pool.hpp"
#include "sweep.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

// device time of the last sweep on this process (HIP events on the compute stream; relayout and PCIe excluded)
static double g_last_sweep_ms = 0;
static double g_last_sweep_flops = 0;

// X T^H = B in place on Bd; Td lower (swept forward) or upper (swept backward) triangular, unit: its
// diagonal is taken as 1.  Both operands on the same grid; Td's index distribution along the grid dimension
// it shares with Bd's columns must be the one of Bd's columns (checked by the caller).
template <class T>
void solve_canonical(TileMatrix<T>& Td, TileMatrix<T>& Bd, bool upper, bool unit) {
  Grid* g = Bd.grid;
  Transport* tr = grid_transport(*g);
  const bool dist = g->nranks > 1;
  const int nb = Bd.nb;
  const long nt = Bd.cols.nt();  // tiles along n
  if (nt == 0 || Bd.rows_global == 0)
    return;
  const size_t tile_elems = Bd.tile_elems;
  const size_t winv_elems = (size_t) ((nb + kDiagBlock - 1) / kDiagBlock) * kDiagBlock * kDiagBlock;
  check_t_aligned(Td, Bd, "triangular solver");

  Sweep sw(false, true);
  const hipStream_t s_main = sw.s_main, s_comm = sw.s_comm;
  int* const info = sw.info.p;
  Events ev_x((size_t) nt), ev_xb((size_t) nt), ev_free((size_t) nt), ev_prep(1);

  // ---- preparation: inverted 64 x 64 diagonal blocks of every local diagonal tile of Td ---------------
  std::vector<long> my_diag;  // global indices of the diagonal tiles I own
  for (long k = 0; k < nt; ++k)
    if (Td.rows.mine(k) && Td.cols.mine(k))
      my_diag.push_back(k);
  DevBuf<T> winv_all(my_diag.size() * winv_elems);
  std::vector<const T*> winv_of((size_t) nt, nullptr);
  DLAF_HIP_CHECK(hipMemsetAsync(winv_all.p, 0, std::max<size_t>(1, my_diag.size() * winv_elems) * sizeof(T), s_main));
  for (size_t q = 0; q < my_diag.size(); ++q) {
    const long k = my_diag[q];
    winv_of[(size_t) k] = winv_all.p + q * winv_elems;
    launch_invert_diag_blocks(Td.tile(Td.rows.local_of(k), Td.cols.local_of(k)), nb, Td.rows.tile_extent(k),
                              winv_all.p + q * winv_elems, info, s_main, upper, unit);
  }
  DLAF_HIP_CHECK(hipEventRecord(ev_prep[0], s_main));
  DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, ev_prep[0], 0));

  // the T operands of every step (and the global step order), the X panel on the processes that do not own it
  TOperandFetch<T> tf(Td, Bd, tr, upper, upper, s_comm, winv_of.data(), winv_elems);
  Ring<T> xpanel((size_t) Bd.ltr * tile_elems, dist);

  auto update = [&](long s, const T* xp, long j0, long j1) {
    const TOperand<T>& o = tf.top[(size_t) s];
    j0 = std::max(j0, o.jl0);
    j1 = std::min(j1, o.jl1);
    if (j0 >= j1 || Bd.ltr == 0)
      return;
    launch_update(rect_update_args(Bd, 0, Bd.ltr, j0, j1, xp, o.base + (j0 - o.jl0) * o.ts, o.ts,
                                   Bd.cols.tile_extent(tf.step_k(s)), info),
                  s_main, 3);
  };

  sw.begin(false);  // (the preparation stays outside the window; s_comm waits for ev_prep)

  // ---- the sweep --------------------------------------------------------------------------------------
  // s_main: TRSM(s) . U(s, next column) . TRSM(s+1) . U(s, the rest) . U(s+1, next column) ...  so that the
  // X panel of step s+1 is on the wire under the bulk of step s; T operands arrive one step ahead on s_comm
  tf.fetch(0);
  const T* xp_prev = nullptr;
  for (long s = 0; s < nt; ++s) {
    const long k = tf.step_k(s);
    if (s + 1 < nt) {
      wait_ring_free(s_comm, ev_free, s + 1);  // the buffers of step s + 1 - kBuf, T operands and X panel alike
      tf.fetch(s + 1);
    }
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, tf.ev_t[(size_t) s], 0));

    // column k of Bd: X(:,k) = B(:,k) T_kk^-H
    if (Bd.cols.mine(k) && Bd.ltr > 0) {
      auto ta = panel_args<TrsmArgs<T>>(Bd, 0, Bd.ltr, Bd.cols.local_of(k), tf.top[(size_t) s].diag, Bd.cols.tile_extent(k));
      ta.winv = tf.top[(size_t) s].winv;
      ta.info = info;
      ta.upper = upper ? 1 : 0;
      launch_trsm(ta, s_main);
    }
    DLAF_HIP_CHECK(hipEventRecord(ev_x[(size_t) s], s_main));

    // the solved panel to the other members of my Bd row
    if (Bd.cols.P > 1)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, ev_x[(size_t) s], 0));
    const T* xp = bcast_view_column(tr, Bd, k, xpanel[(int) (s % kBuf)], s_comm);
    if (Bd.cols.P > 1)
      DLAF_HIP_CHECK(hipEventRecord(ev_xb[(size_t) s], s_comm));

    // what is left of the previous step's update runs under that broadcast
    if (s >= 1) {
      const long kn = k;  // the "next column" of step s-1 is this step's column
      const long jn = Bd.cols.mine(kn) ? Bd.cols.local_of(kn) : -1;
      if (jn >= 0) {
        update(s - 1, xp_prev, 0, jn);
        update(s - 1, xp_prev, jn + 1, Bd.ltc);
      }
      else {
        update(s - 1, xp_prev, 0, Bd.ltc);
      }
      DLAF_HIP_CHECK(hipEventRecord(ev_free[(size_t) (s - 1)], s_main));
    }
    if (Bd.cols.P > 1)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, ev_xb[(size_t) s], 0));

    // lookahead: the column the next step solves
    if (s + 1 < nt) {
      const long kn = tf.step_k(s + 1);
      if (Bd.cols.mine(kn)) {
        const long jn = Bd.cols.local_of(kn);
        update(s, xp, jn, jn + 1);
      }
    }
    xp_prev = xp;
  }
  // the last step has nothing beyond it; its event only releases the buffers
  DLAF_HIP_CHECK(hipEventRecord(ev_free[(size_t) (nt - 1)], s_main));

  g_last_sweep_ms = sw.finish();
  // whole-grid algorithmic flops: rows x n^2 (x4 complex)
  g_last_sweep_flops = (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (double) Bd.rows_global * (double) Bd.cols.n * (double) Bd.cols.n;
}

}  // namespace

void solver_last_profile(double* ms, double* flops) {
  if (ms)
    *ms = g_last_sweep_ms;
  if (flops)
    *flops = g_last_sweep_flops;
}

// Host entry of a canonical sweep (the solve, or the multiplication of multiplication.cpp): a the triangular matrix, b
// the matrix B on the grid, overwritten by the result; both have passed require_triangular (api_checks.hpp).
// may_reverse: the one-process reversal of an upper T below is allowed (the solve).
template <class T>
int triangular_canonical_host(CanonicalSweep<T> sweep, bool may_reverse, Grid* g, char side, char uplo, char op, char diag,
                              T alpha, HostOperand<const T> a, HostOperand<T> b) {
  (void) checked_transport(*g);
  if (b.m == 0 || b.n == 0)
    return 0;
  const auto [left, a_upper, unit, t_transposed, t_conj, t_upper] = operand_map(side, uplo, op, diag);
  const long na = a.n;
  const int nb = a.nb;

  ScratchStream s;  // before the matrices: destroyed after them
  TileMatrix<T> Td, Bd;
  Td.create(g, t_transposed, na, na, nb, a.isrc, a.jsrc);
  // B's blocks: A's along the triangular dimension (its rows for side = Left), its own along the other
  Bd.create_rhs(g, left, b.m, b.n, b.mb, b.nb, b.isrc, b.jsrc);
  // One process, whole tiles: an upper triangular T (swept backward by the round-1 strips kernel) is laid out
  // REVERSED -- T'(i, j) = T(na-1-i, na-1-j) is lower triangular, X'(:, j) = X(:, na-1-j) solves X' T'^H = B' -- and
  // the forward sweep of the row-owner kernel does the work; the download reverses back.
  // DLAF_MI355X_SOLVER_REVERSE=0: the backward sweep (A/B).
  static const bool reverse_on = [] {
    const char* e = std::getenv("DLAF_MI355X_SOLVER_REVERSE");
    return e ? std::atoi(e) != 0 : true;
  }();
  const bool reversed = may_reverse && reverse_on && t_upper && g->nranks == 1 && na % nb == 0;
  if (reversed) {
    Td.rev_rows = Td.rev_cols = true;
    Bd.rev_cols = true;  // the view's columns are the triangular dimension
  }
  Td.upload(a.p, a.ld, t_conj, false, T{}, s);
  // Left: B_dev = (alpha B)^H = conj(alpha) B^H (the relayout conjugates first, then scales)
  Bd.upload(b.p, b.ld, left, true, left ? conj_of(alpha) : alpha, s);
  s.sync();
  sweep(Td, Bd, reversed ? false : t_upper, unit);
  Bd.download(b.p, b.ld, left, s);
  s.sync();
  return 0;
}

template <class T>
int triangular_solver_host(Grid* g, char side, char uplo, char op, char diag, T alpha, HostOperand<const T> a,
                           HostOperand<T> b) {
  return triangular_canonical_host<T>(solve_canonical<T>, true, g, side, uplo, op, diag, alpha, a, b);
}

// ================================================================================ device-resident operands
// A general m x n matrix resident in HBM in tile layout (the right-hand sides of a solve), behind an opaque handle.

MatrixBase* general_matrix_create(Grid* g, char type, long m, long n, int nb, int isrc, int jsrc) {
  runtime_init();
  (void) grid_transport(*g);
  auto make = [&](auto* tag) -> MatrixBase* {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto* gm = new GeneralMatrix<T>;
    gm->type = type;
    gm->rows_g = m;
    gm->cols_g = n;
    gm->isrc = isrc;
    gm->jsrc = jsrc;
    gm->m.create(g, false, m, n, nb, isrc, jsrc);
    return gm;
  };
  return dispatch_type(type, make, []() -> MatrixBase* { return nullptr; });
}

template <class T>
static void gm_transfer(GeneralMatrix<T>& gm, void* host, long ld, bool up) {
  ScratchStream s;
  if (up)
    gm.m.upload(static_cast<const T*>(host), ld, false, false, T{}, s);
  else
    gm.m.download(static_cast<T*>(host), ld, false, s);
  s.sync();
}

void general_matrix_transfer(MatrixBase* h, void* host, long ld, bool upload) {
  dispatch_type(h->type, [&](auto* tag) {
    gm_transfer(static_cast<GeneralMatrix<std::remove_pointer_t<decltype(tag)>>&>(*h), host, ld, upload);
  });
}

// dst view tile (il, jl) = alpha * op(src tile): src (il, jl) for the copying ops (4 conjugate, 5 copy), src (jl, il)
// for the transposing ones (0 adjoint, 3 transpose).  A transposed view of a block-cyclic matrix stays on the
// same process (tile (i,j) of the view is tile (j,i) of the source), so this is local work on every rank.
template <class T>
void xform_tiles(T* dst, long dltr, long dltc, const T* src, long sltr, size_t te, int nb, int mode, T alpha,
                        bool use_alpha, hipStream_t s) {
  const bool tr = (mode == 0 || mode == 3);
  for (long jl = 0; jl < dltc; ++jl) {
    // view column jl, all view rows: src tiles (il, jl) [stride te] or (jl, il) [stride sltr * te]
    const T* sp = tr ? src + (size_t) jl * te : src + (size_t) jl * sltr * te;
    launch_tile_xform_alpha(dst + (size_t) jl * dltr * te, (long) nb, (long) te, sp, (long) nb,
                            tr ? (long) (sltr * te) : (long) te, nb, nb, (int) dltr, mode, alpha, use_alpha, s);
  }
}

// A canonical sweep on RESIDENT operands (dlaf::triangular_solver, or the multiplication): A = a DeviceMatrix (its
// uplo triangle: a Cholesky factor, or any triangular matrix uploaded as such), B = a general resident matrix,
// overwritten by the result; the entry has judged them with require_triangular (c_api_device.cpp), and a caller inside
// the library builds them to fit.  Nothing crosses PCIe: the operand views of the one device algorithm (X T^H = B, or
// X = B T^H) are made by tile transforms on the device.
template <class T>
int triangular_canonical_device(const char* who, CanonicalSweep<T> sweep, char side, char uplo, char op, char diag,
                                T alpha, DeviceMatrix<T>& A, GeneralMatrix<T>& B) {
  Grid* g = A.grid;
  if (B.m.grid != g)
    fatal("[dlaf_mi355x] %s: A and B live on different grids\n", who);
  const auto [left, a_upper, unit, t_transposed, t_conj, t_upper] = operand_map(side, uplo, op, diag);
  const long m = B.rows_g, n = B.cols_g, na = A.n;
  const int nb = A.nb;
  if (m == 0 || n == 0)
    return 0;
  // the caller's A and its source process (the DeviceMatrix holds the transposed view for uplo U)
  const Axis& a_rows = A.transposed ? A.cols : A.rows;
  const Axis& a_cols = A.transposed ? A.rows : A.cols;
  // in terms of the STORED tiles S (S = A for uplo L, S = A^T for uplo U): T = op(S)
  const bool s_transpose = t_transposed != A.transposed;
  const int t_mode = s_transpose ? (t_conj ? 0 : 3) : (t_conj ? 4 : 5);

  ScratchStream s;  // before the matrices: destroyed after them
  TileMatrix<T> Td, Bd;
  const size_t te = A.tile_elems;
  if (t_mode == 5) {
    Td.create(g, t_transposed, na, na, nb, a_rows.src, a_cols.src, A.tiles);  // T is the stored matrix itself
  }
  else {
    Td.create(g, t_transposed, na, na, nb, a_rows.src, a_cols.src);
    xform_tiles(Td.tiles, Td.ltr, Td.ltc, A.tiles, A.ltr, te, nb, t_mode, T{}, false, s);
  }
  const bool scale = !is_one(alpha);
  if (left) {
    // B_dev = (alpha B)^H = conj(alpha) B^H
    Bd.create(g, true, m, n, nb, B.isrc, B.jsrc);
    xform_tiles(Bd.tiles, Bd.ltr, Bd.ltc, B.m.tiles, B.m.ltr, te, nb, 0, conj_of(alpha), scale, s);
  }
  else {
    Bd.create(g, false, m, n, nb, B.isrc, B.jsrc, B.m.tiles);  // in place
    if (scale)
      xform_tiles(Bd.tiles, Bd.ltr, Bd.ltc, B.m.tiles, B.m.ltr, te, nb, 5, alpha, true, s);
  }
  s.sync();
  sweep(Td, Bd, t_upper, unit);
  if (left) {
    xform_tiles(B.m.tiles, B.m.ltr, B.m.ltc, Bd.tiles, Bd.ltr, te, nb, 0, T{}, false, s);
    s.sync();
  }
  return 0;
}

int triangular_solver_device(char side, char uplo, char op, char diag, const void* alpha, MatrixBase* a, MatrixBase* b) {
  if (!a || !b || a->type != b->type)
    fatal("[dlaf_mi355x] triangular solver: operands of different element types\n");
  return dispatch_type(a->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    return triangular_canonical_device<T>("triangular solver", solve_canonical<T>, side, uplo, op, diag,
                                          *static_cast<const T*>(alpha), static_cast<DeviceMatrix<T>&>(*a),
                                          static_cast<GeneralMatrix<T>&>(*b));
  });
}

#define DLAF_CANONICAL_INST(T)                                                                                   \
  template int triangular_canonical_host<T>(CanonicalSweep<T>, bool, Grid*, char, char, char, char, T,             \
                                            HostOperand<const T>, HostOperand<T>);                               \
  template int triangular_canonical_device<T>(const char*, CanonicalSweep<T>, char, char, char, char, T,             \
                                              DeviceMatrix<T>&, GeneralMatrix<T>&);                                \
  template void xform_tiles<T>(T*, long, long, const T*, long, size_t, int, int, T, bool, hipStream_t);            \
  template int triangular_solver_host<T>(Grid*, char, char, char, char, T, HostOperand<const T>, HostOperand<T>);
DLAF_CANONICAL_INST(float)
DLAF_CANONICAL_INST(double)
DLAF_CANONICAL_INST(cfloat)
DLAF_CANONICAL_INST(cdouble)
#undef DLAF_CANONICAL_INST

}  // namespace dlaf_mi355x
