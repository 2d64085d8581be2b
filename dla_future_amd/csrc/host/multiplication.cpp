// multiplication.cpp -- distributed triangular multiplication  B = alpha op(A) B  /  B = alpha B op(A)  on the tile
// kernels of the triangular solver, (second part) the Hermitian multiplication  C = beta C + alpha A B  /
// beta C + alpha B A  on its own step kernel, and (third part) the general multiplication  C = beta C + alpha op(A) op(B)
// on a kernel that keeps a block of C in its accumulators over the k dimension.
//
// Reference: dlaf::triangular_multiplication (include/dlaf/multiplication/triangular.h) and its hand-written
// variants (multiplication/triangular/impl.h); dlaf::hermitian_multiplication (include/dlaf/multiplication/hermitian.h),
// which implements side L / uplo L only and reduces a panel of C along process columns at every step;
// dlaf::multiplication::internal::generalMatrix (include/dlaf/multiplication/general.h), NoTrans x NoTrans.
//
// MI355X design: the solver's operand mapping (solver.cpp header: side / op decide T and B_dev, the relayout
// transposes, conjugates and scales) turns every combination into ONE device algorithm,
//
//        X = B T^H        in place, T lower (swept backward, k = nt-1 .. 0) or upper (swept forward)
//
//   step k:  B(:,j) += P_k T(j,k)^H   for the columns j beyond k      grouped NT update kernel, additive (role 4)
//            B(:,k)  = P_k T_kk^H                                    panel TRMM kernel (kernels_trmm.hip)
//
// with P_k the ORIGINAL column k of B.  Sweeping in the opposite direction to the solve, a column receives its own
// diagonal product before the contributions of the columns it depends on, and column k is still untouched when step
// k reads it.  No step reads a computed value: there is no chain, the broadcasts of P_k and of T's panels run ahead
// on the communication stream, and the TRMM of a column runs on a side stream beside the next step's update.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "../device/gemm_forms.hpp"
#include "drivers.hpp"
#include "sweep.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

// device time of the last sweep of either multiplication on this process (HIP events on the compute stream; relayout
// and PCIe excluded)
double g_last_mult_ms = 0;
double g_last_mult_flops = 0;

// X = B T^H in place on Bd; Td lower (swept backward) or upper (swept forward) triangular, unit: its diagonal is
// taken as 1.  The same views, alignment requirement and T-operand fetch as solve_canonical.
template <class T>
void multiply_canonical(TileMatrix<T>& Td, TileMatrix<T>& Bd, bool upper, bool unit) {
  Grid* g = Bd.grid;
  Transport* tr = grid_transport(*g);
  const bool dist = g->nranks > 1;
  const long nt = Bd.cols.nt();  // tiles along n
  if (nt == 0 || Bd.rows_global == 0)
    return;
  const size_t tile_elems = Bd.tile_elems;
  check_t_aligned(Td, Bd, "triangular multiplication");

  // s_main: the updates; s_side: the panel TRMMs; s_comm: T operands and the P_k broadcasts; the update kernel's
  // status word (nothing here fails: it stays 0)
  Sweep sw(true, true);
  const hipStream_t s_main = sw.s_main, s_side = sw.s_side, s_comm = sw.s_comm;
  // ev_u: the update of step s has read P_k; ev_m: the TRMM of step s is done (and every buffer of the step free)
  Events ev_xb((size_t) nt), ev_u((size_t) nt), ev_m((size_t) nt);

  TOperandFetch<T> tf(Td, Bd, tr, upper, !upper, s_comm);
  Ring<T> xpanel((size_t) Bd.ltr * tile_elems, dist);
  std::vector<const T*> xp((size_t) nt, nullptr);  // P_k of step s as the update's first operand

  // s_comm: once the TRMM of step s - kBuf has freed the buffers, the T operands of step s and the original column k
  // to the other members of my Bd row
  auto fetch = [&](long s) {
    wait_ring_free(s_comm, ev_m, s);
    tf.fetch(s);
    xp[(size_t) s] = bcast_view_column(tr, Bd, tf.step_k(s), xpanel[(int) (s % kBuf)], s_comm);
    if (Bd.cols.P > 1)
      DLAF_HIP_CHECK(hipEventRecord(ev_xb[(size_t) s], s_comm));
  };

  auto update = [&](long s, long j0, long j1) {
    const TOperand<T>& o = tf.top[(size_t) s];
    j0 = std::max(j0, o.jl0);
    j1 = std::min(j1, o.jl1);
    if (j0 >= j1 || Bd.ltr == 0)
      return;
    launch_update(rect_update_args(Bd, 0, Bd.ltr, j0, j1, xp[(size_t) s], o.base + (j0 - o.jl0) * o.ts, o.ts,
                                   Bd.cols.tile_extent(tf.step_k(s)), sw.info.p),
                  s_main, 4);
  };

  sw.begin(true);

  // ---- the sweep --------------------------------------------------------------------------------------
  // s_main: U(s, all but the previous step's column) . [TRMM(s-1) done] . U(s, that column) -- the TRMM of step s-1
  // runs on s_side under the bulk of step s's update; operands arrive one step ahead on s_comm
  fetch(0);
  for (long s = 0; s < nt; ++s) {
    const long k = tf.step_k(s);
    if (s + 1 < nt)
      fetch(s + 1);
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, tf.ev_t[(size_t) s], 0));
    if (Bd.cols.P > 1)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, ev_xb[(size_t) s], 0));
    const long kp = s >= 1 ? tf.step_k(s - 1) : -1;  // the column the previous step's TRMM writes (beyond k)
    const long jp = (kp >= 0 && Bd.cols.mine(kp)) ? Bd.cols.local_of(kp) : -1;
    if (jp >= 0) {
      update(s, 0, jp);
      update(s, jp + 1, Bd.ltc);
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, ev_m[(size_t) (s - 1)], 0));
      update(s, jp, jp + 1);
    }
    else {
      update(s, 0, Bd.ltc);
    }
    DLAF_HIP_CHECK(hipEventRecord(ev_u[(size_t) s], s_main));

    // column k: B(:,k) = P_k T_kk^H once every read of P_k (the update above, the broadcast) is done
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_side, ev_u[(size_t) s], 0));
    if (Bd.cols.mine(k) && Bd.ltr > 0) {
      auto ta = panel_args<TrmmArgs<T>>(Bd, 0, Bd.ltr, Bd.cols.local_of(k), tf.top[(size_t) s].diag, Bd.cols.tile_extent(k));
      ta.upper = upper ? 1 : 0;
      ta.unit = unit ? 1 : 0;
      launch_trmm(ta, s_side);
    }
    DLAF_HIP_CHECK(hipEventRecord(ev_m[(size_t) s], s_side));
  }
  DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, ev_m[(size_t) (nt - 1)], 0));

  g_last_mult_ms = sw.finish();
  // whole-grid algorithmic flops: rows x n^2 (x4 complex), as for the solve
  g_last_mult_flops = (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (double) Bd.rows_global * (double) Bd.cols.n * (double) Bd.cols.n;
}

// ================================================================================ Hermitian multiplication
// Y = beta Y + alpha X H, H Hermitian with its LOWER triangle stored in Hd (conj_h: the stored tiles hold conj(H), what
// a resident uplo = U matrix keeps).  Xd and Yd are two views of the same shape and distribution; Hd is aligned with
// their columns like the T of the triangular sweeps.  Step l (forward, no step reads a computed value):
//        Y(:, j) += alpha X(:, l) H(l, j)    for every local tile column j         one launch (kernels_hemm.hip)
// H(l, j) comes from the stored column l (j > l, adjoint), the diagonal tile (j = l) and the stored row l (j < l).
// Broadcasts per step on a grid (all on s_comm, one step ahead, a ring of kBuf buffers per operand; no reduce):
//   X(:, l)            along the process rows of the view from the owner column             Yd.ltr tiles
//   column l of H      TOperandFetch (sweep.hpp)    : one broadcast when H's rows are spread like Y's columns,
//                      else the Cholesky's panel + transposed-panel pair                    <= Yd.ltc (+ Hd.ltr) tiles
//   row l of H         the mirror image: one broadcast when H's COLUMNS are spread like Y's columns, else the row
//                      along Y's columns' dimension and then tile by tile down the other    <= Yd.ltc (+ Hd.ltc) tiles
//   H(l, l)            to the processes that hold column l of Y (TOperandFetch)             1 tile
template <class T>
void hermitian_canonical(TileMatrix<T>& Hd, TileMatrix<T>& Xd, TileMatrix<T>& Yd, T alpha, T beta, bool conj_h) {
  Grid* g = Yd.grid;
  Transport* tr = grid_transport(*g);
  const bool dist = g->nranks > 1;
  const int nb = Yd.nb;
  const long nt = Yd.cols.nt();
  if (nt == 0 || Yd.rows_global == 0)
    return;
  const size_t tile_elems = Yd.tile_elems, tile_bytes = tile_elems * sizeof(T);
  const CommAxis along_row = Yd.transposed ? CommAxis::Col : CommAxis::Row;
  const CommAxis along_col = Yd.transposed ? CommAxis::Row : CommAxis::Col;
  const bool aligned = Hd.row_dim() == Yd.col_dim();
  check_t_aligned(Hd, Yd, "hermitian multiplication");

  Sweep sw(false, false);
  const hipStream_t s_main = sw.s_main, s_comm = sw.s_comm;
  // one step ahead through the pipeline (its ring-reuse wait covers the buffers of TOperandFetch too).  tf.ev_t:
  // column l and the diagonal tile are in place; the pipeline's ev_in: so are row l and X(:, l)
  StepPipeline pipe(nt);

  TOperandFetch<T> tf(Hd, Yd, tr, false, false, s_comm);
  Ring<T> rpanel((size_t) Yd.ltc * tile_elems, dist), rstage((size_t) Hd.ltc * tile_elems, dist && aligned);
  Ring<T> xpanel((size_t) Yd.ltr * tile_elems, dist);
  struct RowOperand {
    const T* base = nullptr;  // stored H(l, j) of local column jl < jr1 of Yd at base + jl * ts
    long ts = 0;
    const T* x = nullptr;     // X(:, l)
  };
  std::vector<RowOperand> rop((size_t) nt);

  // local tiles (lrow, 0 .. count) of Hd, one tile row, packed next to each other
  auto pack_row = [&](T* dst, long lrow, long count) {
    if (count > 0)
      DLAF_HIP_CHECK(hipMemcpy2DAsync(dst, tile_bytes, Hd.tile(lrow, 0), (size_t) Hd.ltr * tile_bytes, tile_bytes,
                                      (size_t) count, hipMemcpyDeviceToDevice, s_comm));
  };

  auto fetch = [&](long l, int buf) {
    tf.fetch(l);
    RowOperand& o = rop[(size_t) l];
    const long jr1 = Yd.cols.next_local(l);  // local columns of Yd left of l
    if (!dist) {
      o.base = Hd.tile(l, 0);
      o.ts = (long) (tile_elems * Hd.ltr);
    }
    else if (!aligned) {
      // Hd's columns are spread like Yd's: row l sits on the process of my Yd-column coordinate whose other
      // coordinate owns Hd's row l -> one broadcast
      const bool have = Hd.rows.mine(l);
      if (Yd.row_P > 1) {
        if (have)
          pack_row(rpanel[buf], Hd.rows.local_of(l), jr1);
        if (jr1 > 0)
          tr->bcast(along_col, Hd.rows.owner(l), Yd.row_rank, rpanel[buf], rpanel[buf], (size_t) jr1 * tile_bytes, s_comm);
        o.base = rpanel[buf];
        o.ts = (long) tile_elems;
      }
      else {
        o.base = Hd.tile(Hd.rows.local_of(l), 0);
        o.ts = (long) (tile_elems * Hd.ltr);
      }
    }
    else {
      // Hd's rows are spread like Yd's columns: row l along that dimension first (every process gets the
      // columns its other coordinate owns), then tile j down the other dimension from the owner of Hd's column j
      const long hj1 = Hd.cols.next_local(l);
      if (Hd.rows.mine(l))
        pack_row(rstage[buf], Hd.rows.local_of(l), hj1);
      if (Yd.cols.P > 1 && hj1 > 0)
        tr->bcast(along_row, Hd.rows.owner(l), Yd.cols.rank, rstage[buf], rstage[buf], (size_t) hj1 * tile_bytes, s_comm);
      if (Yd.row_P > 1) {
        tr->group_begin();
        for (long jl = 0; jl < jr1; ++jl) {
          const long gj = Yd.cols.global_of(jl);
          const int root = Hd.cols.owner(gj);
          const T* src = (Hd.cols.rank == root) ? rstage[buf] + (size_t) Hd.cols.local_of(gj) * tile_elems : nullptr;
          tr->bcast(along_col, root, Yd.row_rank, src, rpanel[buf] + (size_t) jl * tile_elems, tile_bytes, s_comm);
        }
        tr->group_end();
        o.base = rpanel[buf];
        o.ts = (long) tile_elems;
      }
      else {
        // I hold every column of Hd's row l: tile gj sits at local column gj
        o.base = rstage[buf] + (size_t) Yd.cols.global_of(0) * tile_elems;
        o.ts = (long) tile_elems * Yd.cols.P;
      }
    }
    // X(:, l) to the other members of my row of the view (X is not written: the owner sends its own tiles)
    o.x = bcast_view_column(tr, Xd, l, xpanel[buf], s_comm);
  };

  auto apply = [&](long l) {
    if (Yd.ltr > 0 && Yd.ltc > 0) {
      const TOperand<T>& o = tf.top[(size_t) l];
      const RowOperand& r = rop[(size_t) l];
      HemmArgs<T> ha;
      ha.y = Yd.tiles;
      ha.y_tsr = (long) tile_elems;
      ha.y_tsc = (long) (tile_elems * Yd.ltr);
      ha.x = r.x;
      ha.x_ts = (long) tile_elems;
      ha.hc = o.base;
      ha.hc_ts = o.ts;
      ha.jc0 = (int) o.jl0;
      ha.hd = o.diag;
      ha.hr = r.base;
      ha.hr_ts = r.ts;
      ha.l = (int) l;
      ha.K = Yd.cols.tile_extent(l);
      ha.ltr = (int) Yd.ltr;
      ha.ltc = (int) Yd.ltc;
      ha.nb = nb;
      ha.pr = Yd.rows.P;
      ha.ri = Yd.rows.shift();
      ha.nt_r = (int) Yd.rows.nt();
      ha.last_rows = Yd.rows.last_extent();
      ha.pc = Yd.cols.P;
      ha.ci = Yd.cols.shift();
      ha.nt_c = (int) nt;
      ha.last_cols = Yd.cols.last_extent();
      ha.alpha = alpha;
      ha.beta = beta;
      ha.first = l == 0 ? 1 : 0;
      ha.conj_h = conj_h ? 1 : 0;
      launch_hemm(ha, s_main);
    }
  };
  pipe.run(sw, fetch, apply);

  g_last_mult_ms = sw.finish();
  // whole-grid algorithmic flops: 2 x rows x na^2 (x4 complex)
  g_last_mult_flops = (TypeInfo<T>::is_complex ? 8.0 : 2.0) * (double) Yd.rows_global * (double) Yd.cols.n * (double) Yd.cols.n;
}

// ================================================================================ general multiplication
// C = beta C + alpha op(A) op(B).  Ad, Bd, Cd: the three matrices AS STORED (no view is transposed, nothing is
// re-laid out); nkt: the tiles of the k dimension to multiply (0: k == 0 or alpha == 0 -- C = beta C, Ad and Bd are not
// touched).  One process: ONE launch over all the k tiles, every op pair.  A grid (N x N only: the entries refuse the
// rest) runs SUMMA, one step per k tile l, nothing reduced:
//   column l of A      along the process rows from the owner column (bcast_view_column)       Cd.ltr tiles
//   row l of B         packed, then down the process columns from the owner row               Cd.ltc tiles
//   C += A(:, l) B(l, :)   one launch with nk = 1 (first: l == 0)
// both broadcasts on s_comm one step ahead, into a ring of kBuf buffers per operand.  A starts on C's process row and B
// on C's process column (the entries check); A's columns and B's rows need no common source.
template <class T>
void general_canonical(TileMatrix<T>& Ad, TileMatrix<T>& Bd, TileMatrix<T>& Cd, char opa, char opb, long k, long nkt,
                       T alpha, T beta) {
  Grid* g = Cd.grid;
  Transport* tr = grid_transport(*g);
  const bool dist = g->nranks > 1;
  const bool an = gemm_op_is_n(opa), bn = gemm_op_is_n(opb);
  const size_t tile_elems = Cd.tile_elems, tile_bytes = tile_elems * sizeof(T);
  const Axis& ka = an ? Ad.cols : Ad.rows;  // the k axis as A has it (tile extents), and as B has it (owners)
  const Axis& kb = bn ? Bd.rows : Bd.cols;

  GeneralArgs<T> ga;
  ga.c = Cd.tiles;
  ga.c_tsr = (long) tile_elems;
  ga.c_tsc = (long) (tile_elems * Cd.ltr);
  ga.opa = opa;
  ga.opb = opb;
  ga.ltr = (int) Cd.ltr;
  ga.ltc = (int) Cd.ltc;
  ga.nb = Cd.nb;
  ga.pr = Cd.rows.P;
  ga.ri = Cd.rows.shift();
  ga.nt_r = (int) Cd.rows.nt();
  ga.last_rows = Cd.rows.last_extent();
  ga.pc = Cd.cols.P;
  ga.ci = Cd.cols.shift();
  ga.nt_c = (int) Cd.cols.nt();
  ga.last_cols = Cd.cols.last_extent();
  ga.alpha = alpha;
  ga.beta = beta;
  ga.a = ga.b = nullptr;
  ga.a_ts = ga.a_ks = ga.b_ts = ga.b_ks = 0;
  ga.nk = 0;
  ga.k_last = 0;
  const bool work = Cd.ltr > 0 && Cd.ltc > 0;

  Sweep sw(false, false);
  const hipStream_t s_main = sw.s_main, s_comm = sw.s_comm;
  if (nkt == 0 || !dist) {
    sw.begin(false);
    if (nkt > 0) {
      // tile (i, t) of a stored m x k matrix: rows next to each other; tile (t, i) of a stored k x m one: columns
      ga.a = Ad.tiles;
      ga.a_ts = (long) (an ? tile_elems : tile_elems * Ad.ltr);
      ga.a_ks = (long) (an ? tile_elems * Ad.ltr : tile_elems);
      ga.b = Bd.tiles;
      ga.b_ts = (long) (bn ? tile_elems * Bd.ltr : tile_elems);
      ga.b_ks = (long) (bn ? tile_elems : tile_elems * Bd.ltr);
      ga.nk = (int) nkt;
      ga.k_last = ka.last_extent();
    }
    if (work)
      launch_general(ga, s_main);
  }
  else {
    StepPipeline pipe(nkt);
    Ring<T> apanel((size_t) Cd.ltr * tile_elems, Ad.cols.P > 1), bpanel((size_t) Cd.ltc * tile_elems, Bd.rows.P > 1);
    struct StepOperands {
      const T* a = nullptr;
      const T* b = nullptr;
      long b_ts = 0;
    };
    std::vector<StepOperands> sop((size_t) nkt);
    auto fetch = [&](long l, int buf) {
      StepOperands& o = sop[(size_t) l];
      o.a = bcast_view_column(tr, Ad, l, apanel[buf], s_comm);
      if (Bd.rows.P > 1) {
        // local tiles (lrow, 0 .. ltc) of Bd, one tile row, packed next to each other
        if (kb.mine(l) && Bd.ltc > 0)
          DLAF_HIP_CHECK(hipMemcpy2DAsync(bpanel[buf], tile_bytes, Bd.tile(kb.local_of(l), 0), (size_t) Bd.ltr * tile_bytes,
                                          tile_bytes, (size_t) Bd.ltc, hipMemcpyDeviceToDevice, s_comm));
        if (Bd.ltc > 0)
          tr->bcast(CommAxis::Col, kb.owner(l), kb.rank, bpanel[buf], bpanel[buf], (size_t) Bd.ltc * tile_bytes, s_comm);
        o.b = bpanel[buf];
        o.b_ts = (long) tile_elems;
      }
      else {
        o.b = Bd.tile(l, 0);
        o.b_ts = (long) (tile_elems * Bd.ltr);
      }
    };
    auto apply = [&](long l) {
      if (work) {
        ga.a = sop[(size_t) l].a;
        ga.a_ts = (long) tile_elems;
        ga.b = sop[(size_t) l].b;
        ga.b_ts = sop[(size_t) l].b_ts;
        ga.nk = 1;
        ga.k_last = ka.tile_extent(l);
        ga.first = l == 0 ? 1 : 0;
        launch_general(ga, s_main);
      }
    };
    pipe.run(sw, fetch, apply);
  }
  g_last_mult_ms = sw.finish();
  // whole-grid algorithmic flops: 2 m n k (x4 complex)
  g_last_mult_flops = (TypeInfo<T>::is_complex ? 8.0 : 2.0) * (double) Cd.rows.n * (double) Cd.cols.n * (double) k;
}

}  // namespace

void multiplication_set_profile(double ms, double flops) {
  g_last_mult_ms = ms;
  g_last_mult_flops = flops;
}

void multiplication_last_profile(double* ms, double* flops) {
  if (ms)
    *ms = g_last_mult_ms;
  if (flops)
    *flops = g_last_mult_flops;
}

template <class T>
int triangular_multiplication_host(Grid* g, char side, char uplo, char op, char diag, T alpha, HostOperand<const T> a,
                                   HostOperand<T> b) {
  return triangular_canonical_host<T>(multiply_canonical<T>, false, g, side, uplo, op, diag, alpha, a, b);
}

int triangular_multiplication_device(char side, char uplo, char op, char diag, const void* alpha, MatrixBase* a,
                                     MatrixBase* b) {
  if (!a || !b || a->type != b->type)
    fatal("[dlaf_mi355x] triangular multiplication: operands of different element types\n");
  return dispatch_type(a->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    return triangular_canonical_device<T>("triangular multiplication", multiply_canonical<T>, side, uplo, op, diag,
                                          *static_cast<const T*>(alpha), static_cast<DeviceMatrix<T>&>(*a),
                                          static_cast<GeneralMatrix<T>&>(*b));
  });
}

// C = beta C + alpha A B (side L) / beta C + alpha B A (side R), A Hermitian in its uplo triangle.  Side R is the
// canonical form; side L runs it on the adjoints, C^H = conj(beta) C^H + conj(alpha) B^H A (the relayout transposes and
// conjugates).  uplo U: the transposed, conjugated view of A holds A itself with its LOWER triangle valid.
template <class T>
int hermitian_multiplication_host(Grid* g, char side, char uplo, T alpha, HostOperand<const T> a, HostOperand<const T> b,
                                  T beta, HostOperand<T> c) {
  const bool left = side_is_left(side), a_upper = uplo_is_upper(uplo);
  if (c.m == 0 || c.n == 0)
    return 0;
  (void) checked_transport(*g);
  ScratchStream s;  // before the matrices: destroyed after them
  TileMatrix<T> Hd, Xd, Yd;
  Hd.create(g, a_upper, a.n, a.n, a.nb, a.isrc, a.jsrc);
  Xd.create_rhs(g, left, c.m, c.n, c.mb, c.nb, c.isrc, c.jsrc);
  Yd.create_rhs(g, left, c.m, c.n, c.mb, c.nb, c.isrc, c.jsrc);
  Hd.upload(a.p, a.ld, a_upper, false, T{}, s);
  Xd.upload(b.p, b.ld, left, false, T{}, s);
  if (!is_zero(beta))  // beta = 0: C is not read
    Yd.upload(c.p, c.ld, left, false, T{}, s);
  s.sync();
  hermitian_canonical(Hd, Xd, Yd, left ? conj_of(alpha) : alpha, left ? conj_of(beta) : beta, false);
  Yd.download(c.p, c.ld, left, s);
  s.sync();
  return 0;
}

// The same on RESIDENT operands: A a DeviceMatrix (its uplo triangle; for uplo U it holds the transposed view, whose
// lower triangle is conj(A)'s: conj_h), B and C general resident matrices of the same shape, judged by the entry with
// require_hermitian_multiplication (c_api_device.cpp).  Side R works on B's and C's tiles in place; side L on adjoint
// copies made by tile transforms on the device.  Only C is written.
template <class T>
int hermitian_device_t(char side, char uplo, T alpha, DeviceMatrix<T>& A, GeneralMatrix<T>& B, T beta,
                       GeneralMatrix<T>& C) {
  const char* who = "hermitian multiplication";
  Grid* g = A.grid;
  if (B.m.grid != g || C.m.grid != g)
    fatal("[dlaf_mi355x] %s: A, B and C live on different grids\n", who);
  const bool left = side_is_left(side);
  const long m = C.rows_g, n = C.cols_g, na = A.n;
  const int nb = A.nb;
  const Axis& a_rows = A.transposed ? A.cols : A.rows;
  const Axis& a_cols = A.transposed ? A.rows : A.cols;
  if (m == 0 || n == 0)
    return 0;
  ScratchStream s;  // before the matrices: destroyed after them
  TileMatrix<T> Hd, Xd, Yd;
  const size_t te = A.tile_elems;
  Hd.create(g, A.transposed, na, na, nb, a_rows.src, a_cols.src, A.tiles);
  if (left) {
    Xd.create(g, true, m, n, nb, C.isrc, C.jsrc);
    Yd.create(g, true, m, n, nb, C.isrc, C.jsrc);
    xform_tiles(Xd.tiles, Xd.ltr, Xd.ltc, B.m.tiles, B.m.ltr, te, nb, 0, T{}, false, s);
    if (!is_zero(beta))
      xform_tiles(Yd.tiles, Yd.ltr, Yd.ltc, C.m.tiles, C.m.ltr, te, nb, 0, T{}, false, s);
    s.sync();
  }
  else {
    Xd.create(g, false, m, n, nb, C.isrc, C.jsrc, B.m.tiles);
    Yd.create(g, false, m, n, nb, C.isrc, C.jsrc, C.m.tiles);
  }
  hermitian_canonical(Hd, Xd, Yd, left ? conj_of(alpha) : alpha, left ? conj_of(beta) : beta, A.transposed);
  if (left) {
    xform_tiles(C.m.tiles, C.m.ltr, C.m.ltc, Yd.tiles, Yd.ltr, te, nb, 0, T{}, false, s);
    s.sync();
  }
  return 0;
}

int hermitian_multiplication_device(char side, char uplo, const void* alpha, MatrixBase* a, MatrixBase* b,
                                    const void* beta, MatrixBase* c) {
  if (!a || !b || !c || a->type != b->type || a->type != c->type)
    fatal("[dlaf_mi355x] hermitian multiplication: operands of different element types\n");
  return dispatch_type(a->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    return hermitian_device_t<T>(side, uplo, *static_cast<const T*>(alpha), static_cast<DeviceMatrix<T>&>(*a),
                                 static_cast<GeneralMatrix<T>&>(*b), *static_cast<const T*>(beta),
                                 static_cast<GeneralMatrix<T>&>(*c));
  });
}

// C = beta C + alpha op(A) op(B) on host operands: this process's local column-major parts, the three matrices as
// stored (A is m x k or k x m, B k x n or n x k), one square block nb.  The arguments have passed
// require_general_multiplication (api_checks.hpp).  k == 0 or alpha == 0: A and B are not referenced (BLAS).
template <class T>
int general_multiplication_host(Grid* g, char opa, char opb, T alpha, HostOperand<const T> a, HostOperand<const T> b,
                                T beta, HostOperand<T> c) {
  if (c.m == 0 || c.n == 0)
    return 0;
  (void) checked_transport(*g);
  const long k = gemm_op_is_n(opa) ? a.n : a.m;
  const int nb = c.nb;
  const bool product = k > 0 && !is_zero(alpha);
  ScratchStream s;  // before the matrices: destroyed after them
  TileMatrix<T> Ad, Bd, Cd;
  Cd.create(g, false, c.m, c.n, nb, c.isrc, c.jsrc);
  if (product) {
    Ad.create(g, false, a.m, a.n, nb, a.isrc, a.jsrc);
    Bd.create(g, false, b.m, b.n, nb, b.isrc, b.jsrc);
    Ad.upload(a.p, a.ld, false, false, T{}, s);
    Bd.upload(b.p, b.ld, false, false, T{}, s);
  }
  if (!is_zero(beta))  // beta = 0: C is not read
    Cd.upload(c.p, c.ld, false, false, T{}, s);
  s.sync();
  general_canonical(Ad, Bd, Cd, opa, opb, k, product ? (k + nb - 1) / nb : 0, alpha, beta);
  Cd.download(c.p, c.ld, false, s);
  s.sync();
  return 0;
}

// The same on three RESIDENT general matrices (arguments judged by the entry, c_api_device.cpp): the tiles are the
// operands, only C's are written.
int general_multiplication_device(char opa, char opb, const void* alpha, MatrixBase* a, MatrixBase* b, const void* beta,
                                  MatrixBase* c) {
  if (!a || !b || !c || a->type != b->type || a->type != c->type)
    fatal("[dlaf_mi355x] general multiplication: operands of different element types\n");
  return dispatch_type(a->type, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto& A = static_cast<GeneralMatrix<T>&>(*a);
    auto& B = static_cast<GeneralMatrix<T>&>(*b);
    auto& C = static_cast<GeneralMatrix<T>&>(*c);
    if (A.m.grid != C.m.grid || B.m.grid != C.m.grid)
      fatal("[dlaf_mi355x] general multiplication: A, B and C live on different grids\n");
    if (C.rows_g == 0 || C.cols_g == 0)
      return 0;
    const T al = *static_cast<const T*>(alpha), be = *static_cast<const T*>(beta);
    const long k = gemm_op_is_n(opa) ? A.cols_g : A.rows_g;
    const bool product = k > 0 && !is_zero(al);
    general_canonical(A.m, B.m, C.m, opa, opb, k, product ? (k + C.m.nb - 1) / C.m.nb : 0, al, be);
    return 0;
  });
}

#define DLAF_MULT_INST(T)                                                                                          \
  template int hermitian_multiplication_host<T>(Grid*, char, char, T, HostOperand<const T>, HostOperand<const T>, T, \
                                                HostOperand<T>);                                                   \
  template int general_multiplication_host<T>(Grid*, char, char, T, HostOperand<const T>, HostOperand<const T>, T,   \
                                              HostOperand<T>);                                                     \
  template int triangular_multiplication_host<T>(Grid*, char, char, char, char, T, HostOperand<const T>, HostOperand<T>);
DLAF_MULT_INST(float)
DLAF_MULT_INST(double)
DLAF_MULT_INST(cfloat)
DLAF_MULT_INST(cdouble)
#undef DLAF_MULT_INST

}  // namespace dlaf_mi355x
