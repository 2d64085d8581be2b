// multiplication.cpp -- distributed triangular multiplication  B = alpha op(A) B  /  B = alpha B op(A)  on the tile
// kernels of the triangular solver.
//
// Reference: dlaf::triangular_multiplication (include/dlaf/multiplication/triangular.h) and its hand-written
// variants (multiplication/triangular/impl.h).
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

#include "runtime.hpp"
#include "t_operand.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

// device time of the last sweep on this process (HIP events on the compute stream; relayout and PCIe excluded)
double g_last_mult_ms = 0;
double g_last_mult_flops = 0;

// X = B T^H in place on Bd; Td lower (swept backward) or upper (swept forward) triangular, unit: its diagonal is
// taken as 1.  The same views, alignment requirement and T-operand fetch as solve_canonical.
template <class T>
void multiply_canonical(TileMatrix<T>& Td, TileMatrix<T>& Bd, bool upper, bool unit) {
  Grid* g = Bd.grid;
  Transport* tr = grid_transport(*g);
  const bool dist = g->nranks > 1;
  const int nb = Bd.nb;
  const long nt = Bd.cols.nt();  // tiles along n
  if (nt == 0 || Bd.rows_global == 0)
    return;
  const size_t tile_elems = Bd.tile_elems, tile_bytes = tile_elems * sizeof(T);
  const CommAxis along_row = Bd.transposed ? CommAxis::Col : CommAxis::Row;
  const bool aligned = Td.row_dim() == Bd.col_dim();
  check_t_aligned(Td, Bd, "triangular multiplication");

  // s_main: the updates; s_side: the panel TRMMs; s_comm: T operands and the P_k broadcasts
  hipStream_t s_main = nullptr, s_side = nullptr, s_comm = nullptr;
  int lo = 0, hi = 0;
  DLAF_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_main, hipStreamNonBlocking, lo));
  DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_side, hipStreamNonBlocking, hi));
  DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_comm, hipStreamNonBlocking, hi));
  // ev_u: the update of step s has read P_k; ev_m: the TRMM of step s is done (and every buffer of the step free)
  Events ev_t((size_t) nt), ev_xb((size_t) nt), ev_u((size_t) nt), ev_m((size_t) nt);
  // the update kernel's status word (nothing here fails: it stays 0)
  int* info = nullptr;
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&info), sizeof(int)));
  DLAF_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s_main));

  constexpr int kBuf = TOperandFetch<T>::kBuf;
  T* diag_ws[kBuf] = {nullptr, nullptr, nullptr};
  T* tpanel[kBuf] = {nullptr, nullptr, nullptr};
  T* tstage[kBuf] = {nullptr, nullptr, nullptr};
  T* xpanel[kBuf] = {nullptr, nullptr, nullptr};
  for (int b = 0; b < kBuf; ++b) {
    diag_ws[b] = tm_dev_alloc<T>(tile_elems);
    if (dist) {
      tpanel[b] = tm_dev_alloc<T>((size_t) Bd.ltc * tile_elems);
      if (!aligned)
        tstage[b] = tm_dev_alloc<T>((size_t) Td.ltr * tile_elems);
      xpanel[b] = tm_dev_alloc<T>((size_t) Bd.ltr * tile_elems);
    }
  }

  const std::vector<long> my_diag;  // (no inverted blocks)
  std::vector<TOperand<T>> top((size_t) nt);
  TOperandFetch<T> tf{Td, Bd, tr, upper, !upper, s_comm, my_diag, nullptr, 0, diag_ws, tpanel, tstage,
                      ev_m.v.data(), ev_t.v.data(), top};
  std::vector<const T*> xp((size_t) nt, nullptr);  // P_k of step s as the update's first operand

  // s_comm: the T operands of step s and the original column k to the other members of my Bd row
  auto fetch = [&](long s) {
    tf.fetch(s);
    const long k = tf.step_k(s);
    const bool in_col = Bd.cols.mine(k);
    const T* p = in_col ? Bd.tile(0, Bd.cols.local_of(k)) : nullptr;
    if (Bd.cols.P > 1) {
      T* dst = in_col ? Bd.tile(0, Bd.cols.local_of(k)) : xpanel[s % kBuf];
      if (Bd.ltr > 0)
        tr->bcast(along_row, Bd.cols.owner(k), Bd.cols.rank, dst, dst, (size_t) Bd.ltr * tile_bytes, s_comm);
      p = dst;
      DLAF_HIP_CHECK(hipEventRecord(ev_xb[(size_t) s], s_comm));
    }
    xp[(size_t) s] = p;
  };

  auto update = [&](long s, long j0, long j1) {
    const TOperand<T>& o = top[(size_t) s];
    j0 = std::max(j0, o.jl0);
    j1 = std::min(j1, o.jl1);
    if (j0 >= j1 || Bd.ltr == 0)
      return;
    const long k = tf.step_k(s);
    UpdateArgs<T> ua;
    ua.c = Bd.tiles;
    ua.c_tsr = (long) tile_elems;
    ua.c_tsc = (long) (tile_elems * Bd.ltr);
    ua.ldc = nb;
    ua.a = xp[(size_t) s];
    ua.a_ts = (long) tile_elems;
    ua.lda = nb;
    ua.b = o.base + (j0 - o.jl0) * o.ts;
    ua.b_ts = o.ts;
    ua.ldb = nb;
    ua.il0 = 0;
    ua.il1 = (int) Bd.ltr;
    ua.jl0 = (int) j0;
    ua.jl1 = (int) j1;
    ua.nb = nb;
    ua.K = Bd.cols.tile_extent(k);
    ua.pr = Bd.rows.P;
    ua.ri = Bd.rows.shift();
    ua.pc = Bd.cols.P;
    ua.ci = Bd.cols.shift();
    ua.nt = (int) Bd.rows.nt();
    ua.last_rows = Bd.rows.last_extent();
    ua.rect = 1;
    ua.nt_c = (int) nt;
    ua.last_cols = Bd.cols.last_extent();
    ua.info = info;
    launch_update(ua, s_main, 4);
  };

  hipEvent_t ev_t0, ev_t1;
  DLAF_HIP_CHECK(hipEventCreate(&ev_t0));
  DLAF_HIP_CHECK(hipEventCreate(&ev_t1));
  DLAF_HIP_CHECK(hipEventRecord(ev_t0, s_main));
  DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, ev_t0, 0));

  // ---- the sweep --------------------------------------------------------------------------------------
  // s_main: U(s, all but the previous step's column) . [TRMM(s-1) done] . U(s, that column) -- the TRMM of step s-1
  // runs on s_side under the bulk of step s's update; operands arrive one step ahead on s_comm
  fetch(0);
  for (long s = 0; s < nt; ++s) {
    const long k = tf.step_k(s);
    if (s + 1 < nt)
      fetch(s + 1);
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, ev_t[(size_t) s], 0));
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
      TrmmArgs<T> ta;
      ta.b = Bd.tile(0, Bd.cols.local_of(k));
      ta.b_ts = (long) tile_elems;
      ta.ldb = nb;
      ta.il0 = 0;
      ta.il1 = (int) Bd.ltr;
      ta.pr = Bd.rows.P;
      ta.ri = Bd.rows.shift();
      ta.nb = nb;
      ta.nt = (int) Bd.rows.nt();
      ta.last_rows = Bd.rows.last_extent();
      ta.l = top[(size_t) s].diag;
      ta.ldl = nb;
      ta.n = Bd.cols.tile_extent(k);
      ta.upper = upper ? 1 : 0;
      ta.unit = unit ? 1 : 0;
      launch_trmm(ta, s_side);
    }
    DLAF_HIP_CHECK(hipEventRecord(ev_m[(size_t) s], s_side));
  }
  DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, ev_m[(size_t) (nt - 1)], 0));

  DLAF_HIP_CHECK(hipEventRecord(ev_t1, s_main));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_comm));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_side));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_main));
  {
    float ms = 0;
    DLAF_HIP_CHECK(hipEventElapsedTime(&ms, ev_t0, ev_t1));
    g_last_mult_ms = ms;
    // whole-grid algorithmic flops: rows x n^2 (x4 complex), as for the solve
    g_last_mult_flops = (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (double) Bd.rows_global * (double) Bd.cols.n * (double) Bd.cols.n;
  }
  (void) hipEventDestroy(ev_t0);
  (void) hipEventDestroy(ev_t1);
  (void) hipStreamDestroy(s_main);
  (void) hipStreamDestroy(s_side);
  (void) hipStreamDestroy(s_comm);
  (void) hipFree(info);
  for (int b = 0; b < kBuf; ++b) {
    (void) hipFree(diag_ws[b]);
    if (tpanel[b])
      (void) hipFree(tpanel[b]);
    if (tstage[b])
      (void) hipFree(tstage[b]);
    if (xpanel[b])
      (void) hipFree(xpanel[b]);
  }
}

}  // namespace

void multiplication_last_profile(double* ms, double* flops) {
  if (ms)
    *ms = g_last_mult_ms;
  if (flops)
    *flops = g_last_mult_flops;
}

template <class T>
int triangular_multiplication_host(Grid* g, char side, char uplo, char op, char diag, T alpha, const T* a, long lda,
                                   int a_isrc, int a_jsrc, T* b, long ldb, long m, long n, int nb, int b_isrc, int b_jsrc,
                                   int nb_free) {
  return triangular_canonical_host<T>("triangular multiplication", multiply_canonical<T>, false, g, side, uplo, op, diag,
                                      alpha, a, lda, a_isrc, a_jsrc, b, ldb, m, n, nb, b_isrc, b_jsrc, nb_free);
}

int triangular_multiplication_device(char side, char uplo, char op, char diag, const void* alpha, MatrixBase* a,
                                     MatrixBase* b) {
  if (!a || !b || a->type != b->type)
    fatal("[dlaf_mi355x] triangular multiplication: operands of different element types\n");
  auto run = [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    return triangular_canonical_device<T>("triangular multiplication", multiply_canonical<T>, side, uplo, op, diag,
                                          *static_cast<const T*>(alpha), static_cast<DeviceMatrix<T>&>(*a),
                                          static_cast<GeneralMatrix<T>&>(*b));
  };
  switch (a->type) {
    case 's': return run((float*) nullptr);
    case 'd': return run((double*) nullptr);
    case 'c': return run((cfloat*) nullptr);
    case 'z': return run((cdouble*) nullptr);
    default: fatal("[dlaf_mi355x] bad matrix type\n");
  }
}

template int triangular_multiplication_host<float>(Grid*, char, char, char, char, float, const float*, long, int, int,
                                                   float*, long, long, long, int, int, int, int);
template int triangular_multiplication_host<double>(Grid*, char, char, char, char, double, const double*, long, int, int,
                                                    double*, long, long, long, int, int, int, int);
template int triangular_multiplication_host<cfloat>(Grid*, char, char, char, char, cfloat, const cfloat*, long, int, int,
                                                    cfloat*, long, long, long, int, int, int, int);
template int triangular_multiplication_host<cdouble>(Grid*, char, char, char, char, cdouble, const cdouble*, long, int,
                                                     int, cdouble*, long, long, long, int, int, int, int);

}  // namespace dlaf_mi355x
