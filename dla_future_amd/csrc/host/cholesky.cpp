// cholesky.cpp -- the issue side of the tile Cholesky: which kernels, broadcasts and events one factorization
// enqueues on the three streams of a DeviceMatrix, in one of four orders.  See device_matrix.hpp for the matrix,
// transport.hpp for the transports, device_matrix.cpp for wait() and the blocking entry points.
#include "device_matrix.hpp"
#include "launch_args.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace dlaf_mi355x {

// ------------------------------------------------------------------------------- tile POTRF
// Blocked lower Cholesky of one kb x kb tile (ld) with inner block 64: diagonal block kernel,
// sub-panel solve (TRSM kernel, one column block), in-tile trailing update (update kernel).
// winv receives the ceil(kb/64) inverted diagonal blocks.  Replaces rocsolver potrf
// (lapack/tile.h:577-606).
static bool potrf_use_chain() {
  static const bool chain = [] {
    const char* e = std::getenv("DLAF_MI355X_POTRF");
    return e && std::strcmp(e, "chain") == 0;
  }();
  return chain;
}

// One resident cooperative launch (kernels_potrf_coop.hip).  The factorization passes sync_is_zero (it zeroed sync
// itself) and count_strips: the strips register for the POTRF yield, on one process and on grids.
template <class T>
void potrf_tile_coop(T* t, int ld, int kb, T* winv, int* info, int info_base, unsigned* sync, hipStream_t s,
                     bool sync_is_zero, bool count_strips) {
  launch_potrf_coop(t, ld, kb, winv, info, info_base, sync, s, sync_is_zero, count_strips);
}

// The multi-launch form: diagonal block kernel + TRSM kernel + update kernel per 64 columns.
template <class T>
void potrf_tile_chain(T* t, int ld, int kb, T* winv, int* info, int info_base, hipStream_t s) {
  constexpr int JB = kDiagBlock;
  for (int j0 = 0; j0 < kb; j0 += JB) {
    const int jb = std::min(JB, kb - j0);
    T* djj = t + j0 + (size_t) j0 * ld;
    T* wj = winv + (size_t) (j0 / JB) * JB * JB;
    launch_potrf_diag(djj, ld, jb, wj, info, info_base + j0, s);
    const int rem = kb - j0 - jb;
    if (rem <= 0)
      break;
    T* sub = t + (j0 + jb) + (size_t) j0 * ld;  // rem x jb panel below the diagonal block
    TrsmArgs<T> ta;
    ta.b = sub;
    ta.b_ts = 0;
    ta.ldb = ld;
    ta.il0 = 0;
    ta.il1 = 1;
    ta.pr = 1;
    ta.ri = 0;
    ta.nb = rem;
    ta.nt = 1;
    ta.last_rows = rem;
    ta.l = djj;
    ta.ldl = ld;
    ta.winv = wj;
    ta.n = jb;
    ta.info = info;
    launch_trsm(ta, s);
    UpdateArgs<T> ua;
    ua.c = t + (j0 + jb) + (size_t) (j0 + jb) * ld;
    ua.c_tsr = ua.c_tsc = 0;
    ua.ldc = ld;
    ua.a = sub;
    ua.a_ts = 0;
    ua.lda = ld;
    ua.b = sub;
    ua.b_ts = 0;
    ua.ldb = ld;
    ua.il0 = ua.jl0 = 0;
    ua.il1 = ua.jl1 = 1;
    ua.nb = rem;
    ua.K = jb;
    ua.pr = ua.pc = 1;
    ua.ri = ua.ci = 0;
    ua.nt = 1;
    ua.last_rows = rem;
    ua.info = info;
    launch_update(ua, s, 2);
  }
}

// DLAF_MI355X_POTRF=chain selects the multi-launch form, anything else the cooperative launch.
template <class T>
void potrf_tile(T* t, int ld, int kb, T* winv, int* info, int info_base, unsigned* sync, hipStream_t s) {
  if (!potrf_use_chain())
    potrf_tile_coop(t, ld, kb, winv, info, info_base, sync, s, /* sync_is_zero */ true, /* count_strips */ true);
  else
    potrf_tile_chain(t, ld, kb, winv, info, info_base, s);
}

// ------------------------------------------------------------------------------- transposed panel
static long gcd_l(long a, long b) {
  while (b) {
    const long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

template <class T>
int DeviceMatrix<T>::bcast_transposed_panel(Transport* tr, CommAxis ax_col, const T* a_base, long il_n, long jl_n,
                                            T* dst, hipStream_t s, int& period, long& ts2) {
  const size_t tile_bytes = tile_elems * sizeof(T);
  const long ncols = ltc - jl_n;
  // owner(global_of(jl)) repeats in jl with period lcm(Pr, Pc) / Pc = Pr / gcd(Pr, Pc)
  const long g = gcd_l(rows.P, cols.P);
  period = (int) (rows.P / g);
  const long lstep = cols.P / g;  // local-row distance on the root between consecutive tiles of a class
  const long cap = ncols > 0 ? (ncols + period - 1) / period : 0;
  ts2 = cap * (long) tile_elems;
  int issued = 0;
  tr->group_begin();
  for (long c = 0; c < period && c < ncols; ++c) {
    const long jl_first = jl_n + c;
    const long gj_first = cols.global_of(jl_first);
    const int root_r = rows.owner(gj_first);
    long cnt = (ncols - c + period - 1) / period;
    if (cols.global_of(jl_first + (cnt - 1) * period) == nt - 1)
      --cnt;
    if (cnt <= 0)
      continue;
    T* d = dst + c * ts2;
    if (rows.rank == root_r) {
      const T* src = a_base + (size_t) (rows.local_of(gj_first) - il_n) * tile_elems;
      DLAF_HIP_CHECK(hipMemcpy2DAsync(d, tile_bytes, src, (size_t) lstep * tile_bytes, tile_bytes, (size_t) cnt,
                                      hipMemcpyDeviceToDevice, s));
    }
    tr->bcast(ax_col, root_r, rows.rank, d, d, (size_t) cnt * tile_bytes, s);
    ++issued;
  }
  tr->group_end();
  return issued;
}

// ------------------------------------------------------------------------------- the tile DAG
// Right-looking Cholesky (cholesky/impl.h:150-189 local, :192-313 distributed) of the lower
// triangle of the view.  Three in-order streams; events carry the RAW/WAR edges the reference gets
// from per-tile async_rw_mutex.  U(k, J) = trailing update of tile columns J with panel k.
//
// "classic" schedule (one process):
//
//   s_main : U(k-1, col k) . U(k-1, rest_A) . TRSM(k) . U(k-1, rest_B) . U(k, col k+1) . U(k, rest_A) ...
//   s_panel:                  POTRF(k)                                     POTRF(k+1)
//
// the narrow, latency-bound POTRF of the NEXT diagonal tile runs beside the first slice (rest_A) of the
// current bulk update in workgroup slots that slice leaves free.  This is the reference's lookahead rule
// (high priority for potrf/trsm and for trailing column k+1, impl.h:172-173 / :280-281) expressed as an
// explicit order, because on this GPU a high-priority stream's kernels do not pre-empt the queued
// workgroups of a running bulk kernel.
//
// "sidecar" schedule (one process, real types, nb <= 768, where a step's bulk is short and the serial TRSM
// and the split of the bulk into two launches cost most): POTRF(k) AND TRSM(k) ride on s_panel beside the
// WHOLE bulk update of step k-1, one persistent launch that leaves 32 workgroup slots free; the lookahead
// column follows both:
//
//   s_main : U(k-1, rest) ................. U(k, col k+1) . U(k, rest) ...
//   s_panel: POTRF(k) . TRSM(k)                              POTRF(k+1) . TRSM(k+1)
//
// Measured (one MI355X, fp64): nb=512 N=32768 48.6 -> 52.5 TFlop/s, nb=256 N=16384 27.6 -> 30.1, nb=768
// 47.6 -> 51.0; at nb=1024 the classic order with its tuned lookahead slice is 2 % faster, and for complex
// types (one TRSM workgroup per compute unit) it is 3 % faster at every size tried.
//
// "pairs" schedule (one process, the default there): the bulk update takes the panels of TWO steps per pass
// (K = 2 nb): half the read-modify-write traffic of the trailing matrix, half the launches, half the per-block
// epilogues -- what a small block size loses against nb = 1024, and 1.5 % at nb = 1024 itself (measured fp64:
// N=32768 nb=512 55.0 -> 57.2 TFlop/s, N=65536 nb=1024 64.9 -> 65.9; z N=32768 nb=512 57.3 -> 59.7).  Its
// diagram is at issue_pairs().
//
// "early diagonal" schedule (process grids): with broadcasts in the loop the per-step chain POTRF -> bcast ->
// TRSM -> bcast -> U(col k+1) -> POTRF is what bounds a multi-GPU run, so the diagonal tile leaves that chain.
// The lookahead is two columns deep, the panel's first tile ("head": A(k+1,k), the only operand D(k+1) needs)
// is solved and broadcast ahead of the rest, and D(k+1) is updated and factored on s_panel while the panel of
// step k is still on the wire:
//
//   s_main : TRSMhead(k) . TRSMtail(k) . U(k-1, cols >= k+2) . U(k, cols {k+1,k+2} below D(k+1)) . TRSMhead(k+1) ...
//   s_comm : [diag(k)]  head(k) . tail(k) . panelT(k)                                  [diag(k+1)] head(k+1) ...
//   s_panel:             herk D(k+1) -= head head^H . POTRF(k+1)
namespace {

enum class Schedule { Pairs, Sidecar, Early, Classic };

// DLAF_MI355X_SCHEDULE=pairs|sidecar|early|classic overrides the default; pairs and sidecar are one-process
// orders, asked for on a grid they give classic.  Read at every factorization: tests switch it in one process.
Schedule choose_schedule(bool dist, int nb, bool complex_type) {
  const char* e = std::getenv("DLAF_MI355X_SCHEDULE");
  if (e == nullptr) {
    if (dist)
      return Schedule::Early;
    if (nb % 16 == 0)
      return Schedule::Pairs;
    return !complex_type && nb <= 768 ? Schedule::Sidecar : Schedule::Classic;
  }
  if (std::strcmp(e, "early") == 0)
    return Schedule::Early;
  if (!dist && std::strcmp(e, "pairs") == 0)
    return Schedule::Pairs;
  if (!dist && std::strcmp(e, "sidecar") == 0)
    return Schedule::Sidecar;
  return Schedule::Classic;
}

// Workgroup slots the bulk update of the one-process orders leaves free for the panel work beside it: the
// POTRF's strips plus a few TRSM workgroups.  The measured optimum while the bulk outlasts the panel chain (16 ->
// 65.5, 32 -> 67.4, 48 -> 66.8 TFlop/s at N=65536 nb=1024).
constexpr long kSidecarSlots = 32;

// Rate table of the pairs order's two placement decisions (in-situ measurements on MI355X):
// the bulk update, the panel TRSM per free slot beside it, the tile POTRF per (64-column block)^2 beside it.
// r_bulk of real fp64 was 66e12 while its bulk launch ran at 67.4 TFlop/s in situ; it runs at 71.2 since the K loop's
// fragment rotation and scalar slab bases, and the rate moved with it (N=65536 nb=1024: U1 goes to s_main one pair
// earlier, k = 30, and the reservation of pair k = 50 grows from 128 to 192 slots; profiles/kloop_slab_bases_ab.txt).
// The complex kernel has not changed and keeps its rate.
template <class T>
struct PairRates {
  static constexpr bool dbl = sizeof(real_t<T>) == 8;
  static constexpr double r_bulk = dbl ? (TypeInfo<T>::is_complex ? 66e12 : 70e12) : 118e12;
  static constexpr double r_trsm_slot = (dbl ? 5e12 : 8e12) / 32.0;
  static constexpr double t_potrf_blk2 = 11.3e-6 * (TypeInfo<T>::is_complex ? 2.0 : 1.0);  // 2.9 ms per real 1024-tile
};

// operands of step k's trailing update, kept until the update has been issued in full
template <class T>
struct Step {
  const T* a_base = nullptr;  // column panel: tile of local row il at a_base + (il - il_n)*tile_elems
  const T* b_base = nullptr;  // transposed panel: tile of local col jl at b_base + (jl - jl_n)*b_ts
  long b_ts = 0, il_n = 0, jl_n = 0;
  int b_period = 1;  // transposed panel grouped by root process row: see bcast_transposed_panel
  long b_ts2 = 0;
  // two panels applied in one pass (one process, "pairs" order): columns k1 .. kb-1 of the operands are
  // the panel of the following step
  const T* a2_base = nullptr;
  const T* b2_base = nullptr;
  int k1 = 0;
  int kb = 0;
  long rest0 = 0, split = 0;  // classic: rest_A = [rest0, split), rest_B = [split, ltc); early: rest = [rest0, ltc)
  bool valid = false;

  // The panel of one step (kb columns).  Until transposed_panel() replaces it, the column panel is its own
  // transposed operand: what it is on one process, where tile column jl_n + i is tile row il_n + i.
  static Step one_panel(int kb, long il_n, long jl_n, const T* a_base, size_t tile_elems) {
    Step st;
    st.valid = true;
    st.kb = kb;
    st.il_n = il_n;
    st.jl_n = jl_n;
    st.a_base = st.b_base = a_base;
    st.b_ts = (long) tile_elems;
    return st;
  }
  // The panels of two consecutive steps (k1 + k2 columns) on one process, both starting at local row and column n0.
  static Step two_panels(int k1, int k2, long n0, const T* a_base, const T* a2_base, size_t tile_elems) {
    Step st = one_panel(k1 + k2, n0, n0, a_base, tile_elems);
    st.k1 = k1;
    st.a2_base = st.b2_base = a2_base;
    return st;
  }
};

// One factorization of m: the operations every order is built of, and one member function per order.
template <class T>
struct CholeskyIssue {
  using StepT = Step<T>;
  DeviceMatrix<T>& m;
  Transport* tr;
  const bool dist;
  const size_t tile_bytes;
  // uplo == 'U' runs on the transposed view: its process rows are the caller's process columns
  const CommAxis ax_row, ax_col;
  const hipStream_t s_main, s_panel, s_comm;
  // Workgroup slots kept free by the bulk launches for the cooperative POTRF of the next diagonal tile
  // (one workgroup per 64 rows) and for the RCCL broadcast kernels of the step.
  long potrf_slots = 0, comm_slots = 0;
  // early-diagonal order: what the bulk leaves to the tile POTRF and the transport's kernels (a whole round over the
  // shader engines -- 64 slots: nb = 1024 with a device-side transport -- is made as exclusive compute units, see
  // `update`; otherwise the strips share compute units and the bulk workgroups beside them sit out)
  long grid_reserve = 0;
  size_t next_update_slice = 0;  // next pre-zeroed counter slice of coop_sync for a persistent update launch

  explicit CholeskyIssue(DeviceMatrix<T>& mat)
      : m(mat), tr(checked_transport(*mat.grid)), dist(mat.grid->nranks > 1), tile_bytes(mat.tile_elems * sizeof(T)),
        ax_row(mat.transposed ? CommAxis::Col : CommAxis::Row),
        ax_col(mat.transposed ? CommAxis::Row : CommAxis::Col), s_main(mat.s_low), s_panel(mat.s_high),
        s_comm(mat.s_comm) {
    if (const char* e = std::getenv("DLAF_MI355X_POTRF_SLOTS"))
      potrf_slots = std::atol(e);
    else
      potrf_slots = potrf_use_chain() ? 0 : 2 * ((m.nb + kDiagBlock - 1) / kDiagBlock);
    if (const char* e = std::getenv("DLAF_MI355X_COMM_SLOTS"))
      comm_slots = std::atol(e);
    else
      comm_slots = (dist && tr->device_side()) ? 32 : 0;
    grid_reserve = potrf_slots + comm_slots;
  }

  StepT one_panel(long k, long il_n, long jl_n, const T* a_base) const {
    return StepT::one_panel(m.rows.tile_extent(k), il_n, jl_n, a_base, m.tile_elems);
  }

  // algorithmic work of one grouped update launch (BASELINE.md roofline table):
  // gemm tile 2 m n k flop / (m k + n k + 2 m n) elements, herk tile n (n+1) k flop / (n k + n^2) elements
  void update_work(long il0, long il1, long j0, long j1, int kb, double& flops, double& bytes) const {
    flops = bytes = 0;
    const double cx = TypeInfo<T>::is_complex ? 4.0 : 1.0;
    for (long jl = j0; jl < j1; ++jl) {
      const long gj = m.cols.global_of(jl);
      const double nj = m.rows.tile_extent(gj);
      for (long il = std::max(il0, m.rows.next_local(gj)); il < il1; ++il) {
        const long gi = m.rows.global_of(il);
        const double mi = m.rows.tile_extent(gi);
        if (gi == gj) {
          flops += cx * mi * (mi + 1) * kb;
          bytes += (mi * kb + mi * mi) * sizeof(T);
        }
        else {
          flops += cx * 2.0 * mi * nj * kb;
          bytes += (mi * kb + nj * kb + 2.0 * mi * nj) * sizeof(T);
        }
      }
    }
  }

  // flops of the update of local tile column jl, on and below the diagonal, with the panels of `st`
  double column_flops(const StepT& st, long jl) const {
    double f, by;
    update_work(std::max(st.il_n, m.rows.next_local(m.cols.global_of(jl))), m.ltr, jl, jl + 1, st.kb, f, by);
    return f;
  }

  // Update of local tile columns [j0, j1), local tile rows [max(il_from, diagonal), il_to) with the
  // panels of step `st`.  reserve: workgroup slots the launch must leave free (resident POTRF / RCCL
  // kernels run beside it).  kind: profile class.
  void update(const StepT& st, long j0, long j1, hipStream_t s, int role, long reserve, long il_from = -1,
              long il_to = -1, int kind = -1) {
    if (!st.valid || j0 >= j1)
      return;
    // rows that can hold tiles on/below the diagonal of column block j0
    const long il0 = std::max(std::max(st.il_n, il_from), m.rows.next_local(m.cols.global_of(j0)));
    const long il1 = il_to < 0 ? m.ltr : std::min(il_to, m.ltr);
    if (il0 >= il1)
      return;
    UpdateArgs<T> ua = update_args(m, il0, il1, j0, j1, st.a_base + (size_t) (il0 - st.il_n) * m.tile_elems, st.b_base,
                                   st.b_ts, st.kb, m.info);
    ua.b_period = st.b_period;
    ua.b_ts2 = st.b_ts2;
    ua.b_jl0 = (int) st.jl_n;
    if (st.k1 > 0) {
      ua.K1 = st.k1;
      ua.a2 = st.a2_base + (size_t) (il0 - st.il_n) * m.tile_elems;
      ua.b2 = st.b2_base;
    }
    double fl, by;
    update_work(il0, il1, j0, j1, st.kb, fl, by);
    const int pk = kind < 0 ? role : kind;
    m.prof_begin(pk, s);
    // (persistent launches only: each takes the next pre-zeroed slice; past the end of the pool -- never with the
    // schedules below -- the last slice is re-zeroed per launch)
    unsigned* cnt = m.coop_sync;
    bool zero = false;
    if (reserve > 0) {
      const size_t sl = std::min(next_update_slice, m.coop_sync_update_slices - 1);
      cnt = m.coop_sync + 16 * sl;
      zero = next_update_slice < m.coop_sync_update_slices - 1;
      ++next_update_slice;
    }
    // Reservations that are whole rounds over the shader engines (multiples of 64 slots on MI355X: the grid orders
    // with a device-side transport at nb = 1024, the widened reservations near the end of the pairs order) are made
    // as EXCLUSIVE compute units: the launch covers every slot and the workgroups that land on a reserved compute
    // unit leave (kernels_update.hip), so the tile POTRF beside it runs at its stand-alone speed (0.87 instead of
    // 2.3 ms per 1024-tile).  The others -- the 32 slots of the one-process orders, where 64 would cost the bulk
    // launch 7 % -- stay free slots.  DLAF_MI355X_EXCLUSIVE_CUS=0: free slots always.
    static const bool exclusive = [] {
      const char* e = std::getenv("DLAF_MI355X_EXCLUSIVE_CUS");
      return e ? std::atoi(e) != 0 : true;
    }();
    if (reserve > 0 && exclusive)
      launch_update(ua, s, role, m.bulk_slots, cnt, zero, reserve);
    else
      launch_update(ua, s, role, reserve > 0 ? std::max<long>(8, m.bulk_slots - reserve) : 0, cnt, zero);
    DLAF_HIP_CHECK(hipGetLastError());
    m.prof_end(pk, s, fl, by);
  }

  // panel TRSM of local tile rows [il0, il1) of local tile column klc with the factored diagonal tile
  void trsm(long il0, long il1, long klc, const T* Lkk, const T* Wkk, int kb, hipStream_t ts = nullptr) {
    if (ts == nullptr)
      ts = s_main;
    if (il0 >= il1)
      return;
    TrsmArgs<T> ta = panel_args<TrsmArgs<T>>(m, il0, il1, klc, Lkk, kb);
    ta.winv = Wkk;
    ta.info = m.info;
    // on the side stream the solve runs beside the bulk update and every later step waits for it
    ta.prio = (ts != s_main) ? 1 : 0;
    // algorithmic work: n^2 m flop and (n^2/2 + 2 m n) elements per tile
    double fl = 0, by = 0;
    for (long il = il0; il < il1; ++il) {
      const double mi = m.rows.tile_extent(m.rows.global_of(il));
      fl += (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (double) kb * kb * mi;
      by += (0.5 * kb * kb + 2.0 * mi * kb) * sizeof(T);
    }
    m.prof_begin(2, ts);
    launch_trsm(ta, ts);
    DLAF_HIP_CHECK(hipGetLastError());
    m.prof_end(2, ts, fl, by);
  }

  // diagonal tile k on its owner (s_panel); the inverted diagonal blocks alternate between two buffers
  // because POTRF(k+1) may run while TRSM(k) still reads those of step k
  T* winv_of(long k) const { return m.winv + (size_t) (k & 1) * m.winv_elems(); }
  T* diag_ws_of(long k) const { return m.diag_ws + (size_t) (k & 1) * (m.tile_elems + m.winv_elems()); }
  void potrf(long k) {
    if (m.rows.rank != m.rows.owner(k) || m.cols.rank != m.cols.owner(k))
      return;
    const int kb = m.rows.tile_extent(k);
    const double cxf = TypeInfo<T>::is_complex ? 4.0 : 1.0;
    m.prof_begin(3, s_panel);
    potrf_tile(m.tile(m.rows.local_of(k), m.cols.local_of(k)), m.nb, kb, winv_of(k), m.info, (int) (k * m.nb),
               m.coop_sync + 16 * m.coop_sync_update_slices + m.coop_sync_potrf_words * (size_t) k, s_panel);
    DLAF_HIP_CHECK(hipGetLastError());  // (a launch that did not happen leaves winv unwritten and info 0)
    m.prof_end(3, s_panel, cxf * (double) kb * kb * kb / 3.0, (double) kb * kb * sizeof(T));
  }

  // after POTRF(k) on s_panel: the factored tile and its inverse blocks travel down the owning process
  // column; returns through Lkk / Wkk what TRSM(k) reads and records ev_diag[k] when that is ready
  void diag_bcast(long k, bool in_row, bool in_col, const T*& Lkk, const T*& Wkk) {
    Lkk = Wkk = nullptr;
    if (in_row && in_col) {
      Lkk = m.tile(m.rows.local_of(k), m.cols.local_of(k));
      Wkk = winv_of(k);
    }
    if (in_col && m.rows.P > 1) {
      T* ws = diag_ws_of(k);
      if (in_row) {
        DLAF_HIP_CHECK(hipMemcpyAsync(ws, Lkk, tile_bytes, hipMemcpyDeviceToDevice, s_panel));
        DLAF_HIP_CHECK(hipMemcpyAsync(ws + m.tile_elems, Wkk, m.winv_elems() * sizeof(T), hipMemcpyDeviceToDevice, s_panel));
      }
      DLAF_HIP_CHECK(hipEventRecord(m.ev_diag[k], s_panel));
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, m.ev_diag[k], 0));
      tr->bcast(ax_col, m.rows.owner(k), m.rows.rank, ws, ws, tile_bytes + m.winv_elems() * sizeof(T), s_comm);
      DLAF_HIP_CHECK(hipEventRecord(m.ev_diag[k], s_comm));
      Lkk = ws;
      Wkk = ws + m.tile_elems;
    }
    else {
      DLAF_HIP_CHECK(hipEventRecord(m.ev_diag[k], s_panel));
    }
  }

  // transposed panel of a step down the process columns (after the row broadcast), or the view of the
  // column panel that plays its role when this process holds every row
  void transposed_panel(StepT& cur, int buf) {
    if (m.rows.P > 1) {
      m.bcast_transposed_panel(tr, ax_col, cur.a_base, cur.il_n, cur.jl_n, m.panelT[buf], s_comm, cur.b_period,
                               cur.b_ts2);
      cur.b_base = m.panelT[buf];
      cur.b_ts = (long) m.tile_elems;
    }
    else {
      // I hold every row of the panel: tile gj sits at local row gj
      cur.b_base = cur.a_base + (m.cols.global_of(cur.jl_n) - cur.il_n) * (long) m.tile_elems;
      cur.b_ts = (long) m.tile_elems * m.cols.P;
    }
  }

  // the last diagonal tile: s_main waits for its POTRF
  void join_last_diag(long k) {
    DLAF_HIP_CHECK(hipEventRecord(m.ev_diag[k], s_panel));
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_diag[k], 0));
  }

  // the panel of step k is solved: ev_panel[k] on stream s (factorize_and_download follows it)
  void panel_done(long k, hipStream_t s) {
    DLAF_HIP_CHECK(hipEventRecord(m.ev_panel[k], s));
    m.panels_issued.store(k, std::memory_order_release);
  }

  // Workgroup slots rest(p-1) leaves free for the panel work of pair p running beside it (pair p = steps k, k+1;
  // bulk_flops: the flops of rest(p-1)).  kSidecarSlots while the bulk outlasts the panel chain 2 POTRF + 2 TRSM
  // beside it; towards the end of the factorization the bulk of a pair is shorter than the chain, and there the
  // reservation grows until the two balance (the TRSM's throughput is proportional to the slots it finds).
  long pair_slots(long k, double bulk_flops) const {
    using R = PairRates<T>;
    const long nb = m.nb, bulk_slots = m.bulk_slots;
    const double cxf = TypeInfo<T>::is_complex ? 4.0 : 1.0;
    const double below = (double) std::max<long>(0, m.n - (k + 1) * nb) + (double) std::max<long>(0, m.n - (k + 2) * nb);
    const double fl_t = cxf * (double) nb * nb * below;
    const double nblk = (double) nb / kDiagBlock;
    const double t_potrf = 2.0 * nblk * nblk * R::t_potrf_blk2;
    auto t_of = [&](long sl) {
      const double share = (double) sl / (double) bulk_slots;
      return std::max(bulk_flops / (R::r_bulk * (1.0 - share)), t_potrf + fl_t / (R::r_trsm_slot * (double) sl));
    };
    long best = kSidecarSlots;
    double best_t = t_of(best);
    if (bulk_flops / (R::r_bulk * (1.0 - (double) best / (double) bulk_slots)) >= best_t)
      return best;  // the bulk is the longer of the two: nothing to gain
    for (long cand : {48L, 64L, 96L, 128L, 192L, 256L}) {
      if (cand <= kSidecarSlots || cand * 2 > bulk_slots)
        continue;
      const double t = t_of(cand);
      if (t < best_t) {
        best_t = t;
        best = cand;
      }
    }
    return best;
  }

  // U1 (column k+1 under panel k) is on the chain POTRF(k) . TRSM(k) . U1 . POTRF(k+1) . TRSM(k+1).  Two places
  // for it: (a) on s_panel beside the bulk, on the few slots the bulk leaves free -- ~16 ms instead of 1 ms at
  // N=65536 nb=1024, harmless while the bulk of the pair outlasts the chain anyway; (b) alone on s_main between
  // two halves of the bulk -- the chain shrinks to what the GPU can do, at the price of a second ramp-down of
  // the persistent bulk launch.  (a) while the bulk is the longer of the two, (b) towards the end.
  bool u1_on_main(long k, long slots, double bulk_flops) const {
    using R = PairRates<T>;
    const long nb = m.nb;
    const double cxf = TypeInfo<T>::is_complex ? 4.0 : 1.0;
    const double below1 = (double) std::max<long>(0, m.n - (k + 1) * nb), below2 = (double) std::max<long>(0, m.n - (k + 2) * nb);
    const double fl_chain = cxf * (double) nb * nb * (below1 + below2) + cxf * 2.0 * (double) nb * nb * below1;  // 2 TRSM + U1
    const double nblk = (double) nb / kDiagBlock;
    const double t_chain = 2.0 * nblk * nblk * R::t_potrf_blk2 + fl_chain / (R::r_trsm_slot * (double) slots);
    const double t_bulk = bulk_flops / (R::r_bulk * (1.0 - (double) slots / (double) m.bulk_slots));
    return t_bulk < t_chain;
  }

  void issue_pairs();
  void issue_sidecar();
  void issue_early();
  void issue_classic();
};

template <class T>
void CholeskyIssue<T>::issue_pairs() {
  // s_main : LA(p-1) . restA(p-1) ........ U1(k -> col k+1) . restB(p-1) ................. LA(p) . restA(p) ...
  // s_panel:           POTRF(k) . TRSM(k) ^                    POTRF(k+1) . TRSM(k+1) ^
  // pair p = steps (k, k+1); LA(p) = the two-panel update of tile columns k+2, k+3 (what the next pair's panels
  // need), rest(p) = columns >= k+4 in two persistent launches that leave pair_slots() free for the panel
  // kernels beside them, U1 = column k+1 under panel k alone on s_main between the two (see u1_on_main()).
  constexpr double kSplitFrac = 0.3;  // share of rest(p-1) issued BEFORE U1 on s_main (beside POTRF(k) + TRSM(k))
  const long nt = m.nt, ltr = m.ltr, ltc = m.ltc;
  StepT prev;  // the pair before, whose bulk rest(p-1) is still to be issued
  for (long k = 0; k < nt; k += 2) {
    if (tr)
      tr->mark(k);
    if (k >= 2)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_panel, m.ev_high[k - 2], 0));  // LA(p-1): columns k, k+1 are final
    potrf(k);
    const bool second = k + 1 < nt;  // the pair has a second step
    const bool more = k + 2 < nt;    // something trails the pair
    if (second) {
      trsm(k + 1, ltr, k, m.tile(k, k), winv_of(k), m.rows.tile_extent(k), s_panel);
      panel_done(k, s_panel);
    }
    // per-column flops of rest(p-1), summed in column order: one list for both placement decisions
    const bool bulk = prev.valid && prev.rest0 < ltc;
    std::vector<double> colfl;
    double bulk_flops = 0;
    for (long jl = bulk ? prev.rest0 : ltc; jl < ltc; ++jl) {
      colfl.push_back(column_flops(prev, jl));
      bulk_flops += colfl.back();
    }
    const long slots = bulk ? pair_slots(k, bulk_flops) : kSidecarSlots;
    // with nothing to run beside, U1 goes on s_main: plain sequence
    const bool u1_main = second && (!bulk || u1_on_main(k, slots, bulk_flops));
    long splitA = prev.rest0;
    if (u1_main && bulk) {
      double acc = 0;
      while (splitA < ltc && acc < kSplitFrac * bulk_flops)
        acc += colfl[(size_t) (splitA++ - prev.rest0)];
    }
    update(prev, prev.rest0, splitA, s_main, 0, slots);
    if (second) {
      const StepT u1 = one_panel(k, k + 1, k + 1, m.tile(k + 1 < ltr ? k + 1 : 0, k));
      if (u1_main) {
        DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_panel[k], 0));
        update(u1, k + 1, k + 2, s_main, 1, 0);
        DLAF_HIP_CHECK(hipEventRecord(m.ev_head[k], s_main));
        DLAF_HIP_CHECK(hipStreamWaitEvent(s_panel, m.ev_head[k], 0));
      }
      else {
        update(u1, k + 1, k + 2, s_panel, 1, 0);
      }
      potrf(k + 1);
      if (more) {
        trsm(k + 2, ltr, k + 1, m.tile(k + 1, k + 1), winv_of(k + 1), m.rows.tile_extent(k + 1), s_panel);
        panel_done(k + 1, s_panel);
      }
    }
    update(prev, splitA, ltc, s_main, 0, slots);
    if (!more) {
      join_last_diag(k);
      break;
    }
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_panel[k + 1], 0));
    StepT cur = StepT::two_panels(m.rows.tile_extent(k), m.rows.tile_extent(k + 1), k + 2, m.tile(k + 2, k),
                                  m.tile(k + 2, k + 1), m.tile_elems);
    update(cur, k + 2, std::min<long>(k + 4, ltc), s_main, 1, 0);
    DLAF_HIP_CHECK(hipEventRecord(m.ev_high[k], s_main));
    cur.rest0 = std::min<long>(k + 4, ltc);
    prev = cur;
  }
}

template <class T>
void CholeskyIssue<T>::issue_sidecar() {
  const long nt = m.nt, ltr = m.ltr, ltc = m.ltc;
  StepT prev;  // step k-1, whose bulk update is still to be issued
  for (long k = 0; k < nt; ++k) {
    const int kb = m.rows.tile_extent(k);
    if (tr)
      tr->mark(k);
    const long il_n = m.rows.next_local(k + 1), jl_n = m.cols.next_local(k + 1);
    const long klc = m.cols.local_of(k);
    if (k >= 1)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_panel, m.ev_high[k - 1], 0));
    potrf(k);
    if (k == nt - 1) {
      update(prev, prev.rest0, ltc, s_main, 0, kSidecarSlots);
      join_last_diag(k);
      break;
    }
    trsm(il_n, ltr, klc, m.tile(m.rows.local_of(k), klc), winv_of(k), kb, s_panel);
    panel_done(k, s_panel);
    // the whole bulk of step k-1 beside them
    update(prev, prev.rest0, ltc, s_main, 0, kSidecarSlots);
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_panel[k], 0));
    StepT cur = one_panel(k, il_n, jl_n, m.tile(il_n < ltr ? il_n : 0, klc));
    transposed_panel(cur, 0);  // (one process: the view of the column panel, no communication)
    cur.rest0 = jl_n;
    if (jl_n < ltc) {
      update(cur, jl_n, jl_n + 1, s_main, 1, 0);
      cur.rest0 = jl_n + 1;
    }
    DLAF_HIP_CHECK(hipEventRecord(m.ev_high[k], s_main));
    prev = cur;
  }
}

template <class T>
void CholeskyIssue<T>::issue_early() {
  const long nt = m.nt, ltr = m.ltr, ltc = m.ltc;
  StepT prev;  // step k-1, whose bulk update is still to be issued
  potrf(0);
  for (long k = 0; k < nt; ++k) {
    const int kb = m.rows.tile_extent(k);
    if (tr)
      tr->mark(k);
    const int own_c = m.cols.owner(k);
    const bool in_row = m.rows.rank == m.rows.owner(k), in_col = m.cols.rank == own_c;
    const long il_n = m.rows.next_local(k + 1), jl_n = m.cols.next_local(k + 1);
    const int buf = (int) (k & 1);
    const long klc = in_col ? m.cols.local_of(k) : -1;
    if (k == nt - 1) {
      update(prev, prev.rest0, ltc, s_main, 0, 0);  // (empty: nothing lies right of column nt-1)
      join_last_diag(k);
      break;
    }
    const T *Lkk, *Wkk;
    diag_bcast(k, in_row, in_col, Lkk, Wkk);

    // ---- s_main: the head tile A(k+1,k) first, then the rest of the panel -------------------------
    // the head lives in process row owner(k+1), where it is the first local row below the diagonal
    const bool head_row = m.rows.rank == m.rows.owner(k + 1);
    const long il_t = il_n + (head_row ? 1 : 0);  // first local row of the tail
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_diag[k], 0));
    if (in_col && head_row)
      trsm(il_n, il_n + 1, klc, Lkk, Wkk, kb);
    DLAF_HIP_CHECK(hipEventRecord(m.ev_head[k], s_main));
    if (in_col)
      trsm(il_t, ltr, klc, Lkk, Wkk, kb);
    panel_done(k, s_main);

    // ---- s_comm: head, tail along process rows; transposed panel along process columns -----------
    // the workspace of step k-2 is free: its readers are behind TRSM(k) on s_main (ev_head[k])
    T* dst = in_col ? m.tile(il_n < ltr ? il_n : 0, klc) : m.panel[buf];
    StepT cur = one_panel(k, il_n, jl_n, dst);
    if (dist)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, m.ev_head[k], 0));
    if (m.cols.P > 1 && head_row)
      tr->bcast(ax_row, own_c, m.cols.rank, dst, dst, tile_bytes, s_comm);
    if (dist)
      DLAF_HIP_CHECK(hipEventRecord(m.ev_headb[k], s_comm));

    // ---- s_panel: D(k+1) -= head head^H, POTRF(k+1) -------------------------------------------------
    // (every earlier update of D(k+1) is in the two-column lookahead of step k-1: ev_high[k-1]; the herk tile
    // takes both operands from the column panel, as `cur` does before transposed_panel)
    if (head_row && m.cols.rank == m.cols.owner(k + 1)) {
      if (k >= 1)
        DLAF_HIP_CHECK(hipStreamWaitEvent(s_panel, m.ev_high[k - 1], 0));
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_panel, (dist && m.cols.P > 1) ? m.ev_headb[k] : m.ev_head[k], 0));
      update(cur, jl_n, jl_n + 1, s_panel, 2, 0, il_n, il_n + 1, 3);
      potrf(k + 1);
    }

    if (dist)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, m.ev_panel[k], 0));
    if (m.cols.P > 1 && il_t < ltr)
      tr->bcast(ax_row, own_c, m.cols.rank, dst + (size_t) (il_t - il_n) * m.tile_elems,
                dst + (size_t) (il_t - il_n) * m.tile_elems, (size_t) (ltr - il_t) * tile_bytes, s_comm);
    transposed_panel(cur, buf);
    if (dist)
      DLAF_HIP_CHECK(hipEventRecord(m.ev_bcast[k], s_comm));

    // ---- s_main: bulk of step k-1 beside the broadcasts of step k and POTRF(k+1) -----------------
    update(prev, prev.rest0, ltc, s_main, 0, grid_reserve);
    if (dist)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_bcast[k], 0));

    // ---- s_main: two-column lookahead of step k (D(k+1) itself is on s_panel) ----------------------
    cur.rest0 = m.cols.next_local(k + 3);
    update(cur, jl_n, cur.rest0, s_main, 1, 0, m.rows.next_local(k + 2));
    DLAF_HIP_CHECK(hipEventRecord(m.ev_high[k], s_main));
    prev = cur;
  }
}

template <class T>
void CholeskyIssue<T>::issue_classic() {
  // rest_A must last as long as the POTRF of the next diagonal tile takes BESIDE it: nb/64 dependent
  // sub-steps of ~90 us alone, 2-3x that under the bulk kernel's memory traffic (measured at nb = 1024:
  // 1.1 ms alone, 2.2-3.4 ms beside rest_A; the whole factorization is fastest with rest_A ~ 4 ms)
  const double lookahead_flops = 270e-6 * ((double) m.nb / kDiagBlock) * 55e12;
  const long nt = m.nt, ltr = m.ltr, ltc = m.ltc;
  StepT prev;  // step k-1, whose bulk update is still to be issued (in part or in full)
  for (long k = 0; k < nt; ++k) {
    const int kb = m.rows.tile_extent(k);
    if (tr)
      tr->mark(k);
    const int own_c = m.cols.owner(k);
    const bool in_row = m.rows.rank == m.rows.owner(k), in_col = m.cols.rank == own_c;
    const long il_n = m.rows.next_local(k + 1), jl_n = m.cols.next_local(k + 1);
    const int buf = (int) (k & 1);
    const long klc = in_col ? m.cols.local_of(k) : -1;

    // ---- s_panel: diagonal tile (column k is final once U(k-1, col k) has run: ev_high[k-1]) -------
    if (k >= 1)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_panel, m.ev_high[k - 1], 0));
    potrf(k);
    if (k == nt - 1) {
      // nothing trails the last diagonal tile; flush what is left of step k-1
      update(prev, prev.rest0, prev.split, s_main, 0, potrf_slots);
      update(prev, prev.split, ltc, s_main, 0, comm_slots);
      join_last_diag(k);
      break;
    }
    const T *Lkk, *Wkk;
    diag_bcast(k, in_row, in_col, Lkk, Wkk);

    // ---- s_main: first slice of the previous step's bulk update runs beside the POTRF -------------
    update(prev, prev.rest0, prev.split, s_main, 0, potrf_slots);

    // ---- s_main: panel TRSM --------------------------------------------------------------------------
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_diag[k], 0));
    if (in_col)
      trsm(il_n, ltr, klc, Lkk, Wkk, kb);
    panel_done(k, s_main);

    // ---- s_comm: panel along process rows, transposed panel along process columns ----------------
    // the workspace of step k-2 is free: its readers are behind TRSM(k) on s_main (ev_panel[k])
    T* dst = in_col ? m.tile(il_n < ltr ? il_n : 0, klc) : m.panel[buf];  // (one process column: in_col)
    StepT cur = one_panel(k, il_n, jl_n, dst);
    if (dist)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, m.ev_panel[k], 0));
    if (m.cols.P > 1 && il_n < ltr)
      tr->bcast(ax_row, own_c, m.cols.rank, dst, dst, (size_t) (ltr - il_n) * tile_bytes, s_comm);
    transposed_panel(cur, buf);
    if (dist)
      DLAF_HIP_CHECK(hipEventRecord(m.ev_bcast[k], s_comm));

    // ---- s_main: rest of step k-1 (the broadcasts of step k fly underneath) -------------------------
    update(prev, prev.split, ltc, s_main, 0, comm_slots);
    if (dist)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_main, m.ev_bcast[k], 0));

    // ---- s_main: lookahead column of step k, then split the rest ----------------------------------
    cur.rest0 = jl_n;
    if (m.cols.mine(k + 1) && jl_n < ltc) {
      update(cur, jl_n, jl_n + 1, s_main, 1, 0);
      cur.rest0 = jl_n + 1;
    }
    DLAF_HIP_CHECK(hipEventRecord(m.ev_high[k], s_main));
    cur.split = cur.rest0;
    for (double acc = 0; cur.split < ltc && acc < lookahead_flops; ++cur.split)
      acc += column_flops(cur, cur.split);
    prev = cur;
  }
}

}  // namespace

template <class T>
void DeviceMatrix<T>::factorize_async() {
  CholeskyIssue<T> f(*this);
  const Schedule schedule = choose_schedule(f.dist, nb, TypeInfo<T>::is_complex);

  for (auto& ps : prof) {
    ps.used = 0;
    ps.flops = ps.bytes = ps.ms = 0;
    ps.launches = 0;
  }
  DLAF_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), f.s_panel));
  DLAF_HIP_CHECK(hipMemsetAsync(coop_sync, 0, sizeof(unsigned) * coop_sync_words, f.s_panel));
  if (unsigned long long* tb = potrf_coop_trace_buffer())
    DLAF_HIP_CHECK(hipMemsetAsync(tb, 0, 32 * sizeof(unsigned long long), f.s_panel));
  DLAF_HIP_CHECK(hipEventRecord(ev_start[0], f.s_panel));
  DLAF_HIP_CHECK(hipStreamWaitEvent(f.s_main, ev_start[0], 0));
  DLAF_HIP_CHECK(hipStreamWaitEvent(f.s_comm, ev_start[0], 0));

  switch (schedule) {
    case Schedule::Pairs: f.issue_pairs(); break;
    case Schedule::Sidecar: f.issue_sidecar(); break;
    case Schedule::Early: f.issue_early(); break;
    case Schedule::Classic: f.issue_classic(); break;
  }

  DLAF_HIP_CHECK(hipEventRecord(ev_done[0], f.s_main));
  DLAF_HIP_CHECK(hipStreamWaitEvent(f.s_panel, ev_done[0], 0));
  DLAF_HIP_CHECK(hipMemcpyAsync(info_host, info, sizeof(int), hipMemcpyDeviceToHost, f.s_panel));
}

#define INST(T)                                                                                     \
  template void DeviceMatrix<T>::factorize_async();                                                 \
  template int DeviceMatrix<T>::bcast_transposed_panel(Transport*, CommAxis, const T*, long, long, T*, \
                                                       hipStream_t, int&, long&);                   \
  template void potrf_tile<T>(T*, int, int, T*, int*, int, unsigned*, hipStream_t);                  \
  template void potrf_tile_coop<T>(T*, int, int, T*, int*, int, unsigned*, hipStream_t, bool, bool); \
  template void potrf_tile_chain<T>(T*, int, int, T*, int*, int, hipStream_t);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
