// sweep.hpp -- the scaffold shared by the sweeps over a canonical form (solver.cpp: solve_canonical  X T^H = B;
// multiplication.cpp: multiply_canonical  X = B T^H  and hermitian_canonical  Y = beta Y + alpha X H) and by the
// drivers that map side / uplo / op / diag onto them, and by the SUMMA-like walks of general_canonical
// (multiplication.cpp), rank_update.cpp and addition.cpp.  A sweep writes its step logic; from here it takes
//   Sweep              its streams, the timing window and the kernels' status word
//   Events, Ring       one event per step; kBuf device buffers, step s uses s % kBuf
//   wait_ring_free     the ONE statement of the ring-reuse wait: before step s is fetched into buffer s % kBuf, s_comm
//                      waits for the kernels of step s - kBuf
//   StepPipeline       the whole one-step-ahead protocol of a sweep whose step is "fetch on s_comm, then launch on
//                      s_main": the caller gives fetch(s, buf) and apply(s) and touches no event
//   TOperandFetch      the operands taken from the triangular / Hermitian matrix, one step ahead (below)
//   bcast_view_column  tile column k of a view to the other members of the view's row communicator
//   bcast_column_and_transposed_panel   that column, then its whole transposed panel: the row-side and column-side
//                      Panel of a step of the rank-k update and of the transposing addition
//   ScratchStream      (pool.hpp) the scoped stream of a host form: uploads, downloads, tile transforms
//   checked_transport  (transport.hpp) the opening of every entry: runtime, the grid's transport, fatal without one
//   launch_args.hpp    rect_update_args / panel_args over every local row of Bd: the launch arguments of a step
//   operand_map        side / uplo / op / diag -> T and B_dev (the table in solver.cpp's header)
// solve_canonical and multiply_canonical keep loops of their own (a side stream, the update split around the previous
// step's column) and state the ring-reuse wait with wait_ring_free.
#pragma once
#include <algorithm>
#include <vector>

#include "device_matrix.hpp"
#include "launch_args.hpp"
#include "pool.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

// one synchronisation event per step of a sweep
struct Events {
  std::vector<hipEvent_t> v;
  explicit Events(size_t n) : v(n) {
    for (auto& e : v)
      DLAF_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~Events() {
    for (auto e : v)
      (void) hipEventDestroy(e);
  }
  hipEvent_t operator[](size_t i) const { return v[i]; }
};

// kBuf workspaces of one kind: step s uses buffer s % kBuf, so that the operands of step s+1 are fetched while step
// s-1 is still being applied.  wanted = false leaves the ring empty (every entry nullptr).
constexpr int kBuf = 3;
template <class T>
struct Ring {
  DevBuf<T> b[kBuf];
  Ring() = default;
  Ring(size_t elems, bool wanted) {
    for (auto& x : b)
      if (wanted)
        x.alloc(elems);
  }
  T* operator[](int buf) const { return b[buf].p; }
};

// The streams of one sweep -- s_main (lowest priority: the kernels), s_comm (highest: the operands ahead of them) and,
// with_side, s_side (highest: kernels beside s_main) --, the device-time window of the profile hooks, and, with_info,
// the zeroed status word of the update / TRSM kernels.
struct Sweep {
  hipStream_t s_main = nullptr, s_side = nullptr, s_comm = nullptr;
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
  DevBuf<int> info;

  Sweep(bool with_side, bool with_info) {
    int lo = 0, hi = 0;
    DLAF_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_main, hipStreamNonBlocking, lo));
    if (with_side)
      DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_side, hipStreamNonBlocking, hi));
    DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_comm, hipStreamNonBlocking, hi));
    DLAF_HIP_CHECK(hipEventCreate(&ev_t0));
    DLAF_HIP_CHECK(hipEventCreate(&ev_t1));
    if (with_info) {
      info.alloc(1);
      DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s_main));
    }
  }
  Sweep(const Sweep&) = delete;
  Sweep& operator=(const Sweep&) = delete;
  ~Sweep() {
    (void) hipEventDestroy(ev_t0);
    (void) hipEventDestroy(ev_t1);
    (void) hipStreamDestroy(s_main);
    if (s_side)
      (void) hipStreamDestroy(s_side);
    (void) hipStreamDestroy(s_comm);
  }

  // opens the window on s_main; comm_waits: nothing on s_comm starts before that point
  void begin(bool comm_waits) {
    DLAF_HIP_CHECK(hipEventRecord(ev_t0, s_main));
    if (comm_waits)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, ev_t0, 0));
  }
  // closes the window, waits for every stream; the device time between begin() and here in milliseconds
  double finish() {
    DLAF_HIP_CHECK(hipEventRecord(ev_t1, s_main));
    DLAF_HIP_CHECK(hipStreamSynchronize(s_comm));
    if (s_side)
      DLAF_HIP_CHECK(hipStreamSynchronize(s_side));
    DLAF_HIP_CHECK(hipStreamSynchronize(s_main));
    float ms = 0;
    DLAF_HIP_CHECK(hipEventElapsedTime(&ms, ev_t0, ev_t1));
    return ms;
  }
};

// The ring-reuse wait: buffer s % kBuf was last read by the kernels of step s - kBuf, whose end ev_done[s - kBuf] marks
// (recorded before this call is made).  Nothing may be fetched into the buffers of step s before s_comm has waited here.
inline void wait_ring_free(hipStream_t s_comm, const Events& ev_done, long s) {
  if (s >= kBuf)
    DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, ev_done[(size_t) (s - kBuf)], 0));
}

// The one-step-ahead pipeline of a sweep whose step is "operands on s_comm, then kernels on s_main".  fetch(s, buf)
// enqueues the broadcasts of step s on s_comm into ring buffer buf and stores the operand pointers; apply(s) fills the
// arguments and launches on s_main.  ev_in[s]: the operands of step s are in place; ev_done[s]: its kernels are done,
// its buffers are free.  run() opens the sweep's window; the caller closes it (Sweep::finish).  Declare the pipeline
// before the Rings it guards, so that its events outlive them.
struct StepPipeline {
  Events ev_in, ev_done;
  explicit StepPipeline(long nsteps) : ev_in((size_t) nsteps), ev_done((size_t) nsteps) {}

  template <class Fetch, class Apply>
  void run(Sweep& sw, Fetch&& fetch, Apply&& apply) {
    const long nsteps = (long) ev_in.v.size();
    auto fetch_step = [&](long s) {
      wait_ring_free(sw.s_comm, ev_done, s);
      fetch(s, (int) (s % kBuf));
      DLAF_HIP_CHECK(hipEventRecord(ev_in[(size_t) s], sw.s_comm));
    };
    sw.begin(true);
    if (nsteps > 0)
      fetch_step(0);
    for (long s = 0; s < nsteps; ++s) {
      if (s + 1 < nsteps)
        fetch_step(s + 1);
      DLAF_HIP_CHECK(hipStreamWaitEvent(sw.s_main, ev_in[(size_t) s], 0));
      apply(s);
      DLAF_HIP_CHECK(hipEventRecord(ev_done[(size_t) s], sw.s_main));
    }
  }
};

// ---- scalars of the device element types (host side) ------------------------------------------------------
template <class T>
T conj_of(T v) {
  if constexpr (TypeInfo<T>::is_complex)
    v.im = -v.im;
  return v;
}
template <class T>
bool is_value(const T& v, double x) {
  if constexpr (TypeInfo<T>::is_complex)
    return v.re == x && v.im == 0;
  else
    return v == x;
}
template <class T>
bool is_zero(const T& v) {
  return is_value(v, 0);
}
template <class T>
bool is_one(const T& v) {
  return is_value(v, 1);
}

// ---- the T-operand fetch ----------------------------------------------------------------------------------
// Step s of a sweep needs, on every process of Bd's column k = k(s), the diagonal tile T_kk (and, for the solve, its
// inverted 64 x 64 diagonal blocks), and on every process the tiles T(j, k) for its local columns j of Bd "beyond" k
// (j > k for lower T, j < k for upper T).  They depend on A only, so they are issued on the communication stream
// ahead of the sweep.  Two communication shapes: "aligned" (Td's rows are spread like Bd's columns: one broadcast of
// T's column panel) and "crossed" (Td's rows are spread like Bd's rows: the Cholesky's panel + transposed-panel pair).
template <class T>
struct TOperand {
  const T* diag = nullptr;  // T_kk
  const T* winv = nullptr;  // its inverted diagonal blocks (solve only)
  const T* base = nullptr;  // T(j,k) for local column jl of Bd at base + (jl - jl0) * ts
  long ts = 0;
  long jl0 = 0, jl1 = 0;    // local columns of Bd beyond step k
};

// Td's index distribution along the grid dimension it shares with Bd's columns must be the one of Bd's columns
template <class T>
void check_t_aligned(const TileMatrix<T>& Td, const TileMatrix<T>& Bd, const char* who) {
  const bool aligned = Td.row_dim() == Bd.col_dim();
  const Axis& t_match = aligned ? Td.rows : Td.cols;  // Td axis that shares Bd.cols' dimension
  if (t_match.P != Bd.cols.P || t_match.src != Bd.cols.src || t_match.n != Bd.cols.n)
    fatal("[dlaf_mi355x] %s: A and B are not aligned along the triangular dimension (source process %d vs %d)\n", who,
          t_match.src, Bd.cols.src);
}

// Owns its workspaces (a ring each of [T_kk | W_k], of the T column panel as the update's second operand -- one tile
// per local column of Bd --, and of its staging for the crossed shape), the events ev_t[s] it records on s_comm once
// the operands of step s are in place, and the operands top[s] themselves.  fetch(s) fills the buffers s % kBuf: its
// caller states the ring-reuse wait first (wait_ring_free, or the StepPipeline that calls it).
template <class T>
struct TOperandFetch {
  TileMatrix<T>& Td;
  TileMatrix<T>& Bd;
  Transport* tr;
  bool upper;      // T upper triangular: the columns beyond k are j < k
  bool backward;   // step s works on column nt - 1 - s (else s)
  hipStream_t s_comm;
  const T* const* winv_of;  // winv_of[k]: the inverted blocks of the diagonal tile k, where this process owns it
  size_t winv_elems;        // their size (0, winv_of == nullptr: the sweep uses none)
  const bool dist, aligned;
  Ring<T> diag_ws, tpanel, tstage;
  Events ev_t;
  std::vector<TOperand<T>> top;

  TOperandFetch(TileMatrix<T>& Td_, TileMatrix<T>& Bd_, Transport* tr_, bool upper_, bool backward_, hipStream_t s_comm_,
                const T* const* winv_of_ = nullptr, size_t winv_elems_ = 0)
      : Td(Td_), Bd(Bd_), tr(tr_), upper(upper_), backward(backward_), s_comm(s_comm_), winv_of(winv_of_),
        winv_elems(winv_elems_), dist(Bd_.grid->nranks > 1), aligned(Td_.row_dim() == Bd_.col_dim()),
        diag_ws(Bd_.tile_elems + winv_elems_, true), tpanel((size_t) Bd_.ltc * Bd_.tile_elems, dist),
        tstage((size_t) Td_.ltr * Bd_.tile_elems, dist && !aligned), ev_t((size_t) Bd_.cols.nt()),
        top((size_t) Bd_.cols.nt()) {}

  long nt() const { return Bd.cols.nt(); }
  long step_k(long s) const { return backward ? nt() - 1 - s : s; }

  void fetch(long s) {
    const size_t tile_elems = Bd.tile_elems, tile_bytes = tile_elems * sizeof(T);
    const size_t diag_elems = tile_elems + winv_elems;
    const CommAxis along_row = Bd.transposed ? CommAxis::Col : CommAxis::Row;
    const CommAxis along_col = Bd.transposed ? CommAxis::Row : CommAxis::Col;
    const Axis& t_other = aligned ? Td.cols : Td.rows;  // the Td axis that shares Bd.rows' dimension
    const long k = step_k(s);
    const int buf = (int) (s % kBuf);
    TOperand<T>& o = top[(size_t) s];
    // local columns of Bd beyond k
    o.jl0 = upper ? 0 : Bd.cols.next_local(k + 1);
    o.jl1 = upper ? Bd.cols.next_local(k) : Bd.ltc;

    // (1) T_kk (and its inverted diagonal blocks) to every process holding column k of Bd
    const bool own_diag = Td.rows.mine(k) && Td.cols.mine(k);
    const bool need_diag = Bd.cols.mine(k);
    const T* tkk = nullptr;
    const T* wk = nullptr;
    if (own_diag) {
      tkk = Td.tile(Td.rows.local_of(k), Td.cols.local_of(k));
      if (winv_elems > 0)
        wk = winv_of[k];
    }
    if (need_diag && Bd.row_P > 1) {
      // (own_diag implies need_diag: the owner sits in Bd's column k by the alignment requirement)
      if (own_diag) {
        DLAF_HIP_CHECK(hipMemcpyAsync(diag_ws[buf], tkk, tile_bytes, hipMemcpyDeviceToDevice, s_comm));
        if (winv_elems > 0)
          DLAF_HIP_CHECK(hipMemcpyAsync(diag_ws[buf] + tile_elems, wk, winv_elems * sizeof(T), hipMemcpyDeviceToDevice, s_comm));
      }
      tr->bcast(along_col, t_other.owner(k), Bd.row_rank, diag_ws[buf], diag_ws[buf], diag_elems * sizeof(T), s_comm);
      tkk = diag_ws[buf];
      wk = winv_elems > 0 ? diag_ws[buf] + tile_elems : nullptr;
    }
    o.diag = tkk;
    o.winv = wk;

    // (2) T(j,k) for the local columns j of Bd beyond k
    const long ncols = o.jl1 - o.jl0;
    if (!dist) {
      // one process: Td's local row index of global j is Bd's local column index
      o.base = Td.tile(o.jl0 < Td.ltr ? o.jl0 : 0, k);
      o.ts = (long) tile_elems;
    }
    else if (aligned) {
      // Td's rows are spread like Bd's columns: the tiles sit on the process of the same Bd-column
      // coordinate whose Bd-row coordinate owns Td's column k -> one broadcast along Bd's columns
      const bool have = t_other.mine(k);
      T* dst = tpanel[buf];
      if (ncols > 0) {
        const T* src = have ? Td.tile(o.jl0, Td.cols.local_of(k)) : nullptr;
        if (Bd.row_P > 1)
          tr->bcast(along_col, t_other.owner(k), Bd.row_rank, src, dst, (size_t) ncols * tile_bytes, s_comm);
        else
          dst = const_cast<T*>(src);
      }
      o.base = dst;
      o.ts = (long) tile_elems;
    }
    else {
      // crossed: Td's rows are spread like Bd's ROWS.  Column panel k of Td along Bd's rows first, then
      // tile j down Bd's columns from the Bd-row coordinate that owns Td's row j (broadcast_panel.h:125-210)
      const long il0 = upper ? 0 : Td.rows.next_local(k + 1);
      const long il1 = upper ? Td.rows.next_local(k) : Td.ltr;
      const bool have = Td.cols.mine(k);
      const T* colp = nullptr;  // my rows [il0, il1) of Td's column k
      if (il1 > il0) {
        if (Bd.cols.P > 1) {
          const T* src = have ? Td.tile(il0, Td.cols.local_of(k)) : nullptr;
          tr->bcast(along_row, Td.cols.owner(k), Bd.cols.rank, src, tstage[buf], (size_t) (il1 - il0) * tile_bytes, s_comm);
          colp = tstage[buf];
        }
        else {
          colp = Td.tile(il0, Td.cols.local_of(k));
        }
      }
      if (Bd.row_P > 1) {
        tr->group_begin();
        for (long jl = o.jl0; jl < o.jl1; ++jl) {
          const long gj = Bd.cols.global_of(jl);
          const int root = Td.rows.owner(gj);
          const T* src = (Td.rows.rank == root) ? colp + (size_t) (Td.rows.local_of(gj) - il0) * tile_elems : nullptr;
          tr->bcast(along_col, root, Bd.row_rank, src, tpanel[buf] + (size_t) (jl - o.jl0) * tile_elems, tile_bytes, s_comm);
        }
        tr->group_end();
        o.base = tpanel[buf];
        o.ts = (long) tile_elems;
      }
      else {
        // I hold every row of Td's column k: tile gj sits at local row gj
        o.base = colp ? colp + (size_t) (Bd.cols.global_of(o.jl0 < Bd.ltc ? o.jl0 : 0) - il0) * tile_elems : nullptr;
        o.ts = (long) tile_elems * Bd.cols.P;
      }
    }
    DLAF_HIP_CHECK(hipEventRecord(ev_t[(size_t) s], s_comm));
  }
};

// Tile column k of the view V (every local row) to the other members of V's row communicator, on s_comm: in place on
// the process column that owns it, into `elsewhere` on the others.  Returns what a kernel reads as that column.
template <class T>
const T* bcast_view_column(Transport* tr, const TileMatrix<T>& V, long k, T* elsewhere, hipStream_t s_comm) {
  T* p = V.cols.mine(k) ? V.tile(0, V.cols.local_of(k)) : elsewhere;
  if (V.cols.P > 1 && V.ltr > 0)
    tr->bcast(V.transposed ? CommAxis::Col : CommAxis::Row, V.cols.owner(k), V.cols.rank, p, p,
              (size_t) V.ltr * V.tile_elems * sizeof(T), s_comm);
  return p;
}

// The WHOLE transposed panel of a step (DeviceMatrix::bcast_transposed_panel leaves out the last global tile row, which
// the factorization never needs): `have` is the axis the column panel at a_base is spread over -- the tile of global row
// g sits at a_base + have.local_of(g) * tile_elems on the process have.owner(g) of my communicator `ax` --, `want` the
// axis whose EVERY local tile jl needs the panel's tile of global row want.global_of(jl).  One broadcast per root
// process: the local tiles fall into `period` classes by root, class c = tiles c, c + period, ... lands contiguously
// at dst + c * ts2 (the root packs its -- strided -- tiles there first), so tile jl is read at
// dst + (jl % period) * ts2 + (jl / period) * tile_elems.  dst holds (want.local_tiles() + have.P) tiles.  Returns the
// number of broadcasts issued.
template <class T>
int bcast_transposed_panel_whole(Transport* tr, CommAxis ax, const Axis& have, const Axis& want, const T* a_base, T* dst,
                                 size_t tile_elems, hipStream_t s, int& period, long& ts2) {
  const size_t tile_bytes = tile_elems * sizeof(T);
  const long ncols = want.local_tiles();
  long g = have.P, r = want.P;
  while (r) {
    const long t = g % r;
    g = r;
    r = t;
  }
  // owner(global_of(jl)) repeats in jl with period lcm(have.P, want.P) / want.P
  period = (int) (have.P / g);
  const long lstep = want.P / g;  // local-row distance on the root between consecutive tiles of a class
  const long cap = ncols > 0 ? (ncols + period - 1) / period : 0;
  ts2 = cap * (long) tile_elems;
  int issued = 0;
  tr->group_begin();
  for (long c = 0; c < period && c < ncols; ++c) {
    const long gj_first = want.global_of(c);
    const int root = have.owner(gj_first);
    const long cnt = (ncols - c + period - 1) / period;
    T* d = dst + c * ts2;
    if (have.rank == root)
      DLAF_HIP_CHECK(hipMemcpy2DAsync(d, tile_bytes, a_base + (size_t) have.local_of(gj_first) * tile_elems,
                                      (size_t) lstep * tile_bytes, tile_bytes, (size_t) cnt, hipMemcpyDeviceToDevice, s));
    tr->bcast(ax, root, have.rank, d, d, (size_t) cnt * tile_bytes, s);
    ++issued;
  }
  tr->group_end();
  return issued;
}

// A panel of tiles as a kernel reads it: tile j at base + (j % period) * ts2 + (j / period) * ts (period 1: base + j * ts)
template <class T>
struct Panel {
  const T* base = nullptr;
  long ts = 0, ts2 = 0;
  int period = 1;
};
template <class T>
struct PanelPair {
  Panel<T> row, col;
};

// Tile column l of M for both sides of a step, on s_comm: `row`, the column as it is spread over `have` (M's rows) -- the
// tiles of my local tile rows, through bcast_view_column into rbuf --, and `col`, its whole transposed panel -- the tiles
// of every local tile of `want`, down the process columns into cbuf (bcast_transposed_panel_whole).
template <class T>
PanelPair<T> bcast_column_and_transposed_panel(Transport* tr, const TileMatrix<T>& M, long l, const Axis& have,
                                               const Axis& want, T* rbuf, T* cbuf, hipStream_t s_comm) {
  const size_t te = M.tile_elems;
  PanelPair<T> p;
  p.row.base = bcast_view_column(tr, M, l, rbuf, s_comm);
  p.row.ts = (long) te;
  if (have.P > 1) {
    (void) bcast_transposed_panel_whole(tr, CommAxis::Col, have, want, p.row.base, cbuf, te, s_comm, p.col.period,
                                        p.col.ts2);
    p.col.base = cbuf;
    p.col.ts = (long) te;
  }
  else {
    // no hop: I hold every tile row of the panel, the tile of global row gj sits at local row gj
    p.col.base = p.row.base + (size_t) want.shift() * te;
    p.col.ts = (long) te * want.P;
  }
  return p;
}

// ---- drivers ----------------------------------------------------------------------------------------------
inline bool side_is_left(char side) {
  return side == 'L' || side == 'l';
}
inline bool uplo_is_upper(char uplo) {
  return uplo == 'U' || uplo == 'u';
}

// The operand mapping table in solver.cpp's header:
// T = A (Right C / Left N), A^H (Right N / Left C), conj(A) (Right T), A^T (Left T)
struct OperandMap {
  bool left, a_upper, unit;
  bool t_transposed, t_conj, t_upper;  // T = the (conjugated) (transposed) A, and the triangle it fills
};
inline OperandMap operand_map(char side, char uplo, char op, char diag) {
  OperandMap m;
  m.left = side_is_left(side);
  m.a_upper = uplo_is_upper(uplo);
  m.unit = (diag == 'U' || diag == 'u');
  const char o = (op == 'n') ? 'N' : (op == 't') ? 'T' : (op == 'c') ? 'C' : op;
  m.t_transposed = m.left ? (o != 'N') : (o == 'N');
  m.t_conj = m.left ? (o == 'C') : (o == 'N' || o == 'T');
  m.t_upper = m.a_upper != m.t_transposed;
  return m;
}

// The sweeps over a triangular T and the drivers that map side / uplo / op / diag / alpha onto them (solver.cpp).
// sweep(Td, Bd, upper, unit) works in place on Bd.
template <class T>
using CanonicalSweep = void (*)(TileMatrix<T>& Td, TileMatrix<T>& Bd, bool upper, bool unit);
template <class T>
int triangular_canonical_host(CanonicalSweep<T> sweep, bool may_reverse, Grid* g, char side, char uplo, char op, char diag,
                              T alpha, HostOperand<const T> a, HostOperand<T> b);
template <class T>
int triangular_canonical_device(const char* who, CanonicalSweep<T> sweep, char side, char uplo, char op, char diag,
                                T alpha, DeviceMatrix<T>& A, GeneralMatrix<T>& B);

// dst view tile (il, jl) = alpha * op(src tile) for the dltr x dltc tiles of a view (solver.cpp): mode 0 adjoint and
// 3 transpose take src tile (jl, il), 4 conjugate and 5 copy take src tile (il, jl); sltr: local tile rows of src
template <class T>
void xform_tiles(T* dst, long dltr, long dltc, const T* src, long sltr, size_t te, int nb, int mode, T alpha,
                 bool use_alpha, hipStream_t s);

}  // namespace dlaf_mi355x
