// t_operand.hpp -- the T-operand fetch shared by the two sweeps over the canonical form  X T^H = B / X = B T^H
// (solver.cpp: solve_canonical, multiplication.cpp: multiply_canonical).  Step s of a sweep needs, on every
// process of Bd's column k = k(s), the diagonal tile T_kk (and, for the solve, its inverted 64 x 64 diagonal
// blocks), and on every process the tiles T(j, k) for its local columns j of Bd "beyond" k (j > k for lower T,
// j < k for upper T).  They depend on A only, so they are issued on the communication stream ahead of the sweep.
// Two communication shapes: "aligned" (Td's rows are spread like Bd's columns: one broadcast of T's column panel)
// and "crossed" (Td's rows are spread like Bd's rows: the Cholesky's panel + transposed-panel pair).
#pragma once
#include <algorithm>
#include <vector>

#include "runtime.hpp"
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

template <class T>
struct TOperandFetch {
  static constexpr int kBuf = 3;  // step s uses buffer s % kBuf
  TileMatrix<T>& Td;
  TileMatrix<T>& Bd;
  Transport* tr;
  bool upper;      // T upper triangular: the columns beyond k are j < k
  bool backward;   // step s works on column nt - 1 - s (else s)
  hipStream_t s_comm;
  const std::vector<long>& my_diag;  // global indices of the diagonal tiles of Td this process owns
  const T* winv_all;                 // their inverted blocks, winv_elems each (winv_elems == 0: none)
  size_t winv_elems;
  T* const* diag_ws;                 // kBuf x [T_kk | W_k]
  T* const* tpanel;                  // kBuf x (Bd.ltc tiles)       (dist only)
  T* const* tstage;                  // kBuf x (Td.ltr tiles)       (dist, crossed only)
  const hipEvent_t* ev_free;         // ev_free[s]: the kernels of step s are done with its buffers
  const hipEvent_t* ev_t;            // recorded on s_comm once step s's operands are in place
  std::vector<TOperand<T>>& top;

  long nt() const { return Bd.cols.nt(); }
  long step_k(long s) const { return backward ? nt() - 1 - s : s; }
  bool aligned() const { return Td.row_dim() == Bd.col_dim(); }

  void fetch(long s) {
    const bool dist = Bd.grid->nranks > 1;
    const size_t tile_elems = Bd.tile_elems, tile_bytes = tile_elems * sizeof(T);
    const size_t diag_elems = tile_elems + winv_elems;
    const CommAxis along_row = Bd.transposed ? CommAxis::Col : CommAxis::Row;
    const CommAxis along_col = Bd.transposed ? CommAxis::Row : CommAxis::Col;
    const Axis& t_other = aligned() ? Td.cols : Td.rows;  // the Td axis that shares Bd.rows' dimension
    const long k = step_k(s);
    const int buf = (int) (s % kBuf);
    TOperand<T>& o = top[(size_t) s];
    // local columns of Bd beyond k
    o.jl0 = upper ? 0 : Bd.cols.next_local(k + 1);
    o.jl1 = upper ? Bd.cols.next_local(k) : Bd.ltc;
    // these buffers were last read by the kernels of step s - kBuf (event recorded before this call is made)
    if (s >= kBuf)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_comm, ev_free[(size_t) (s - kBuf)], 0));

    // (1) T_kk (and its inverted diagonal blocks) to every process holding column k of Bd
    const bool own_diag = Td.rows.mine(k) && Td.cols.mine(k);
    const bool need_diag = Bd.cols.mine(k);
    const T* tkk = nullptr;
    const T* wk = nullptr;
    if (own_diag) {
      tkk = Td.tile(Td.rows.local_of(k), Td.cols.local_of(k));
      if (winv_elems > 0) {
        const size_t q = (size_t) (std::find(my_diag.begin(), my_diag.end(), k) - my_diag.begin());
        wk = winv_all + q * winv_elems;
      }
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
    else if (aligned()) {
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

// The canonical sweeps and the drivers that map side / uplo / op / diag / alpha onto them (solver.cpp: the operand
// mapping table in its header).  sweep(Td, Bd, upper, unit) works in place on Bd.
template <class T>
using CanonicalSweep = void (*)(TileMatrix<T>& Td, TileMatrix<T>& Bd, bool upper, bool unit);
template <class T>
int triangular_canonical_host(const char* who, CanonicalSweep<T> sweep, bool may_reverse, Grid* g, char side, char uplo,
                              char op, char diag, T alpha, const T* a, long lda, int a_isrc, int a_jsrc, T* b, long ldb,
                              long m, long n, int nb, int b_isrc, int b_jsrc, int nb_free);
template <class T>
int triangular_canonical_device(const char* who, CanonicalSweep<T> sweep, char side, char uplo, char op, char diag,
                                T alpha, DeviceMatrix<T>& A, GeneralMatrix<T>& B);

// dst view tile (il, jl) = alpha * op(src tile) for the dltr x dltc tiles of a view (solver.cpp): mode 0 adjoint and
// 3 transpose take src tile (jl, il), 4 conjugate and 5 copy take src tile (il, jl); sltr: local tile rows of src
template <class T>
void xform_tiles(T* dst, long dltr, long dltc, const T* src, long sltr, size_t te, int nb, int mode, T alpha,
                 bool use_alpha, hipStream_t s);

}  // namespace dlaf_mi355x
