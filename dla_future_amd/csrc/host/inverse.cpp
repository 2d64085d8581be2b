// inverse.cpp -- triangular_inverse  A <- A^-1  (LAPACK xTRTRI) and inverse_from_cholesky_factor: the uplo triangle of
// (L L^H)^-1 / (U^H U)^-1 from the Cholesky factor held in it (LAPACK xPOTRI), in place on a DeviceMatrix.  uplo = U
// runs on the transposed view like the Cholesky and gen_to_std: inv(U)^T = inv(U^T), and with L' = U^T, W' = inv(L')
// the view of inv(U) inv(U)^H is W'^H W'.  So only the lower forms exist on the device.
//
// Both are sweeps over the tile rows k = 0 .. nt-1 whose O(n^3) work is one launch of the grouped update kernel per
// step, in its additive form.  ALL the work on diagonal tiles is done ahead of the sweep, batched over the local
// diagonal tiles (kernels_inverse.hip), because no diagonal tile depends on another tile's result:
//   inverse:  W_kk = inv(L_kk) depends on L_kk alone, and nothing but step k reads L_kk;
//   product:  L_kk^H L_kk can be formed before the steps k' > k add their L(k',k)^H L(k',k) to it, once
//             Z_kk = L_kk^H -- which step k multiplies row k by -- has been set aside.
//
// Inverse, step k  (before it: the leading k x k block is inverted, column block j < k of the rows below holds
// -L(:, j) W_jj accumulated over the steps so far):
//   (1) panel   L(i,k) <- L(i,k) (-W_kk)                   i > k     panel TRMM against N_kk = -W_kk^H (upper)
//   (2) update  L(i,j) += L(i,k) L(k,j)                    i > k > j ONE rectangular additive update; second operand =
//                                                                    the adjoint tiles of row k (tile transform)
//   (3) row     L(k,j) <- W_kk L(k,j)                      j < k     panel TRMM on the same adjoint tiles, then back
//   (4) L(k,k) <- W_kk                                               done ahead of the sweep (see above)
// Product  A = W^H W in place of W (lower), step k >= 1:
//   (1) update  A(i,j) += L(k,i)^H L(k,j)                  k > i >= j ONE additive triangle-form update with the adjoint
//                                                                    tiles of row k as BOTH operands (diagonal tiles:
//                                                                    herk, imag(diag) = 0)
//   (2) row     L(k,j) <- L(k,k)^H L(k,j)                  j < k     panel TRMM against Z_kk (upper), then back
//   (3) L(k,k) <- L(k,k)^H L(k,k)                                    done ahead of the sweep
// Communication per step on a process grid (everything on one stream): [W_kk | N_kk] (product: Z_kk) along the owning
// process row and column; the adjoint tiles of row k down the process columns; the column panel along the process rows
// (inverse) / the adjoint tiles once more along the process rows to the processes that hold the matching tile ROWS
// (product: one grouped broadcast per local tile row, the "transposed panel" of the Cholesky).
// Workspaces come from the workspace pool and are sized by panels: (ltr + ltc + 2 (local diagonal tiles + 1)) tiles.
#include <algorithm>
#include <numeric>

#include "drivers.hpp"
#include "launch_args.hpp"
#include "pool.hpp"
#include "sweep.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

double g_profile_ms = 0, g_profile_flops = 0;

}  // namespace

// The local diagonal tiles of a block-cyclic square matrix: global tiles k0, k0 + kstep, ... (kstep = lcm(Pr, Pc)), at
// local (il0 + m il_step, jl0 + m jl_step) -- an arithmetic progression, so that one batched launch with ONE tile
// stride covers them.
DiagTiles local_diag_tiles(const Axis& rows, const Axis& cols) {
  DiagTiles d{};
  const long nt = rows.nt();
  d.kstep = std::lcm((long) rows.P, (long) cols.P);
  d.il_step = d.kstep / rows.P;
  d.jl_step = d.kstep / cols.P;
  d.k0 = -1;
  for (long k = 0; k < std::min(nt, d.kstep); ++k)
    if (rows.mine(k) && cols.mine(k)) {
      d.k0 = k;
      break;
    }
  if (d.k0 < 0)
    return d;
  d.count = (nt - 1 - d.k0) / d.kstep + 1;
  d.il0 = rows.local_of(d.k0);
  d.jl0 = cols.local_of(d.k0);
  const long klast = d.k0 + (d.count - 1) * d.kstep;
  d.last = rows.tile_extent(klast);
  return d;
}

// The local ranges step k of either sweep works on
InverseStep inverse_step_ranges(const Axis& rows, const Axis& cols, long k) {
  InverseStep s{};
  s.own_r = rows.owner(k);
  s.own_c = cols.owner(k);
  s.il_below = rows.next_local(k + 1);
  s.nrl = rows.next_local(k);
  s.ncl = cols.next_local(k);
  s.lr = rows.mine(k) ? rows.local_of(k) : -1;
  s.lc = cols.mine(k) ? cols.local_of(k) : -1;
  return s;
}

long inverse_workspace_tiles(const Axis& rows, const Axis& cols) {
  const DiagTiles d = local_diag_tiles(rows, cols);
  return rows.local_tiles() + cols.local_tiles() + 2 * (d.count + 1);
}

namespace {

template <class T>
struct Inverse {
  DeviceMatrix<T>& A;
  Transport* const tr;
  const bool dist;
  const Axis &rows, &cols;
  const long nt, ltr, ltc;
  const int nb;
  const size_t te;
  const CommAxis ax_row, ax_col;  // uplo == 'U': the view's process rows are the caller's process columns
  int* const info;
  const hipStream_t s;
  const DiagTiles dt;
  PoolScope ws;
  T* const wn;     // per local diagonal tile [W | N] (product: [Z | unused]); one more pair for a received one
  T* const tw;     // adjoint tiles of row k, one per local column left of the diagonal
  T* const panel;  // received column panel (inverse) / the adjoint tiles by local ROW (product)

  Inverse(DeviceMatrix<T>& A_, Transport* tr_)
      : A(A_), tr(tr_), dist(A_.grid->nranks > 1), rows(A_.rows), cols(A_.cols), nt(A_.nt), ltr(A_.ltr), ltc(A_.ltc),
        nb(A_.nb), te(A_.tile_elems), ax_row(A_.transposed ? CommAxis::Col : CommAxis::Row),
        ax_col(A_.transposed ? CommAxis::Row : CommAxis::Col), info(A_.info), s(A_.s_high),
        dt(local_diag_tiles(A_.rows, A_.cols)), wn(ws.get<T>((size_t) 2 * (dt.count + 1) * te)),
        tw(ws.get<T>((size_t) ltc * te)), panel(ws.get<T>((size_t) ltr * te)) {}

  long diag_slot(long k) const { return (k - dt.k0) / dt.kstep; }
  // [first | second] tile of the diagonal tile k: the owner's own slot, elsewhere the slot a broadcast fills
  T* pair_of(long k) const {
    const bool own = rows.mine(k) && cols.mine(k);
    return wn + (size_t) 2 * (own ? diag_slot(k) : dt.count) * te;
  }
  template <class U>
  TileBatch<U> diag_batch() const {
    TileBatch<U> b{};
    b.base = dt.count > 0 ? A.tile(dt.il0, dt.jl0) : nullptr;
    b.stride = (long) ((dt.il_step + dt.jl_step * ltr) * (long) te);
    b.ld = nb;
    b.nb = nb;
    b.count = (int) dt.count;
    b.last = dt.last;
    return b;
  }
  TileBatch<T> pair_batch(int which) const {
    TileBatch<T> b = diag_batch<T>();
    b.base = wn + (size_t) which * te;
    b.stride = 2 * (long) te;
    return b;
  }

  // LAPACK's info of xTRTRI: the first exactly-zero diagonal element, before anything is written (this process's)
  int scan_zero_diagonal() {
    PoolScope scan;
    unsigned* first = scan.get<unsigned>(1);
    DLAF_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned), s));
    launch_diag_zero_scan(diag_batch<const T>(), dt.k0, dt.kstep, first, s);
    unsigned h = 0;
    DLAF_HIP_CHECK(hipMemcpyAsync(&h, first, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    return h == 0xffffffffu ? 0 : (int) h;
  }

  void trmm_tiles(T* b, long ntiles, int rows_each, const T* l, int n, bool upper) {
    if (ntiles <= 0)
      return;
    auto ta = tile_batch_args<TrmmArgs<T>>(b, (long) te, nb, ntiles, rows_each, l, nb, n);
    ta.upper = upper ? 1 : 0;
    launch_trmm(ta, s);
  }
  // row k's tiles left of the diagonal <-> their adjoints in tw
  void stage_row(const InverseStep& st, int kb) {
    launch_tile_xform(tw, (long) nb, (long) te, A.tile(st.lr, 0), (long) nb, (long) (te * ltr), kb, nb, (int) st.ncl, 0,
                      1.0, s);
  }
  void unstage_row(const InverseStep& st, int kb) {
    launch_tile_xform(A.tile(st.lr, 0), (long) nb, (long) (te * ltr), tw, (long) nb, (long) te, nb, kb, (int) st.ncl, 0,
                      1.0, s);
  }
  void end_of_step() {
    if (dist)
      DLAF_HIP_CHECK(hipStreamSynchronize(s));  // single workspaces: reused by the next step
  }

  // ============================================================================ triangular inverse
  // every local diagonal tile at once: W = inv(L_kk) and N = -W^H set aside, L_kk <- W
  void invert_diag_tiles(bool unit) {
    if (dt.count == 0)
      return;
    const size_t wel = A.winv_elems();
    PoolScope blocks;
    T* winv = blocks.get<T>((size_t) dt.count * wel);
    const TileBatch<const T> tiles = diag_batch<const T>();
    for (long m = 0; m < dt.count; ++m)
      launch_invert_diag_blocks(tiles.base + m * tiles.stride, nb, m == dt.count - 1 ? dt.last : nb, winv + m * wel,
                                info, s, false, unit);
    launch_tile_trtri(tiles, winv, (long) wel, wn + te, 2 * (long) te, s);
    // W = -N^H
    launch_tile_xform_alpha(wn, (long) nb, 2 * (long) te, wn + te, (long) nb, 2 * (long) te, nb, nb, (int) dt.count,
                            0, neg_one(), true, s);
    launch_tri_tile(diag_batch<T>(), wn, 2 * (long) te, 0, unit, s);
  }
  static T neg_one() {
    if constexpr (TypeInfo<T>::is_complex)
      return T{-1, 0};
    else
      return T(-1);
  }

  void inverse_step(long k) {
    const InverseStep st = inverse_step_ranges(rows, cols, k);
    const int kb = rows.tile_extent(k);
    const bool in_row = rows.rank == st.own_r, in_col = cols.rank == st.own_c;
    T* W = pair_of(k);
    T* N = W + te;
    if (in_col && rows.P > 1 && k + 1 < nt)
      tr->bcast(ax_col, st.own_r, rows.rank, W, W, 2 * te * sizeof(T), s);
    if (in_row && cols.P > 1 && k > 0)
      tr->bcast(ax_row, st.own_c, cols.rank, W, W, 2 * te * sizeof(T), s);
    // (1) panel
    if (in_col && st.il_below < ltr) {
      auto ta = panel_args<TrmmArgs<T>>(A, st.il_below, ltr, st.lc, N, kb);
      ta.upper = 1;
      launch_trmm(ta, s);
    }
    if (k == 0)
      return end_of_step();
    T* colL = in_col ? A.tile(st.il_below < ltr ? st.il_below : 0, st.lc) : panel;
    if (cols.P > 1 && st.il_below < ltr)
      tr->bcast(ax_row, st.own_c, cols.rank, colL, colL, (size_t) (ltr - st.il_below) * te * sizeof(T), s);
    // (2) update with the adjoint tiles of row k as it is before (3)
    if (in_row && st.ncl > 0)
      stage_row(st, kb);
    if (rows.P > 1 && st.ncl > 0 && k + 1 < nt)
      tr->bcast(ax_col, st.own_r, rows.rank, tw, tw, (size_t) st.ncl * te * sizeof(T), s);
    if (st.il_below < ltr && st.ncl > 0)
      launch_update(rect_update_args(A, st.il_below, ltr, 0, st.ncl, colL, tw, (long) te, kb, info), s, 4);
    // (3) row: (W L(k,j))^H = L(k,j)^H W^H
    if (in_row && st.ncl > 0) {
      trmm_tiles(tw, st.ncl, nb, W, kb, false);
      unstage_row(st, kb);
    }
    end_of_step();
  }

  // ============================================================================ product W^H W
  // every local diagonal tile at once: Z = L_kk^H set aside, L_kk <- Z Z^H
  void multiply_diag_tiles() {
    if (dt.count == 0)
      return;
    launch_tri_tile(pair_batch(0), A.tile(dt.il0, dt.jl0), diag_batch<T>().stride, 1, false, s);
    launch_tile_lauum(diag_batch<T>(), wn, 2 * (long) te, s);
  }

  void product_step(long k) {
    const InverseStep st = inverse_step_ranges(rows, cols, k);
    const int kb = rows.tile_extent(k);
    const bool in_row = rows.rank == st.own_r;
    T* Z = pair_of(k);
    if (in_row && cols.P > 1)
      tr->bcast(ax_row, st.own_c, cols.rank, Z, Z, te * sizeof(T), s);
    if (in_row && st.ncl > 0)
      stage_row(st, kb);
    if (rows.P > 1 && st.ncl > 0)
      tr->bcast(ax_col, st.own_r, rows.rank, tw, tw, (size_t) st.ncl * te * sizeof(T), s);
    // the first operand: the adjoint tile of global column i for every local tile ROW i < k
    const T* a = tw;
    if (dist && st.nrl > 0) {
      a = panel;
      if (cols.P > 1)
        tr->group_begin();
      for (long il = 0; il < st.nrl; ++il) {
        const long gi = rows.global_of(il);
        const int root = cols.owner(gi);
        const T* src = cols.rank == root ? tw + (size_t) cols.local_of(gi) * te : nullptr;
        if (cols.P > 1)
          tr->bcast(ax_row, root, cols.rank, src, panel + (size_t) il * te, te * sizeof(T), s);
        else
          DLAF_HIP_CHECK(hipMemcpyAsync(panel + (size_t) il * te, src, te * sizeof(T), hipMemcpyDeviceToDevice, s));
      }
      if (cols.P > 1)
        tr->group_end();
    }
    // (1) update, triangle form
    if (st.nrl > 0 && st.ncl > 0)
      launch_update(update_args(A, 0, st.nrl, 0, st.ncl, a, (const T*) tw, (long) te, kb, info), s, 4);
    // (2) row: (L_kk^H L(k,j))^H = L(k,j)^H L_kk = L(k,j)^H Z^H
    if (in_row && st.ncl > 0) {
      trmm_tiles(tw, st.ncl, nb, Z, kb, true);
      unstage_row(st, kb);
    }
    end_of_step();
  }
};

template <class T>
Transport* transport_of(DeviceMatrix<T>& A) {
  Transport* tr = checked_transport(*A.grid);
  // work enqueued on the matrix's other streams (a cholesky_start without a wait) must be done before it is read here
  for (hipStream_t ls : {A.s_low, A.s_comm})
    if (ls != nullptr && ls != A.s_high)
      DLAF_HIP_CHECK(hipStreamSynchronize(ls));
  DLAF_HIP_CHECK(hipMemsetAsync(A.info, 0, sizeof(int), A.s_high));
  return tr;
}

// the timed window of inverse_last_profile around `body`, which enqueues on A.s_high
template <class T, class F>
void timed(DeviceMatrix<T>& A, double flops, F&& body) {
  hipEvent_t e0, e1;
  DLAF_HIP_CHECK(hipEventCreate(&e0));
  DLAF_HIP_CHECK(hipEventCreate(&e1));
  DLAF_HIP_CHECK(hipEventRecord(e0, A.s_high));
  body();
  DLAF_HIP_CHECK(hipEventRecord(e1, A.s_high));
  DLAF_HIP_CHECK(hipStreamSynchronize(A.s_high));
  float ms = 0;
  DLAF_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void) hipEventDestroy(e0);
  (void) hipEventDestroy(e1);
  g_profile_ms = ms;
  g_profile_flops = flops;
}

template <class T>
double half_flops(long n) {
  return (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (double) n * (double) n * (double) n / 3.0;
}

bool is_unit(char diag) {
  if (diag == 'U' || diag == 'u')
    return true;
  if (diag != 'N' && diag != 'n')
    fatal("[dlaf_mi355x] triangular inverse: diag must be 'N' or 'U', got '%c'\n", diag);
  return false;
}

// both halves share the scan and the window: product == true runs W^H W after the inverse
template <class T>
int inverse_device(DeviceMatrix<T>& A, bool unit, bool product) {
  Transport* tr = transport_of(A);
  g_profile_ms = 0;
  g_profile_flops = 0;
  if (A.nt == 0)
    return 0;
  Inverse<T> w(A, tr);
  const int h = unit ? 0 : agree_on_info(*A.grid, w.scan_zero_diagonal());
  if (h != 0)
    return h;
  timed(A, (product ? 2.0 : 1.0) * half_flops<T>(A.n), [&] {
    w.invert_diag_tiles(unit);
    for (long k = 0; k < A.nt; ++k) {
      if (tr)
        tr->mark(k);
      w.inverse_step(k);
    }
    if (product) {
      w.multiply_diag_tiles();
      for (long k = 1; k < A.nt; ++k) {
        if (tr)
          tr->mark(A.nt + k);
        w.product_step(k);
      }
    }
  });
  return 0;
}

}  // namespace

template <class T>
int triangular_inverse_device(char diag, DeviceMatrix<T>& A) {
  return inverse_device(A, is_unit(diag), false);
}
template <class T>
int inverse_from_cholesky_factor_device(DeviceMatrix<T>& A) {
  return inverse_device(A, false, true);
}

// Host entries: a = this process's local column-major part; only the uplo triangle is moved back
template <class T>
int triangular_inverse_host(Grid* g, char uplo, char diag, HostOperand<T> a) {
  const bool unit = is_unit(diag);
  DeviceMatrix<T> A;
  A.create(g, uplo, a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  const int r = inverse_device(A, unit, false);
  if (r == 0)
    A.download(a.p, a.ld, true);
  return r;
}
template <class T>
int inverse_from_cholesky_factor_host(Grid* g, char uplo, HostOperand<T> a) {
  DeviceMatrix<T> A;
  A.create(g, uplo, a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  const int r = inverse_device(A, false, true);
  if (r == 0)
    A.download(a.p, a.ld, true);
  return r;
}

void inverse_last_profile(double* ms, double* flops) {
  if (ms)
    *ms = g_profile_ms;
  if (flops)
    *flops = g_profile_flops;
}

#define INST(T)                                                                                   \
  template int triangular_inverse_device<T>(char, DeviceMatrix<T>&);                              \
  template int inverse_from_cholesky_factor_device<T>(DeviceMatrix<T>&);                          \
  template int triangular_inverse_host<T>(Grid*, char, char, HostOperand<T>);                     \
  template int inverse_from_cholesky_factor_host<T>(Grid*, char, HostOperand<T>);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
