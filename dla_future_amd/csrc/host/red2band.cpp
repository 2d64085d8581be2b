// red2band.cpp -- reduction of a Hermitian matrix to band form, Q^H A Q = B, and the matching
// back-transformation C <- Q C (first stage of the eigensolver of BASELINE
// configuration 5).
//
// Reference: dlaf::eigensolver::internal::reduction_to_band (include/dlaf/eigensolver/reduction_to_band.h:40-122),
// ReductionToBand::call local (eigensolver/reduction_to_band/impl.h:968-1110) and distributed (:1113-1462);
// bt_reduction_to_band (eigensolver/bt_reduction_to_band.h, impl.h:132-370).  Per panel of `band` columns the
// reference: copies the panel to the HOST and computes its Householder reflectors there with a thread team
// (:881-961, :297-361), forms T (t_factor_impl.h), W = V T, X = A W tile by tile with partial sums reduced
// over both communicators (:692-807), W2 = W^H X, X -= 1/2 V W2, broadcasts x / v row- and column-wise and
// updates the trailing matrix with her2k / gemm tile tasks (:810-852).
//
// MI355X design.  The matrix stays in the tile layout of the Cholesky path (lower tiles), everything else is
// organised around REPLICATED, ZERO-EXTENDED PANELS: V, W and X are column-major arrays that cover the global
// rows [e0, n), e0 = the origin of the tile row that holds the first row r0 of the panel, with zeros in
// [e0, r0).  With that
//   * the trailing update A -= X V^H + V X^H is ONE launch of the Cholesky path's two-segment her2k update
//     kernel over whole tiles (the rows / columns in front of r0 subtract exact zeros): no sub-tile views;
//   * X = A W is one launch of tile_panel_kernel over the lower tiles (each tile used straight and
//     conjugate-transposed) + one reduction of the partial layers;
//   * on a process grid every rank holds the whole panels, so the reference's six row / column panel
//     broadcasts and two tile-wise reductions per step collapse into: an all-gather of the panel's tile rows
//     inside the owning process column, one row broadcast of the factored panel (+ taus), one all-reduce of X.
//     T, W, W2 and the X update are recomputed by every rank from the replicated panels (b x b work).  The panel
//     itself is factored redundantly by the ranks of the owning process column from the gathered copy: ONE
//     cooperative kernel (panel_qr_kernel) instead of a per-reflector reduction over the column communicator.
// On one process the trailing update of a panel runs beside the next panel's chain (use_lookahead below).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../device/band_api.hpp"
#include "device_matrix.hpp"
#include "launch_args.hpp"
#include "pool.hpp"
#include "red2band.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {
template <class T>
T scalar(double re) {
  return make_host_el<T>(re);
}

// The thresholds of the blocked panel factorization (kernels_hr.hip).  oracle/red2band.py restates them
// (HR_GATE_RATIO, HR_SKIP_TOL, HR_ORTH_FAIL_SCALE, blocked_panel_path) and tests/test_oracle_red2band.py reads them
// from this file.
constexpr double kHrGateRatio = 1.0e4;       // max / min of diag(L1) beyond which the panel is sent back at once
constexpr double kHrSkipTol = 2.0e-13;       // |Q1^H Q1 - I| up to which the second CholeskyQR pass is skipped
constexpr double kHrOrthFailScale = 2.0e-5;  // see hr_orth_fail_tol

// The failure threshold of hr_orth for an m x b panel.  CholeskyQR2 is proven backward stable with an orthonormal Q for
// cond(P) <= (11 (m b + b (b + 1)) u)^(-1/2), u = 2^-53 (Yamamoto et al., ETNA 44, 2015); the first pass's
// |Q1^H Q1 - I| grows like cond(P)^2 u, which is 1 / (11 (m b + b (b + 1))) at that bound.  The scale below it is
// chosen with the CPU model (oracle/red2band.py: blocked_panel_path over Kahan-like panels, which measure >= 2.5e-4 of
// that value once they are past the bound) so that an accepted panel is inside the bound with margin for the device's
// other rounding.  Never below kHrSkipTol: a panel that one pass leaves orthonormal is accepted whatever m is.
double hr_orth_fail_tol(long m, int b) {
  return std::max(kHrSkipTol, kHrOrthFailScale / (11.0 * ((double) m * b + (double) b * (b + 1))));
}

double g_last_ms = 0, g_last_flops = 0;
long g_last_panels[2] = {0, 0};  // panels of the last reduction factored blocked / sent back to the reflector kernel
}  // namespace

void red2band_last_panels(long* blocked, long* fallback) {
  if (blocked)
    *blocked = g_last_panels[0];
  if (fallback)
    *fallback = g_last_panels[1];
}

void red2band_last_profile(double* ms, double* flops) {
  if (ms)
    *ms = g_last_ms;
  if (flops)
    *flops = g_last_flops;
}

// tune parameter eigensolver_min_band (include/dlaf/tune.h:71-75,128; default 100): set from DLAF_EIGENSOLVER_MIN_BAND /
// --dlaf:eigensolver-min-band by dlaf_initialize (src/init.cpp:220) or by dlaf_mi355x_set_eigensolver_min_band
static int g_eigensolver_min_band = 100;
int eigensolver_min_band() {
  return g_eigensolver_min_band;
}
void set_eigensolver_min_band(int b_min) {
  if (b_min < 2)
    fatal("[dlaf_mi355x] eigensolver_min_band = %d must be >= 2 (get_band_size.h:24)\n", b_min);
  g_eigensolver_min_band = b_min;
}

int get_band_size(int nb) {
  // eigensolver/internal/get_band_size.h:20-31: the smallest divisor of nb that is >= eigensolver_min_band, else nb
  const int min_band = g_eigensolver_min_band;
  for (int div = nb / min_band; div >= 2; --div)
    if (nb % div == 0)
      return nb / div;
  return nb;
}

namespace {
template <class T>
void gemm(int M, int N, int K, const T* a, long lda, char opa, const T* b, long ldb, char opb, T* c, long ldc,
          double alpha, double beta, hipStream_t s, int ksplit = 1, T* partial = nullptr) {
  GemmArgs<T> g;
  g.M = M;
  g.N = N;
  g.K = K;
  g.a = a;
  g.lda = lda;
  g.opa = opa;
  g.b = b;
  g.ldb = ldb;
  g.opb = opb;
  g.c = c;
  g.ldc = ldc;
  g.alpha = scalar<T>(alpha);
  g.beta = scalar<T>(beta);
  g.ksplit = ksplit;
  g.partial = partial;
  launch_gemm(g, s);
}

// B L^-H in place for the rows x b matrix B (ld ldb), in tiles of b rows; L: b x b lower (ld b), winv: its inverted
// diagonal blocks
template <class T>
void trsm_rows(T* B, long ldb, long rows, int b, const T* L, const T* winv, const int* status, hipStream_t s) {
  TrsmArgs<T> ta;
  ta.b = B;
  ta.b_ts = b;
  ta.ldb = (int) ldb;
  ta.il0 = 0;
  ta.il1 = (int) ((rows + b - 1) / b);
  ta.pr = 1;
  ta.ri = 0;
  ta.nb = b;
  ta.nt = ta.il1;
  ta.last_rows = (int) (rows - (long) (ta.il1 - 1) * b);
  ta.l = L;
  ta.ldl = b;
  ta.winv = winv;
  ta.n = b;
  ta.info = status;
  launch_trsm(ta, s);
}

// Lookahead (one process): the trailing update of panel p is issued in two launches -- the tile column that holds panel
// p + 1 on the panel stream, everything else on a second stream -- so that the latency-bound panel chain of p + 1 runs
// beside the bulk of the update of p; X = A W of p + 1 waits for both.  DLAF_MI355X_R2B_LOOKAHEAD=0/1 forces it; default:
// on where the panel is factored blocked (a chain of small kernels that finds room beside the update: 27.9 -> 30.0
// TFlop/s at N = 20480, nb = 512, profiles/r04_red2band_lookahead_ab.txt), off with the reflector-by-reflector kernel
// (measured in round 3: no gain, its 1024-thread workgroups need whole CUs).  The bulk is a plain launch: leaving
// workgroup slots free for the panel chain measured slower at every count tried (same profile).
bool use_lookahead(bool blocked, bool dist, bool two_streams) {
  static const int want = [] {
    const char* e = std::getenv("DLAF_MI355X_R2B_LOOKAHEAD");
    return e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
  }();
  return (want < 0 ? blocked : want != 0) && !dist && two_streams;
}

// One panel of reflectors: columns [c0, c0 + nr) of A (tile column J0, tile-local columns from cc), stored below row r0;
// held transposed in qt as w x me, and in V, W, X zero-extended over the me = n - e0 rows from e0, the origin of r0's
// tile row.  il0: the first local tile row at or below I0; pcol: the process column that owns the panel.
struct Panel {
  long k, r0, c0, I0, e0, J0, me, il0;
  int cc, w, nr, pcol;
  bool in_pcol;
};

// The panel steps that the reduction and the back-transformation share, on the matrix A that holds the reflectors; every
// step is enqueued on the panel stream s.  The workspaces are allocated by the caller.
template <class T>
struct PanelSteps {
  DeviceMatrix<T>& A;
  Transport* const tr;
  const bool dist;
  const hipStream_t s;
  const long ldp;  // leading dimension of V, W, X: n rounded up to 16
  T *qt = nullptr, *S = nullptr, *Tm = nullptr, *W = nullptr, *taus = nullptr, *gpart = nullptr;
  int ksplit_max = 1;  // most K slices of the panel-width Gram products (K <= n); gpart holds their partial sums

  PanelSteps(DeviceMatrix<T>& a, Transport* t)
      : A(a), tr(t), dist(a.grid->nranks > 1), s(a.s_high), ldp(((a.n + 15) / 16) * 16) {}

  Panel make_panel(long k, long r0, long c0, int w, int nr) const {
    const long I0 = r0 / A.nb, e0 = I0 * A.nb, J0 = c0 / A.nb;
    const int pcol = A.cols.owner(J0);
    return {k, r0, c0, I0, e0, J0, A.n - e0, A.rows.next_local(I0), (int) (c0 % A.nb), w, nr, pcol, A.cols.rank == pcol};
  }

  // the panel's columns of A (rows >= r0 of this rank's tiles) into qt, or back
  void move_panel(const Panel& P, bool to_qt) const {
    launch_panel_move(A.tiles, A.ltr, A.nb, (int) P.il0, (int) A.ltr, (int) A.cols.local_of(P.J0), A.rows.P,
                      A.rows.shift(), (int) A.nt, A.rows.last_extent(), P.cc, P.w, qt, P.e0, P.r0, to_qt, s);
  }

  // ranks of the owning process column: the panel, transposed, gathered from all process rows
  void gather_panel(const Panel& P) const {
    move_panel(P, true);
    if (A.rows.P > 1) {
      tr->group_begin();
      for (long I = P.I0; I < A.nt; ++I) {
        T* q = qt + (size_t) (I * A.nb - P.e0) * P.w;
        tr->bcast(CommAxis::Col, A.rows.owner(I), A.rows.rank, q, q, (size_t) A.rows.tile_extent(I) * P.w * sizeof(T), s);
      }
      tr->group_end();
    }
  }

  // the factored panel from the owning process column to the others; with_taus: its taus too (the reduction's, which
  // only that column has computed)
  void bcast_panel(const Panel& P, bool with_taus) const {
    if (A.cols.P == 1)
      return;
    tr->bcast(CommAxis::Row, P.pcol, A.cols.rank, qt, qt, (size_t) P.me * P.w * sizeof(T), s);
    if (with_taus)
      tr->bcast(CommAxis::Row, P.pcol, A.cols.rank, taus + P.c0, taus + P.c0, (size_t) P.nr * sizeof(T), s);
  }

  // well-formed V from qt; unless t_given, S = V^H V and the T factor in Tm (S and Tm: ld lds; zero_t: Tm is zeroed
  // first, for a product that reads T past the panel's nr reflectors); then W = V op_t(T).  Every rank, from the
  // replicated panel.
  void form_vtw(const Panel& P, T* V, int lds, bool t_given, bool zero_t, char op_t) const {
    launch_make_v(qt, P.w, P.nr, P.e0, P.r0, A.n, V, ldp, s);
    if (!t_given) {
      gemm(P.w, P.w, (int) P.me, V, ldp, 'C', V, ldp, 'N', S, lds, 1.0, 0.0, s,
           std::min(ksplit_max, gemm_pick_ksplit<T>(P.w, P.w, P.me)), gpart);
      if (zero_t)
        DLAF_HIP_CHECK(hipMemsetAsync(Tm, 0, (size_t) lds * lds * sizeof(T), s));
      launch_tfactor(S, (long) lds, taus + P.c0, P.nr, Tm, (long) lds, s);
    }
    gemm((int) P.me, P.w, P.w, V, ldp, 'N', Tm, lds, op_t, W, ldp, 1.0, 0.0, s);
  }
};

// The issue side of one reduction_to_band: the workspaces, events and streams, and one member per step of a panel.
template <class T>
struct Red2BandIssue : PanelSteps<T> {
  using Base = PanelSteps<T>;
  using Base::A, Base::tr, Base::dist, Base::s, Base::ldp, Base::qt, Base::S, Base::Tm, Base::W, Base::taus,
      Base::gpart, Base::ksplit_max;
  const int b;
  const long nrefls;
  // the blocked panel factorization may take panels of this matrix: its workspaces exist
  const bool blocked;
  const bool lookahead;
  const hipStream_t s2;  // the bulk of the trailing update (the panel stream s without lookahead)
  // V and X alternate between two buffers: the bulk of the trailing update of panel p reads them on the second
  // stream while the panel chain of p + 1 is already writing the next ones
  T *Vb[2] = {}, *Xb[2] = {}, *W2 = nullptr;
  long cap_s = 2, cap_t = 2;
  T *part_s = nullptr, *part_t = nullptr;
  void* qr_scratch = nullptr;
  // blocked panel factorization (kernels_hr.hip): the panel column-major, two Gram / Cholesky factors, U^T, V1, the
  // inverted diagonal blocks of the three triangular solves, the flag that sends a panel to the reflector-by-reflector
  // kernel, the cooperative POTRF's flags
  T *Pcm = nullptr, *hr_g = nullptr, *hr_l2 = nullptr, *hr_r = nullptr, *hr_lu = nullptr, *hr_y1 = nullptr,
    *hr_winv = nullptr;
  const size_t hr_wblk;
  int* hr_flag = nullptr;
  unsigned* hr_sync = nullptr;
  int* hr_flag_host = nullptr;
  long panels_blocked = 0, panels_fallback = 0;
  hipEvent_t ev0, ev1, ev_x[2], ev_rest[2];
  PoolScope ws;

  Red2BandIssue(DeviceMatrix<T>& a, Transport* t, int band, long nr)
      : Base(a, t), b(band), nrefls(nr),
        blocked(panel_qr_blocked_supported(b, std::max<long>(a.n - b, 0), b, sizeof(T), TypeInfo<T>::is_complex)),
        lookahead(use_lookahead(blocked, this->dist, a.s_low != a.s_high)), s2(lookahead ? a.s_low : a.s_high),
        hr_wblk((size_t) ((b + kDiagBlock - 1) / kDiagBlock) * kDiagBlock * kDiagBlock) {
    // (the pool hands out blocks of equal size in the order they were released: this order is kept on purpose)
    const long n = A.n, ltr = A.ltr, ltc = A.ltc;
    const int nb = A.nb;
    qt = ws.get<T>((size_t) b * (size_t) n);
    Vb[0] = ws.get<T>((size_t) ldp * b);
    Vb[1] = ws.get<T>((size_t) ldp * b);
    W = ws.get<T>((size_t) ldp * b);
    Xb[0] = ws.get<T>((size_t) ldp * b);
    Xb[1] = ws.get<T>((size_t) ldp * b);
    S = ws.get<T>((size_t) b * b);
    Tm = ws.get<T>((size_t) b * b);
    W2 = ws.get<T>((size_t) b * b);
    taus = ws.get<T>((size_t) nrefls + 1);
    for (int q = 0; q < 2; ++q) {
      DLAF_HIP_CHECK(hipMemsetAsync(Vb[q], 0, (size_t) ldp * b * sizeof(T), s));
      DLAF_HIP_CHECK(hipMemsetAsync(Xb[q], 0, (size_t) ldp * b * sizeof(T), s));
    }
    DLAF_HIP_CHECK(hipMemsetAsync(W, 0, (size_t) ldp * b * sizeof(T), s));
    DLAF_HIP_CHECK(hipMemsetAsync(taus, 0, ((size_t) nrefls + 1) * sizeof(T), s));
    ksplit_max = std::max(1, gemm_pick_ksplit<T>(b, b, n));
    gpart = ws.get<T>(gemm_partial_elems<T>(b, b, ksplit_max));
    // partial layers of the xHEMM: (layers + 1) * out tiles at its maximum over the panels (trailing matrices of
    // ot x ot local tiles: the local tile counts shrink together)
    for (long k = 0; k <= std::max(ltr, ltc); ++k) {
      const long otr = std::max<long>(ltr - k, 0), otc = std::max<long>(ltc - k, 0);
      if (otr == 0 || otc == 0)
        break;
      const int cs = tile_panel_pick_chunk(otr, nb, b, otc, true, sizeof(T));
      const int ct = tile_panel_pick_chunk(otc, nb, b, otr, true, sizeof(T));
      cap_s = std::max<long>(cap_s, (long) (tile_panel_layers(otc, cs) + 1) * otr);
      cap_t = std::max<long>(cap_t, (long) (tile_panel_layers(otr, ct) + 1) * otc);
      // (rows and columns of a process grid need not shrink in step: one more tile either way)
      cap_s = std::max<long>(cap_s, (long) (tile_panel_layers(otc + 1, cs) + 1) * (otr + 1));
      cap_t = std::max<long>(cap_t, (long) (tile_panel_layers(otr + 1, ct) + 1) * (otc + 1));
    }
    part_s = ws.get<T>((size_t) cap_s * nb * (size_t) b);
    part_t = ws.get<T>((size_t) cap_t * nb * (size_t) b);
    DLAF_HIP_CHECK(hipMalloc(&qr_scratch, panel_qr_scratch_bytes(b, sizeof(T))));
    if (blocked) {
      Pcm = ws.get<T>((size_t) ldp * b);
      hr_g = ws.get<T>((size_t) b * b);
      hr_l2 = ws.get<T>((size_t) b * b);
      hr_r = ws.get<T>((size_t) b * b);
      hr_lu = ws.get<T>((size_t) b * b);
      hr_y1 = ws.get<T>((size_t) b * b);
      hr_winv = ws.get<T>(4 * hr_wblk);
      // [0] failure, [1] second pass skipped, [2] status of the second Cholesky factorization
      DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&hr_flag), 3 * sizeof(int)));
      DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&hr_sync), sizeof(unsigned) * potrf_coop_sync_words(b)));
    }
    DLAF_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&hr_flag_host), sizeof(int), hipHostMallocDefault));
    DLAF_HIP_CHECK(hipEventCreate(&ev0));
    DLAF_HIP_CHECK(hipEventCreate(&ev1));
    DLAF_HIP_CHECK(hipEventRecord(ev0, s));
    for (int q = 0; q < 2; ++q) {
      DLAF_HIP_CHECK(hipEventCreateWithFlags(&ev_x[q], hipEventDisableTiming));
      DLAF_HIP_CHECK(hipEventCreateWithFlags(&ev_rest[q], hipEventDisableTiming));
    }
    if (lookahead) {
      DLAF_HIP_CHECK(hipEventRecord(ev_x[0], s));
      DLAF_HIP_CHECK(hipStreamWaitEvent(s2, ev_x[0], 0));  // the workspaces are ready
    }
  }

  // the events and the workspaces, in the order of their creation
  void release() {
    DLAF_HIP_CHECK(hipEventDestroy(ev0));
    DLAF_HIP_CHECK(hipEventDestroy(ev1));
    for (int q = 0; q < 2; ++q) {
      DLAF_HIP_CHECK(hipEventDestroy(ev_x[q]));
      DLAF_HIP_CHECK(hipEventDestroy(ev_rest[q]));
    }
    ws.release();
    DLAF_HIP_CHECK(hipFree(qr_scratch));
    if (blocked) {
      DLAF_HIP_CHECK(hipFree(hr_flag));
      DLAF_HIP_CHECK(hipFree(hr_sync));
    }
    DLAF_HIP_CHECK(hipHostFree(hr_flag_host));
  }

  Panel panel(long p) const {
    return this->make_panel(p, (p + 1) * b, p * b, b, (int) std::min<long>(b, nrefls - p * b));
  }
  T* V(const Panel& P) const { return Vb[P.k & 1]; }
  T* X(const Panel& P) const { return Xb[P.k & 1]; }

  // CholeskyQR2 on the column-major copy of the panel, then the Householder reconstruction (kernels_hr.hip): the
  // reflectors in qt, their taus, and T in Tm.  Every kernel behind the first factorization looks at hr_flag and does
  // nothing once it is raised; returns whether the panel was accepted (hr_flag still zero).
  bool factor_panel_blocked(const Panel& P) {
    const long m = A.n - P.r0;
    T* qtp = qt + (size_t) (P.r0 - P.e0) * b;
    const int ks = std::min(ksplit_max, gemm_pick_ksplit<T>(b, b, m));
    DLAF_HIP_CHECK(hipMemsetAsync(hr_flag, 0, 3 * sizeof(int), s));
    launch_hr_transpose(qtp, b, m, Pcm, ldp, true, nullptr, s);
    gemm(b, b, (int) m, Pcm, ldp, 'C', Pcm, ldp, 'N', hr_g, b, 1.0, 0.0, s, ks, gpart);
    launch_potrf_coop(hr_g, b, b, hr_winv, hr_flag, 0, hr_sync, s, false, false);
    // max / min of the factor's diagonal is only a LOWER bound of cond(P): a cheap first exit for panels that are
    // plainly ill conditioned; the bound that keeps the path inside CholeskyQR2's proven range is hr_orth's below
    launch_hr_gate(hr_g, b, b, kHrGateRatio, hr_flag, nullptr, nullptr, s);
    trsm_rows(Pcm, ldp, m, b, hr_g, hr_winv, hr_flag, s);
    gemm(b, b, (int) m, Pcm, ldp, 'C', Pcm, ldp, 'N', hr_l2, b, 1.0, 0.0, s, ks, gpart);
    // second pass -- unless the first one left Q orthonormal already (|Q1^T Q1 - I| <= kHrSkipTol: hr_flag[1] is
    // raised, hr_l2 becomes the identity, and the three launches below return at once: 19 ms of the 380 at
    // N = 20480).  A measure above hr_orth_fail_tol(m, b) sends the panel to the reflector-by-reflector kernel.
    // The second factorization has a status word of its own, hr_flag[2] (hr_orth sets it as well when it skips):
    // the second gate folds a failure of it into hr_flag[0], which everything downstream looks at.
    launch_hr_orth(hr_l2, b, b, kHrSkipTol, hr_orth_fail_tol(m, b), hr_flag + 1, hr_flag + 2, hr_flag, s);
    launch_potrf_coop(hr_l2, b, b, hr_winv + hr_wblk, hr_flag + 2, 0, hr_sync, s, false, false);
    launch_hr_gate(hr_l2, b, b, 0.0, hr_flag, hr_flag + 1, hr_flag + 2, s);  // (no ratio gate)
    trsm_rows(Pcm, ldp, m, b, hr_l2, hr_winv + hr_wblk, hr_flag + 1, s);
    gemm(b, b, b, hr_l2, b, 'C', hr_g, b, 'C', hr_r, b, 1.0, 0.0, s);  // R = L2^T L1^T
    // reconstruction: top block, V2 = Q2 U^-1, T = -U S V1^-T
    launch_hr_lu(Pcm, ldp, b, hr_r, hr_lu, hr_y1, Tm, taus + P.c0, hr_flag, s);
    launch_invert_diag_blocks(hr_lu, b, b, hr_winv + 2 * hr_wblk, hr_flag, s, false, false);
    trsm_rows(Pcm + b, ldp, m - b, b, hr_lu, hr_winv + 2 * hr_wblk, hr_flag, s);
    launch_invert_diag_blocks(hr_y1, b, b, hr_winv + 3 * hr_wblk, hr_flag, s, false, true);
    trsm_rows(Tm, b, b, b, hr_y1, hr_winv + 3 * hr_wblk, hr_flag, s);
    launch_hr_transpose(qtp, b, m, Pcm, ldp, false, hr_flag, s);
    DLAF_HIP_CHECK(hipMemcpyAsync(hr_flag_host, hr_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    return *hr_flag_host == 0;
  }

  // 2. the reflectors of the gathered panel (xGEQR2 without the size-1 reflector), on the ranks of the owning process
  // column: blocked where the panel qualifies and passes its checks, else the reflector-by-reflector kernel.  The one
  // place where a panel's path is chosen; returns whether T is in Tm already.
  bool factor_panel(const Panel& P) {
    bool t_ready = false;
    if constexpr (!std::is_same_v<T, cfloat>) {  // (the small kernels are instantiated for float, double, cdouble)
      if (blocked && panel_qr_blocked_supported(b, A.n - P.r0, P.nr, sizeof(T), TypeInfo<T>::is_complex)) {
        t_ready = factor_panel_blocked(P);
        ++(t_ready ? panels_blocked : panels_fallback);
      }
    }
    if (!t_ready)
      launch_panel_qr(qt + (size_t) (P.r0 - P.e0) * b, A.n - P.r0, b, P.nr, taus + P.c0, qr_scratch, A.info, s);
    return t_ready;
  }

  // 4. X = A_t W (xHEMM on the lower tiles), summed over the grid
  void hemm_x(const Panel& P) {
    const Axis &rows = A.rows, &cols = A.cols;
    const long ltr = A.ltr, ltc = A.ltc, il0 = P.il0, jl0 = cols.next_local(P.I0);
    const int nb = A.nb;
    TilePanelArgs<T> h;
    h.tiles = A.tiles;
    h.ltr = ltr;
    h.nb = nb;
    h.il0 = (int) il0;
    h.il1 = (int) ltr;
    h.jl0 = (int) jl0;
    h.jl1 = (int) ltc;
    h.pr = rows.P;
    h.ri = rows.shift();
    h.pc = cols.P;
    h.ci = cols.shift();
    h.nt_r = (int) A.nt;
    h.last_rows = rows.last_extent();
    h.nt_c = (int) A.nt;
    h.last_cols = cols.last_extent();
    h.herm = 1;
    h.w = W;
    h.ldw = ldp;
    h.e0 = P.e0;
    h.ncols = b;
    // (a rank without local trailing rows or columns has no work items at all: nothing to sum either)
    h.kinds = (il0 < ltr && jl0 < ltc) ? 3 : 0;
    h.chunk_s = tile_panel_pick_chunk(ltr - il0, nb, b, std::max<long>(ltc - jl0, 1), true, sizeof(T));
    h.chunk_t = tile_panel_pick_chunk(ltc - jl0, nb, b, std::max<long>(ltr - il0, 1), true, sizeof(T));
    h.layers_s = tile_panel_layers(std::max<long>(ltc - jl0, 1), h.chunk_s);
    h.layers_t = tile_panel_layers(std::max<long>(ltr - il0, 1), h.chunk_t);
    if ((size_t) (h.layers_s + 1) * (size_t) (ltr - il0) > (size_t) cap_s || (size_t) (h.layers_t + 1) * (size_t) (ltc - jl0) > (size_t) cap_t)
      fatal("[dlaf_mi355x] reduction_to_band: partial-layer workspace too small (%d x %ld, %d x %ld; caps %ld, %ld)\n",
            h.layers_s + 1, ltr - il0, h.layers_t + 1, ltc - jl0, cap_s, cap_t);
    h.part_s = part_s;
    h.part_t = part_t;
    if (lookahead && P.k > 0)
      DLAF_HIP_CHECK(hipStreamWaitEvent(s, ev_rest[(P.k - 1) & 1], 0));  // the bulk of the previous trailing update
    launch_tile_panel(h, s);
    launch_hemm_reduce(h, P.r0, X(P), ldp, s);
    if (dist)
      tr->allreduce_sum(X(P), (size_t) ldp * b, TypeInfo<T>::tag, 'A', s);
  }

  // 5. W2 = W^H X,  X -= 1/2 V W2
  void correct_x(const Panel& P) {
    gemm(b, b, (int) P.me, W, ldp, 'C', X(P), ldp, 'N', W2, b, 1.0, 0.0, s,
         std::min(ksplit_max, gemm_pick_ksplit<T>(b, b, P.me)), gpart);
    gemm((int) P.me, b, b, V(P), ldp, 'N', W2, b, 'N', X(P), ldp, -0.5, 1.0, s);
  }

  // A_t -= X V^H + V X^H on the local tile columns [ja, jb) (tile::her2k / 2 x tile::gemm, impl.h:545-585)
  void her2k(const Panel& P, long ja, long jb, hipStream_t st) {
    const Axis &rows = A.rows, &cols = A.cols;
    if (P.il0 >= A.ltr || ja >= jb)
      return;
    const int nb = A.nb;
    // the operands are row ranges of the column-major panels X and V (ld ldp), not tiles
    UpdateArgs<T> ua = update_args(A, P.il0, A.ltr, ja, jb, X(P) + (rows.global_of(P.il0) * nb - P.e0),
                                   V(P) + (cols.global_of(ja) * nb - P.e0), (long) cols.P * nb, 2 * b, A.info);
    ua.a2 = V(P) + (rows.global_of(P.il0) * nb - P.e0);
    ua.b2 = X(P) + (cols.global_of(ja) * nb - P.e0);
    ua.a_ts = (long) rows.P * nb;
    ua.lda = ua.ldb = (int) ldp;
    ua.K1 = b;
    ua.her2k = 1;
    launch_update(ua, st, 3);
  }

  // 6. the trailing update; with lookahead the tile column of the next panel first, on the panel stream, and the rest
  // beside the next panel chain
  void trailing_update(const Panel& P) {
    const long jl0 = A.cols.next_local(P.I0);
    if (!lookahead) {
      her2k(P, jl0, A.ltc, s);
      return;
    }
    const long jsplit = std::min<long>(A.ltc, jl0 + 1);
    DLAF_HIP_CHECK(hipEventRecord(ev_x[P.k & 1], s));
    her2k(P, jl0, jsplit, s);
    DLAF_HIP_CHECK(hipStreamWaitEvent(s2, ev_x[P.k & 1], 0));
    her2k(P, jsplit, A.ltc, s2);
    DLAF_HIP_CHECK(hipEventRecord(ev_rest[P.k & 1], s2));
  }
};
}  // namespace

template <class T>
int reduction_to_band_device(DeviceMatrix<T>& A, int band, T* taus_host) {
  if (A.transposed)
    fatal("[dlaf_mi355x] reduction_to_band: the matrix must be held as uplo = L (the reference references the lower "
          "triangle only, reduction_to_band.h:66-68)\n");
  if (band < 2 || A.nb % band != 0)
    fatal("[dlaf_mi355x] reduction_to_band: band_size %d must be >= 2 and divide the block size %d\n", band, A.nb);
  Transport* tr = checked_transport(*A.grid);
  const long n = A.n;
  hipStream_t s = A.s_high;
  DLAF_HIP_CHECK(hipMemsetAsync(A.info, 0, sizeof(int), s));
  const long nrefls = std::max<long>(0, n - band - 1);
  if (nrefls == 0) {
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  }

  Red2BandIssue<T> r(A, tr, band, nrefls);
  const long npanels = (nrefls - 1) / band + 1;
  for (long p = 0; p < npanels; ++p) {
    if (tr)
      tr->mark(p);
    const Panel P = r.panel(p);
    bool t_ready = false;  // the blocked factorization left the T factor in Tm
    if (P.in_pcol) {
      r.gather_panel(P);
      t_ready = r.factor_panel(P);
      r.move_panel(P, false);
    }
    r.bcast_panel(P, true);
    // 3. (the blocked factorization delivers T = -U S V1^-T with the reflectors; on a grid with several process columns
    // the ranks outside the panel's column have only the reflectors, and every rank forms T the same way)
    r.form_vtw(P, r.V(P), band, t_ready && A.cols.P == 1, true, 'N');
    r.hemm_x(P);
    r.correct_x(P);
    r.trailing_update(P);
    if (r.dist)
      DLAF_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (r.lookahead) {
    DLAF_HIP_CHECK(hipEventRecord(r.ev_rest[0], r.s2));
    DLAF_HIP_CHECK(hipStreamWaitEvent(s, r.ev_rest[0], 0));
  }
  DLAF_HIP_CHECK(hipEventRecord(r.ev1, s));
  int h_info = 0;
  DLAF_HIP_CHECK(hipMemcpyAsync(&h_info, A.info, sizeof(int), hipMemcpyDeviceToHost, s));
  if (taus_host)
    DLAF_HIP_CHECK(hipMemcpyAsync(taus_host, r.taus, (size_t) nrefls * sizeof(T), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  float ms = 0;
  DLAF_HIP_CHECK(hipEventElapsedTime(&ms, r.ev0, r.ev1));
  g_last_ms = ms;
  // miniapp_reduction_to_band.cpp:163-168: add_mul = 2/3 n^3 - n^2 nb, one add + one mul each (x4 complex)
  g_last_flops = (TypeInfo<T>::is_complex ? 4.0 : 1.0) * 2.0 * (2.0 / 3.0 * (double) n * n * n - (double) n * n * A.nb);
  r.release();
  g_last_panels[0] = r.panels_blocked;
  g_last_panels[1] = r.panels_fallback;
  if (h_info == kInfoSchedulingFailure)
    fatal("[dlaf_mi355x] reduction_to_band: the cooperative panel kernel could not make progress (its workgroups were "
          "not co-resident)\n");
  return h_info;
}

// Host entry: a = the Hermitian matrix (lower triangle referenced), overwritten with the band + reflectors; taus:
// n - band - 1 values, all of them on every rank
template <class T>
int reduction_to_band_host(Grid* g, HostOperand<T> a, int band, T* taus) {
  DeviceMatrix<T> A;
  A.create(g, 'L', a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  const int r = reduction_to_band_device(A, band, taus);
  A.download(a.p, a.ld, true);
  return r;
}


// ------------------------------------------------------------------------------------------------ back-transformation
// C <- Q C with Q = H_0 H_1 ... (the reflectors reduction_to_band left below the band of A), applied in blocks of nb
// reflectors, last block first (bt_reduction_to_band/impl.h:132-236 local, :239-370 distributed):
//     W = V T^H,   W2 = W^H C,   C -= V W2.
// C: n x k general matrix in tile layout with A's block size and row distribution.  Same replicated, zero-extended
// panels as above; W2 = W^H C runs as the adjoint kind of tile_panel_kernel over the tiles of C (its result W2^H is
// summed over the process column), C -= V W2 as one rectangular launch of the Cholesky update kernel.
template <class T>
int bt_reduction_to_band_device(int band, TileMatrix<T>& C, DeviceMatrix<T>& A, const T* taus_host) {
  if (A.transposed)
    fatal("[dlaf_mi355x] bt_reduction_to_band: the reflectors must be held as uplo = L\n");
  if (C.grid != A.grid || C.nb != A.nb || C.rows.n != A.n || C.rows.src != A.rows.src || C.transposed)
    fatal("[dlaf_mi355x] bt_reduction_to_band: C must have A's block size, row count and row source rank\n");
  Transport* tr = checked_transport(*A.grid);
  const Axis& rows = A.rows;
  const Axis& ccols = C.cols;
  const long n = A.n, nt = A.nt;
  const int nb = A.nb, b = band;
  hipStream_t s = A.s_high;
  int* info = A.info;
  DLAF_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s));
  const long total = n - b - 1;
  const long cltc = C.ltc, cltr = C.ltr;
  if (total <= 0 || ccols.n == 0) {
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  }
  const long nblocks = (total - 1) / nb + 1;
  PanelSteps<T> ps(A, tr);
  const long ldp = ps.ldp;
  const long ldw2 = std::max<long>(cltc * nb, 1);

  PoolScope ws;
  ps.qt = ws.get<T>((size_t) nb * (size_t) n);
  T* V = ws.get<T>((size_t) ldp * nb);
  ps.W = ws.get<T>((size_t) ldp * nb);
  ps.S = ws.get<T>((size_t) nb * nb);
  ps.Tm = ws.get<T>((size_t) nb * nb);
  T* W2H = ws.get<T>((size_t) ldw2 * nb);
  ps.taus = ws.get<T>((size_t) total + 1);
  DLAF_HIP_CHECK(hipMemcpyAsync(ps.taus, taus_host, (size_t) total * sizeof(T), hipMemcpyHostToDevice, s));
  DLAF_HIP_CHECK(hipMemsetAsync(V, 0, (size_t) ldp * nb * sizeof(T), s));
  DLAF_HIP_CHECK(hipMemsetAsync(ps.W, 0, (size_t) ldp * nb * sizeof(T), s));
  ps.ksplit_max = std::max(1, gemm_pick_ksplit<T>(nb, nb, n));
  ps.gpart = ws.get<T>(gemm_partial_elems<T>(nb, nb, ps.ksplit_max));
  long lay_cap = 2;
  for (long src = 1; src <= std::max<long>(cltr, 1); ++src) {
    const int ch = tile_panel_pick_chunk(std::max<long>(cltc, 1), nb, nb, src, false, sizeof(T));
    lay_cap = std::max<long>(lay_cap, (long) (tile_panel_layers(src, ch) + 1) * std::max<long>(cltc, 1));
  }
  T* part_t = ws.get<T>((size_t) lay_cap * nb * (size_t) nb);

  hipEvent_t ev0, ev1;
  DLAF_HIP_CHECK(hipEventCreate(&ev0));
  DLAF_HIP_CHECK(hipEventCreate(&ev1));
  DLAF_HIP_CHECK(hipEventRecord(ev0, s));

  for (long k = nblocks - 1; k >= 0; --k) {
    if (tr)
      tr->mark(k);
    const int nrefl = (int) std::min<long>(nb, total - k * nb);
    const Panel P = ps.make_panel(k, k * nb + b, k * nb, nrefl, nrefl);
    const long il0 = P.il0, e0 = P.e0;
    if (P.in_pcol)
      ps.gather_panel(P);
    ps.bcast_panel(P, false);
    ps.form_vtw(P, V, nb, false, false, 'C');  // W = V T^H
    if (cltc > 0) {
      // W2^H = C^H W over the local tiles of C with global tile row >= I0
      TilePanelArgs<T> h;
      h.tiles = C.tiles;
      h.ltr = cltr;
      h.nb = nb;
      h.il0 = (int) il0;
      h.il1 = (int) cltr;
      h.jl0 = 0;
      h.jl1 = (int) cltc;
      h.pr = rows.P;
      h.ri = rows.shift();
      h.pc = ccols.P;
      h.ci = ccols.shift();
      h.nt_r = (int) nt;
      h.last_rows = rows.last_extent();
      h.nt_c = (int) ccols.nt();
      h.last_cols = ccols.last_extent();
      h.herm = 0;
      h.w = ps.W;
      h.ldw = ldp;
      h.e0 = e0;
      h.ncols = nrefl;
      h.kinds = 2;
      h.chunk_t = tile_panel_pick_chunk(cltc, nb, nrefl, std::max<long>(cltr - il0, 1), false, sizeof(T));
      h.layers_t = tile_panel_layers(std::max<long>(cltr - il0, 1), h.chunk_t);
      h.part_t = part_t;
      if (il0 < cltr) {
        launch_tile_panel(h, s);
        // (every tile column of C has the same cltr - il0 sources: all layers_t runs exist, + the extra layer)
        launch_layers_reduce(part_t, h.layers_t + h.split, cltc * nb, nrefl, W2H, ldw2, s);
      }
      else {
        DLAF_HIP_CHECK(hipMemsetAsync(W2H, 0, (size_t) ldw2 * nrefl * sizeof(T), s));
      }
      if (rows.P > 1)
        tr->allreduce_sum(W2H, (size_t) ldw2 * nrefl, TypeInfo<T>::tag, 'C', s);
      // C -= V W2 = V (W2^H)^H
      if (il0 < cltr) {
        // (C's rows are spread like A's; V is a row range of the column-major panel, W2^H one nb-row block per column)
        UpdateArgs<T> ua = rect_update_args(C, il0, cltr, 0, cltc, V + (rows.global_of(il0) * nb - e0), W2H, (long) nb,
                                            nrefl, info);
        ua.a_ts = (long) rows.P * nb;
        ua.lda = (int) ldp;
        ua.ldb = (int) ldw2;
        launch_update(ua, s, 3);
      }
    }
    if (ps.dist)
      DLAF_HIP_CHECK(hipStreamSynchronize(s));
  }
  DLAF_HIP_CHECK(hipEventRecord(ev1, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  float ms = 0;
  DLAF_HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
  g_last_ms = ms;
  // miniapp_bt_reduction_to_band.cpp:160-164: add_mul = (m - b)^2 n
  g_last_flops = (TypeInfo<T>::is_complex ? 4.0 : 1.0) * 2.0 * (double) (n - b) * (double) (n - b) * (double) ccols.n;
  DLAF_HIP_CHECK(hipEventDestroy(ev0));
  DLAF_HIP_CHECK(hipEventDestroy(ev1));
  return 0;
}

template <class T>
int bt_reduction_to_band_host(Grid* g, int band, HostOperand<T> c, HostOperand<const T> a, const T* taus) {
  DeviceMatrix<T> A;
  A.create(g, 'L', a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  TileMatrix<T> C;
  C.create(g, false, c.m, c.n, c.nb, c.isrc, c.jsrc);
  C.upload(c.p, c.ld, false, false, T{}, A.s_high);
  const int r = bt_reduction_to_band_device(band, C, A, taus);
  C.download(c.p, c.ld, false, A.s_high);
  DLAF_HIP_CHECK(hipStreamSynchronize(A.s_high));
  return r;
}

#define INST(T)                                                           \
  template int reduction_to_band_device<T>(DeviceMatrix<T>&, int, T*);    \
  template int reduction_to_band_host<T>(Grid*, HostOperand<T>, int, T*); \
  template int bt_reduction_to_band_device<T>(int, TileMatrix<T>&, DeviceMatrix<T>&, const T*); \
  template int bt_reduction_to_band_host<T>(Grid*, int, HostOperand<T>, HostOperand<const T>, const T*);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
