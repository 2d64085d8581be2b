// device_matrix.cpp -- the life of a DeviceMatrix: workspaces, streams and events, upload / download, wait() and the
// blocking entry points, the residual checker and the measurement hooks; the issue order of a factorization is in
// cholesky.cpp.  See device_matrix.hpp for what each piece replaces in the reference.
#include "device_matrix.hpp"
#include "launch_args.hpp"
#include "pool.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace dlaf_mi355x {

// =============================================================================== DeviceMatrix
static std::vector<hipEvent_t> make_events(size_t n) {
  std::vector<hipEvent_t> v(n);
  for (auto& e : v)
    DLAF_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return v;
}

static int compute_units() {
  hipDeviceProp_t prop;
  int dev = 0;
  DLAF_HIP_CHECK(hipGetDevice(&dev));
  DLAF_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  return prop.multiProcessorCount;
}

template <class T>
long update_bulk_slots() {
  runtime_init();
  return (long) compute_units() * update_blocks_per_cu<T>();
}

template <class T>
void DeviceMatrix<T>::create(Grid* g, char uplo_, long n_, int nb_, int isrc, int jsrc) {
  runtime_init();
  type = TypeInfo<T>::tag;
  grid = g;
  (void) grid_transport(*g);
  uplo = (uplo_ == 'U' || uplo_ == 'u') ? 'U' : 'L';
  transposed = (uplo == 'U');
  n = n_;
  nb = nb_;
  Axis srow{n, nb, g->nprow, g->myrow, isrc};
  Axis scol{n, nb, g->npcol, g->mycol, jsrc};
  rows = transposed ? scol : srow;
  cols = transposed ? srow : scol;
  nt = rows.nt();
  ltr = rows.local_tiles();
  ltc = cols.local_tiles();
  tile_elems = (size_t) nb * nb;

  tiles = dev_alloc<T>((size_t) ltr * ltc * tile_elems);
  winv = dev_alloc<T>(2 * winv_elems());  // alternating by step parity
  const bool dist = g->nranks > 1;
  if (dist) {
    diag_ws = dev_alloc<T>(2 * (tile_elems + winv_elems()));  // alternating by step parity
    for (int b = 0; b < 2; ++b) {
      panel[b] = dev_alloc<T>((size_t) ltr * tile_elems);
      // grouped by root process row: up to rows.P classes of ceil(ltc / classes) tiles each
      panelT[b] = dev_alloc<T>((size_t) (ltc + rows.P) * tile_elems);
    }
  }
  bulk_slots = update_bulk_slots<T>();
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&info), sizeof(int)));
  // NOT hipMemset: that call returns before its fill has run, on the null stream, which the streams below do not
  // synchronise with -- the fill could land after the first diagonal tile's POTRF had flagged its pivot, and the
  // factorization of a matrix that is not positive definite came back with info 0 (README, round 4).
  DLAF_HIP_CHECK(zero_device_now(info, sizeof(int)));
  // Flags and counters of the launches that need them: a slice of 16 words (8 dequeue heads + 8 pacing counters)
  // per persistent update launch, then a slice per diagonal tile for the cooperative POTRF.  The whole buffer is
  // zeroed ONCE per factorization and every launch gets a slice of its own: no fill kernel in front of every
  // bulk launch and every tile POTRF.  (Measured A/B on one box, N = 32768 nb = 512: 59.43 against 59.40 TFlop/s --
  // the fill kernels were not on the critical path; kept because it removes ~110 launches per factorization.)
  {
    const size_t nt_ = (size_t) std::max<long>(1, (n + nb - 1) / nb);
    coop_sync_update_slices = 6 * nt_ + 8;
    coop_sync_potrf_words = potrf_coop_sync_words(nb);
    coop_sync_words = 16 * coop_sync_update_slices + coop_sync_potrf_words * nt_;
  }
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&coop_sync), sizeof(unsigned) * coop_sync_words));
  DLAF_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&info_host), sizeof(int), hipHostMallocDefault));
  *info_host = 0;

  // POTRF / TRSM / lookahead column on a high-priority stream, the bulk of the trailing update on a
  // normal one (the reference's priority rule, cholesky/impl.h:172-173, src/init.cpp:70-83)
  int lo = 0, hi = 0;
  DLAF_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_high, hipStreamNonBlocking, hi));
  // Tuning knobs (tune.h analogue): DLAF_MI355X_SERIAL=1 issues everything on one stream (no
  // lookahead); DLAF_MI355X_RESERVED_CUS=R keeps R compute units out of the bulk-update stream so
  // the critical-path kernels (POTRF chain, panel TRSM) never queue behind long update workgroups.
  const char* serial = std::getenv("DLAF_MI355X_SERIAL");
  const char* rcu = std::getenv("DLAF_MI355X_RESERVED_CUS");
  const int reserved = rcu ? std::atoi(rcu) : 0;  // CU-masked streams measured slower on MI355X
  if (serial && std::atoi(serial) != 0) {
    s_low = s_high;
  }
  else if (reserved > 0) {
    const int ncu = compute_units();
    std::vector<uint32_t> mask((size_t) (ncu + 31) / 32, 0u);
    for (int cu = reserved; cu < ncu; ++cu)
      mask[(size_t) cu / 32] |= 1u << (cu % 32);
    DLAF_HIP_CHECK(hipExtStreamCreateWithCUMask(&s_low, (uint32_t) mask.size(), mask.data()));
  }
  else {
    DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_low, hipStreamNonBlocking, lo));
  }
  DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_comm, hipStreamNonBlocking, hi));
  const size_t ne = (size_t) (nt > 0 ? nt : 1);
  ev_panel = make_events(ne);
  ev_done = make_events(1);
  ev_high = make_events(ne);
  ev_diag = make_events(ne);
  ev_bcast = make_events(ne);
  ev_head = make_events(ne);
  ev_headb = make_events(ne);
  ev_start = make_events(2);
}

template <class T>
void DeviceMatrix<T>::destroy() {
  if (!tiles)
    return;
  (void) hipDeviceSynchronize();
  for (auto* v : {&ev_panel, &ev_done, &ev_high, &ev_diag, &ev_bcast, &ev_start, &ev_head, &ev_headb}) {
    for (auto e : *v)
      (void) hipEventDestroy(e);
    v->clear();
  }
  for (auto& ps : prof) {
    for (auto e : ps.start)
      (void) hipEventDestroy(e);
    for (auto e : ps.stop)
      (void) hipEventDestroy(e);
    ps.start.clear();
    ps.stop.clear();
  }
  if (s_low != s_high)
    (void) hipStreamDestroy(s_low);
  (void) hipStreamDestroy(s_high);
  (void) hipStreamDestroy(s_comm);
  (void) hipFree(tiles);
  (void) hipFree(winv);
  if (diag_ws)
    (void) hipFree(diag_ws);
  for (int b = 0; b < 2; ++b) {
    if (panel[b])
      (void) hipFree(panel[b]);
    if (panelT[b])
      (void) hipFree(panelT[b]);
  }
  if (staging)
    (void) hipFree(staging);
  (void) hipFree(info);
  (void) hipFree(coop_sync);
  (void) hipHostFree(info_host);
  tiles = nullptr;
}

template <class T>
static void ensure_staging(DeviceMatrix<T>& m, size_t elems) {
  if (m.staging && m.staging_elems >= elems)
    return;
  if (m.staging)
    DLAF_HIP_CHECK(hipFree(m.staging));
  m.staging = dev_alloc<T>(elems);
  m.staging_elems = elems;
}

// The uplo triangle of the caller's local array as one rectangle per local tile column of the SOURCE:
// f(row0, nrows, col0, ncols) in source element coordinates; diag(row0, col0, rows, cols) for every local
// diagonal tile (whose other half lies inside a rectangle but is not part of the triangle).
template <class T, class F, class D>
static void for_each_triangle_block(const DeviceMatrix<T>& m, F&& f, D&& diag) {
  long srows, scols;
  source_extents(m, srows, scols);
  // source axes: rows of the source are the view's rows (uplo L) or the view's columns (uplo U)
  const Axis& srow_ax = m.transposed ? m.cols : m.rows;
  const Axis& scol_ax = m.transposed ? m.rows : m.cols;
  const long nlc = scol_ax.local_tiles();
  for (long jl = 0; jl < nlc; ++jl) {
    const long gj = scol_ax.global_of(jl);
    const long col0 = jl * m.nb, ncols = std::min<long>(m.nb, scols - col0);
    long row0, row1;
    if (!m.transposed) {  // lower: source tile rows with global index >= gj
      row0 = std::min(srow_ax.next_local(gj) * m.nb, srows);
      row1 = srows;
    }
    else {  // upper: source tile rows with global index <= gj
      row0 = 0;
      row1 = std::min(srow_ax.next_local(gj + 1) * m.nb, srows);
    }
    if (ncols > 0 && row1 > row0)
      f(row0, row1 - row0, col0, ncols);
    if (srow_ax.mine(gj)) {
      const long r0 = srow_ax.local_of(gj) * m.nb;
      diag(r0, col0, std::min<long>(m.nb, srows - r0), ncols);
    }
  }
}

template <class T>
void DeviceMatrix<T>::upload(const T* host, long ld) {
  long srows, scols;
  source_extents(*this, srows, scols);
  if (srows == 0 || scols == 0)
    return;
  const long lds = srows;
  ensure_staging(*this, (size_t) lds * scols);
  // only the uplo triangle crosses PCIe (the relayout never reads the other one); the copies, the relayout and the
  // closing synchronisation share one stream, so the caller's array is free to go when this returns
  for_each_triangle_block(
      *this,
      [&](long r0, long nr, long c0, long nc) {
        DLAF_HIP_CHECK(hipMemcpy2DAsync(staging + r0 + c0 * lds, (size_t) lds * sizeof(T), host + r0 + c0 * ld,
                                        (size_t) ld * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                        hipMemcpyHostToDevice, s_high));
      },
      [](long, long, long, long) {});
  launch_to_tiles(layout_args(*this, staging, lds), s_high);
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
}

template <class T>
void DeviceMatrix<T>::download(T* host, long ld, bool staging_is_current) {
  long srows, scols;
  source_extents(*this, srows, scols);
  if (srows == 0 || scols == 0)
    return;
  const long lds = srows;
  ensure_staging(*this, (size_t) lds * scols);
  // The other half of the diagonal tiles travels back inside the rectangles and must come back unchanged:
  // it is already in the staging copy when that was filled from this very array and no caller code ran in
  // between (the blocking host entry points say so), otherwise the diagonal tiles are staged first.
  if (!staging_is_current) {
    for_each_triangle_block(
        *this, [](long, long, long, long) {},
        [&](long r0, long c0, long nr, long nc) {
          if (nr > 0 && nc > 0)
            DLAF_HIP_CHECK(hipMemcpy2DAsync(staging + r0 + c0 * lds, (size_t) lds * sizeof(T), host + r0 + c0 * ld,
                                            (size_t) ld * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                            hipMemcpyHostToDevice, s_high));
        });
  }
  launch_from_tiles(layout_args(*this, staging, lds), s_high);
  for_each_triangle_block(
      *this,
      [&](long r0, long nr, long c0, long nc) {
        DLAF_HIP_CHECK(hipMemcpy2DAsync(host + r0 + c0 * ld, (size_t) ld * sizeof(T), staging + r0 + c0 * lds,
                                        (size_t) lds * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                        hipMemcpyDeviceToHost, s_high));
      },
      [](long, long, long, long) {});
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
}

template <class T>
void DeviceMatrix<T>::copy_from(const DeviceMatrix<T>& o) {
  if (o.n != n || o.nb != nb || o.ltr != ltr || o.ltc != ltc || o.transposed != transposed)
    fatal("[dlaf_mi355x] copy_from: matrices differ in shape or distribution\n");
  DLAF_HIP_CHECK(hipMemcpyAsync(tiles, o.tiles, (size_t) ltr * ltc * tile_elems * sizeof(T),
                                hipMemcpyDeviceToDevice, s_high));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
}

template <class T>
void DeviceMatrix<T>::prof_begin(int kind, hipStream_t s) {
  if (!profiling)
    return;
  ProfSlot& p = prof[kind];
  if (p.used == p.start.size()) {
    hipEvent_t a, b;
    DLAF_HIP_CHECK(hipEventCreate(&a));
    DLAF_HIP_CHECK(hipEventCreate(&b));
    p.start.push_back(a);
    p.stop.push_back(b);
  }
  DLAF_HIP_CHECK(hipEventRecord(p.start[p.used], s));
}

template <class T>
void DeviceMatrix<T>::prof_end(int kind, hipStream_t s, double flops, double bytes) {
  if (!profiling)
    return;
  ProfSlot& p = prof[kind];
  DLAF_HIP_CHECK(hipEventRecord(p.stop[p.used], s));
  ++p.used;
  p.flops += flops;
  p.bytes += bytes;
}

// ------------------------------------------------------------------------------- residual checker
// max|A - L L^H| / max|A| as the reference's miniapp computes it (miniapp_cholesky.cpp:243-443:
// setUpperToZeroForDiagonalTiles, cholesky_diff with row/column broadcasts + reduce, max_norm), on the
// device: the same grouped update kernel subtracts L(:,k) L(:,k)^H column panel by column panel, the
// panels travel exactly like in the factorization, the norms are reduced over the grid with MAX.
template <class T>
void DeviceMatrix<T>::residual_of(DeviceMatrix<T>& L, double* max_diff, double* max_a) {
  if (L.n != n || L.nb != nb || L.ltr != ltr || L.ltc != ltc || L.transposed != transposed)
    fatal("[dlaf_mi355x] residual_of: matrices differ in shape or distribution\n");
  Transport* tr = grid_transport(*grid);
  const bool dist = grid->nranks > 1;
  const CommAxis ax_row = transposed ? CommAxis::Col : CommAxis::Row;
  const CommAxis ax_col = transposed ? CommAxis::Row : CommAxis::Col;
  const size_t tile_bytes = tile_elems * sizeof(T);
  hipStream_t s = s_low;
  double* dnorm = nullptr;
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dnorm), 2 * sizeof(double)));
  DLAF_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s));
  launch_max_norm(tiles, (int) ltr, (int) ltc, nb, rows.local_size(), cols.local_size(), rows.P, rows.shift(), cols.P,
                  cols.shift(), dnorm + 1, s);
  launch_zero_upper_diag(L.tiles, (int) ltr, (int) ltc, nb, rows.P, rows.shift(), cols.P, cols.shift(), s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  for (long k = 0; k < nt; ++k) {
    const int kb = rows.tile_extent(k);
    const int own_c = cols.owner(k);
    const bool in_col = cols.rank == own_c;
    const long il_f = rows.next_local(k), jl_f = cols.next_local(k);
    const long klc = in_col ? cols.local_of(k) : -1;
    if (il_f >= ltr && !dist)
      continue;
    const T* a_base;
    const T* b_base;
    long b_ts = (long) tile_elems;
    if (cols.P > 1) {
      T* dst = in_col ? L.tile(il_f < ltr ? il_f : 0, klc) : panel[0];
      if (il_f < ltr)
        tr->bcast(ax_row, own_c, cols.rank, dst, dst, (size_t) (ltr - il_f) * tile_bytes, s);
      a_base = dst;
    }
    else {
      a_base = L.tile(il_f < ltr ? il_f : 0, klc);
    }
    int b_period = 1;
    long b_ts2 = 0;
    if (rows.P > 1) {
      bcast_transposed_panel(tr, ax_col, a_base, il_f, jl_f, panelT[0], s, b_period, b_ts2);
      b_base = panelT[0];
    }
    else {
      b_base = a_base + (cols.global_of(jl_f) - il_f) * (long) tile_elems;
      b_ts = (long) tile_elems * cols.P;
    }
    if (il_f >= ltr || jl_f >= ltc)
      continue;
    const long il0 = std::max(il_f, rows.next_local(cols.global_of(jl_f)));
    if (il0 >= ltr)
      continue;
    UpdateArgs<T> ua = update_args(*this, il0, ltr, jl_f, ltc, a_base + (size_t) (il0 - il_f) * tile_elems, b_base, b_ts,
                                   kb, info);
    ua.b_period = b_period;
    ua.b_ts2 = b_ts2;
    ua.b_jl0 = (int) jl_f;
    launch_update(ua, s, 3);
    if (dist)
      DLAF_HIP_CHECK(hipStreamSynchronize(s));  // the single panel workspace is reused by the next step
  }
  launch_max_norm(tiles, (int) ltr, (int) ltc, nb, rows.local_size(), cols.local_size(), rows.P, rows.shift(), cols.P,
                  cols.shift(), dnorm, s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  double h[2];
  DLAF_HIP_CHECK(hipMemcpy(h, dnorm, sizeof(h), hipMemcpyDeviceToHost));
  DLAF_HIP_CHECK(hipFree(dnorm));
  if (dist)
    tr->allreduce_max(h, 2, grid->nprow, grid->npcol, grid->myrow, grid->mycol);
  if (max_diff)
    *max_diff = h[0];
  if (max_a)
    *max_a = h[1];
}

template <class T>
int DeviceMatrix<T>::wait() {
  DLAF_HIP_CHECK(hipStreamSynchronize(s_comm));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_low));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
  DLAF_HIP_CHECK(hipMemcpy(info_host, info, sizeof(int), hipMemcpyDeviceToHost));
  local_info = *info_host;
  // DLAF_MI355X_INFO_VERBOSE=1: this rank's own status word before the grid agrees on one (diagnosis of the
  // intermittent "owner did not report its negative pivot" failure of the six-rank test worker, README status)
  static const bool info_verbose = [] {
    const char* e = std::getenv("DLAF_MI355X_INFO_VERBOSE");
    return e && std::atoi(e) != 0;
  }();
  if (info_verbose)
    std::fprintf(stderr, "[dlaf_mi355x] rank (%d,%d) of %dx%d: local info %d (n %ld nb %d)\n", grid->myrow, grid->mycol,
                 grid->nprow, grid->npcol, *info_host, n, nb);
  // one value for the whole grid (ScaLAPACK's p?potrf contract; the reference aborts every rank,
  // src/cusolver/assert_info.cu:35-45)
  *info_host = agree_on_info(*grid, *info_host);
  if (*info_host == kInfoSchedulingFailure)
    fatal("[dlaf_mi355x] cooperative POTRF: a bounded inter-workgroup wait expired (workgroups not co-resident); "
          "the result is invalid. DLAF_MI355X_POTRF=chain selects the non-cooperative path.\n");
  for (auto& ps : prof) {
    ps.ms = 0;
    ps.launches = (long) ps.used;
    for (size_t i = 0; i < ps.used; ++i) {
      float ms = 0;
      DLAF_HIP_CHECK(hipEventElapsedTime(&ms, ps.start[i], ps.stop[i]));
      ps.ms += ms;
    }
  }
  return *info_host;
}

template <class T>
bool DeviceMatrix<T>::fetch_tile(long gi, long gj, T* host, long ld) {
  // view indices: the device holds the transposed view for uplo == 'U'
  const long vi = transposed ? gj : gi, vj = transposed ? gi : gj;
  if (vi < 0 || vj < 0 || vi >= nt || vj >= nt || !rows.mine(vi) || !cols.mine(vj))
    return false;
  const int r = rows.tile_extent(vi), c = cols.tile_extent(vj);
  const T* src = tile(rows.local_of(vi), cols.local_of(vj));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_low));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
  if (!transposed) {
    DLAF_HIP_CHECK(hipMemcpy2D(host, (size_t) ld * sizeof(T), src, (size_t) nb * sizeof(T), (size_t) r * sizeof(T),
                               (size_t) c, hipMemcpyDeviceToHost));
  }
  else {
    T* tmp = dev_alloc<T>(tile_elems);
    launch_copy2d(tmp, (long) c, src, (long) nb, c, r, 1, 0, s_high);  // caller's tile is c x r
    DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
    DLAF_HIP_CHECK(hipMemcpy2D(host, (size_t) ld * sizeof(T), tmp, (size_t) c * sizeof(T), (size_t) c * sizeof(T),
                               (size_t) r, hipMemcpyDeviceToHost));
    DLAF_HIP_CHECK(hipFree(tmp));
  }
  return true;
}

template <class T>
double DeviceMatrix<T>::trsm_profile(int reps, double* flops, double* bytes) {
  if (flops)
    *flops = 0;
  if (bytes)
    *bytes = 0;
  if (grid->nranks != 1 || nt < 2 || reps < 1)
    return 0.0;
  const long ntiles = ltr - 1;
  T* scratch = dev_alloc<T>((size_t) ntiles * tile_elems);
  T* w = dev_alloc<T>(winv_elems());
  hipStream_t s = s_low;
  DLAF_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s));
  launch_invert_diag_blocks(tile(0, 0), nb, nb, w, info, s, false, false);
  // the panel of step 0 (one process: local row il is global tile il), solved on the copy
  TrsmArgs<T> ta = panel_args<TrsmArgs<T>>(*this, 1, ltr, 0, tile(0, 0), nb);
  ta.b = scratch;
  ta.winv = w;
  ta.info = info;
  hipEvent_t e0, e1;
  DLAF_HIP_CHECK(hipEventCreate(&e0));
  DLAF_HIP_CHECK(hipEventCreate(&e1));
  float total = 0;
  for (int r = -1; r < reps; ++r) {  // r = -1: warm-up
    // a fresh copy of the solved panel each time (X L^-H applied again and again would shrink to nothing)
    DLAF_HIP_CHECK(hipMemcpyAsync(scratch, tile(1, 0), (size_t) ntiles * tile_elems * sizeof(T), hipMemcpyDeviceToDevice, s));
    DLAF_HIP_CHECK(hipEventRecord(e0, s));
    launch_trsm(ta, s);
    DLAF_HIP_CHECK(hipEventRecord(e1, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    DLAF_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0)
      total += ms;
  }
  (void) hipEventDestroy(e0);
  (void) hipEventDestroy(e1);
  DLAF_HIP_CHECK(hipFree(scratch));
  DLAF_HIP_CHECK(hipFree(w));
  double fl = 0, by = 0;
  for (long il = 1; il < ltr; ++il) {
    const double mi = rows.tile_extent(rows.global_of(il));
    fl += (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (double) nb * nb * mi;
    by += (0.5 * nb * nb + 2.0 * mi * nb) * sizeof(T);
  }
  if (flops)
    *flops = fl;
  if (bytes)
    *bytes = by;
  return (double) total / reps;
}

template <class T>
int DeviceMatrix<T>::factorize() {
  factorize_async();
  return wait();
}

// View tile column k (rows on/below the diagonal) as a rectangle of the caller's local array.
template <class T>
static bool view_column_rect(const DeviceMatrix<T>& m, long k, long& r0, long& nr, long& c0, long& nc) {
  if (!m.cols.mine(k))
    return false;
  long srows, scols;
  source_extents(m, srows, scols);
  const long jl = m.cols.local_of(k);
  const long first = m.rows.next_local(k) * m.nb;  // first view row (element) on/below the diagonal
  if (!m.transposed) {
    r0 = std::min(first, srows);
    nr = srows - r0;
    c0 = jl * m.nb;
    nc = std::min<long>(m.nb, scols - c0);
  }
  else {  // the view column is a row block of the source
    r0 = jl * m.nb;
    nr = std::min<long>(m.nb, srows - r0);
    c0 = std::min(first, scols);
    nc = scols - c0;
  }
  return nr > 0 && nc > 0;
}

template <class T>
int DeviceMatrix<T>::factorize_and_download(T* host, long ld) {
  long srows, scols;
  source_extents(*this, srows, scols);
  const char* off = std::getenv("DLAF_MI355X_OVERLAP_DOWNLOAD");
  if (srows == 0 || scols == 0 || nt < 3 || (off && std::atoi(off) == 0)) {
    const int r = factorize();
    if (r == 0)
      download(host, ld, true);
    return r;
  }
  const long lds = srows;
  int dev = 0;
  DLAF_HIP_CHECK(hipGetDevice(&dev));
  panels_issued.store(-1, std::memory_order_release);
  std::atomic<bool> stop{false};
  auto fetch_column = [&](long k, hipStream_t s) {
    long r0, nr, c0, nc;
    if (!view_column_rect(*this, k, r0, nr, c0, nc))
      return;
    LayoutArgs<T> la = layout_args(*this, staging, lds);
    la.jl_first = (int) cols.local_of(k);
    la.jl_count = 1;
    launch_from_tiles(la, s);
    DLAF_HIP_CHECK(hipMemcpy2DAsync(host + r0 + c0 * ld, (size_t) ld * sizeof(T), staging + r0 + c0 * lds,
                                    (size_t) lds * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                    hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
  };
  // columns 0 .. nt-2 leave as soon as their panel is solved; the helper never touches a column whose event
  // has not been recorded yet (panels_issued), and the device flag stops it on a failed factorization
  std::thread helper([&] {
    DLAF_HIP_CHECK(hipSetDevice(dev));
    hipStream_t s_dl = nullptr;
    DLAF_HIP_CHECK(hipStreamCreateWithFlags(&s_dl, hipStreamNonBlocking));
    for (long k = 0; k + 1 < nt; ++k) {
      while (panels_issued.load(std::memory_order_acquire) < k && !stop.load(std::memory_order_acquire))
        std::this_thread::yield();
      if (panels_issued.load(std::memory_order_acquire) < k)
        break;
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_dl, ev_panel[k], 0));
      fetch_column(k, s_dl);
    }
    DLAF_HIP_CHECK(hipStreamDestroy(s_dl));
  });
  factorize_async();
  const int r = wait();
  stop.store(true, std::memory_order_release);
  helper.join();
  if (r == 0)
    fetch_column(nt - 1, s_high);
  return r;
}

#define INST(T)                         \
  template long update_bulk_slots<T>(); \
  template struct DeviceMatrix<T>;
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
