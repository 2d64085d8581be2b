// eigensolver.cpp -- band -> tridiagonal, the back-transformation band <- tridiagonal, and the drivers of the
// Hermitian (generalized) eigensolver (BASELINE configuration 5).
//
// Reference: Eigensolver::call (include/dlaf/eigensolver/eigensolver/impl.h:38-55 local, :57-95 distributed):
//   reduction_to_band -> band_to_tridiagonal<Backend::MC> -> tridiagonal_eigensolver -> bt_band_to_tridiagonal ->
//   bt_reduction_to_band;  GenEigensolver::call (gen_eigensolver/impl.h:33-92): cholesky_factorization of B,
//   generalized_to_standard, the eigensolver, triangular_solver (Left, uplo, ConjTrans) on the eigenvectors.
//   band_to_tridiagonal: band_to_tridiag/mc.h:681-867 (local), :1016-1558 (distributed, a pipeline of sweeps over
//   1-D blocks of the band with point-to-point messages); bt_band_to_tridiagonal: bt_band_to_tridiag/impl.h:609-736.
//
// MI355X design.  The band (2 b n elements: 42 MB at n = 20480) and the tridiagonal problem are small next to one
// GPU's memory and bandwidth, so a process grid does not pipeline them over ranks: the band is summed over the grid
// (one all-reduce), the bulge chase runs replicated, ONE launch per rank (kernels_tridiag.hip); what is distributed
// is what costs n^3: the eigenvector matrix of the back-transformations.
//   bt_band_to_tridiagonal: the b x b blocks of compact reflectors become well-formed 2b x b blocks V with their
//   T factors (all blocks at once: one expand launch, three strided-batch launches), then the blocks are applied in
//   WAVEFRONTS -- block (jb, step) touches rows [1 + (jb + step) b, +2b) and must follow (jb, step - 1) and the blocks
//   of sweep group jb + 1 that overlap it, so all blocks with the same step - jb are independent: W2 = V^H E and
//   E -= (V T) W2 run as two strided-batch GEMM launches per wavefront instead of two per block.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../device/band_api.hpp"
#include "../device/tridiag_api.hpp"
#include "bt_wavefronts.hpp"
#include "drivers.hpp"
#include "eigensolver.hpp"
#include "pool.hpp"

namespace dlaf_mi355x {

namespace {
double g_stage_ms[5] = {0, 0, 0, 0, 0};

struct StageTimer {
  hipEvent_t a, b;
  hipStream_t s;
  explicit StageTimer(hipStream_t st) : s(st) {
    DLAF_HIP_CHECK(hipEventCreate(&a));
    DLAF_HIP_CHECK(hipEventCreate(&b));
    DLAF_HIP_CHECK(hipEventRecord(a, s));
  }
  double stop() {
    DLAF_HIP_CHECK(hipEventRecord(b, s));
    DLAF_HIP_CHECK(hipEventSynchronize(b));
    float ms = 0;
    DLAF_HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    DLAF_HIP_CHECK(hipEventDestroy(a));
    DLAF_HIP_CHECK(hipEventDestroy(b));
    return ms;
  }
};

// an on/off switch of the environment; every caller keeps what it read (static const): a switch is read once
bool env_flag(const char* name, bool dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) != 0 : dflt;
}

// DLAF_MI355X_EIG_DEBUG=1: a checksum of every stage's output (diagnosis: each stage is deterministic).  Who prints:
// the words in front of the name and the width of the name's column.
struct DebugWho {
  char words[48];
  int width;
};
const DebugWho kBtDebug = {"bt debug", 22};
DebugWho eig_debug(const Grid* g) {
  DebugWho w;
  std::snprintf(w.words, sizeof(w.words), "eig debug rank (%d,%d)", g->myrow, g->mycol);
  w.width = 24;
  return w;
}
bool debug_on() {
  static const bool on = env_flag("DLAF_MI355X_EIG_DEBUG", false);
  return on;
}
// FNV-1a over the 64-bit words of a device range (the last one padded with zeros), continued from acc
constexpr unsigned long long kFnvSeed = 1469598103934665603ull;
unsigned long long fnv1a_device(unsigned long long acc, const void* dev, size_t bytes) {
  std::vector<unsigned long long> h((bytes + 7) / 8, 0ull);
  DLAF_HIP_CHECK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
  for (unsigned long long x : h)
    acc = (acc ^ x) * 1099511628211ull;
  return acc;
}
void debug_print(const DebugWho& who, const char* what, unsigned long long acc) {
  std::fprintf(stderr, "[dlaf_mi355x] %s %-*s %016llx\n", who.words, who.width, what, acc);
}
void debug_checksum(const DebugWho& who, hipStream_t s, const char* what, const void* dev, size_t bytes) {
  if (!debug_on())
    return;
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  debug_print(who, what, fnv1a_device(kFnvSeed, dev, bytes));
}
}  // namespace

// E of the back-transformation band <- tridiagonal: leading dimension a multiple of 16 bytes, element 1 (not 0) on a
// 16-byte boundary
long bt_aligned_ld(long n) {
  return ((n + 1) / 2) * 2;
}
template <class T>
T* bt_aligned_base(T* alloc) {
  // hipMalloc returns 256-byte aligned memory: one element in front for 8-byte types, none for 16-byte ones, three for
  // 4-byte ones
  if (sizeof(T) == 16)
    return alloc;
  return alloc + (16 / sizeof(T) - 1);
}

void eigensolver_last_profile(double ms[5]) {
  for (int i = 0; i < 5; ++i)
    ms[i] = g_stage_ms[i];
}
void eigensolver_set_stage_ms(int stage, double ms) {
  g_stage_ms[stage] = ms;
}

// ------------------------------------------------------------------------------------------------ band -> tridiagonal
template <class T>
int band_to_tridiag_device(DeviceMatrix<T>& A, int band, real_t<T>* d, real_t<T>* e, T* v, long ldv) {
  if (A.transposed)
    fatal("[dlaf_mi355x] band_to_tridiagonal: the matrix must be held as uplo = L (band_to_tridiag.h:82-92: Upper is "
          "not implemented upstream either)\n");
  if (band < 2 || A.nb % band != 0)
    fatal("[dlaf_mi355x] band_to_tridiagonal: band_size %d must be >= 2 and divide the block size %d "
          "(band_to_tridiag.h:78-80)\n", band, A.nb);
  if (band > b2t_max_band())
    fatal("[dlaf_mi355x] band_to_tridiagonal: band_size %d above the supported %d\n", band, b2t_max_band());
  Grid* grid = A.grid;
  Transport* tr = checked_transport(*grid);
  const bool dist = grid->nranks > 1;
  const long n = A.n;
  hipStream_t s = A.s_high;
  DLAF_HIP_CHECK(hipMemsetAsync(A.info, 0, sizeof(int), s));
  if (n == 0)
    return 0;
  StageTimer timer(s);
  PoolScope ws;
  T* bandm = ws.get<T>((size_t) (n + 2) * 2 * band);
  // (the two columns of slack behind the matrix are read, never used: they must hold numbers)
  DLAF_HIP_CHECK(hipMemsetAsync(bandm + (size_t) n * 2 * band, 0, (size_t) 2 * 2 * band * sizeof(T), s));
  unsigned* sync = ws.get<unsigned>(b2t_sync_words(n));
  launch_band_extract(A.tiles, A.ltr, A.nb, A.rows.P, A.rows.shift(), A.cols.P, A.cols.shift(), n, band, bandm, s);
  if (dist)
    tr->allreduce_sum(bandm, (size_t) n * 2 * band, TypeInfo<T>::tag, 'A', s);
  DLAF_HIP_CHECK(hipMemset2DAsync(v, (size_t) ldv * sizeof(T), 0, (size_t) n * sizeof(T), (size_t) n, s));
  // the bulge chase works on 2^-k A, max(|Re|, |Im|) in [1, 2): its unscaled sums of squares neither overflow nor
  // underflow whatever the scale of A (every rank holds the same band after the all-reduce and takes the same k)
  unsigned long long* mx = ws.get<unsigned long long>(1);
  launch_band_normalise(bandm, n, band, mx, s);
  launch_band_to_tridiag(bandm, n, band, v, ldv, sync, A.info, s);
  launch_tridiag_extract(bandm, n, band, mx, d, e, s);
  int h_info = 0;
  DLAF_HIP_CHECK(hipMemcpyAsync(&h_info, A.info, sizeof(int), hipMemcpyDeviceToHost, s));
  g_stage_ms[1] = timer.stop();
  ws.release();
  if (h_info == kInfoSchedulingFailure)
    fatal("[dlaf_mi355x] band_to_tridiagonal: a sweep gave up waiting for its predecessor (the workgroup that owns it "
          "made no progress)\n");
  return h_info;
}

template <class T>
int band_to_tridiag_host(Grid* g, HostOperand<const T> a, int band, real_t<T>* d, real_t<T>* e, T* v, long ldv) {
  using R = real_t<T>;
  const long n = a.n;
  DeviceMatrix<T> A;
  A.create(g, 'L', n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  PoolScope ws;
  R* dd = ws.get<R>((size_t) n);
  R* de = ws.get<R>((size_t) n);
  T* dv = ws.get<T>((size_t) n * n);
  const int r = band_to_tridiag_device(A, band, dd, de, dv, n);
  if (n > 0) {
    DLAF_HIP_CHECK(hipMemcpy(d, dd, (size_t) n * sizeof(R), hipMemcpyDeviceToHost));
    DLAF_HIP_CHECK(hipMemcpy(e, de, (size_t) n * sizeof(R), hipMemcpyDeviceToHost));
    DLAF_HIP_CHECK(hipMemcpy2D(v, (size_t) ldv * sizeof(T), dv, (size_t) n * sizeof(T), (size_t) n * sizeof(T), (size_t) n,
                               hipMemcpyDeviceToHost));
  }
  return r;
}

// ------------------------------------------------------------------------------------------------ band <- tridiagonal
namespace {
// what the steps of bt_band_to_tridiagonal share.  Block (jb, ib) -- sweep group jb, rows 1 + ib b -- lives in slot
// jb nblk + ib of vx (V, 2b x b; fused: V^T), wx (W = V T), sm (S = V^H V), tm (T) and taus; it exists for jb <= ib only.
template <class T>
struct BtBlocks {
  long n;
  int b;
  long nblk;    // block rows and columns of the block grid
  size_t vblk;  // elements of a block of vx / wx
  bool fused;   // fp64, band 128: the fused kernel (kernels_bt.hip) on E transposed
  const T* v;
  long ldv;
  T* e;
  long lde, ncols;
  T *vx, *wx, *sm, *tm, *taus;
  double* et;  // fused: E^T (ncols x n, ldet)
  long ldet;
  T* w2;  // strided batch: W2 = V^H E of a batch
  hipStream_t s;
};

// DLAF_MI355X_BT_VERBOSE=1: wall time of the phases of this stage (synchronising: diagnosis only)
struct BtPhases {
  hipStream_t s;
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    static const bool verbose = env_flag("DLAF_MI355X_BT_VERBOSE", false);
    if (!verbose)
      return;
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[dlaf_mi355x] bt_band_to_tridiagonal: %-28s %8.2f ms\n", what,
                 std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  }
};

// The reflector blocks: the compact reflectors expanded to well-formed V (and their taus), then per row of the block
// grid -- the blocks ib = jb .. nblk - 1 of sweep group jb, instead of all nblk^2 slots (half of which hold zeros: 28 ms
// of T factors alone at n = 20480) -- S = V^H V, the T factors and W = V T as three strided-batch launches.
// (no memsets: the expansion writes every block (jb <= ib) in full, zeros included, and nothing reads the others)
template <class T>
void bt_prepare_blocks(const BtBlocks<T>& k, long jb_end) {
  const int b = k.b;
  const bool fused = k.fused;
  const size_t vblk = k.vblk, tblk = (size_t) b * b;
  hipStream_t s = k.s;
  // (fused: the expansion writes V^T directly; S = V^H V and W = V T take it as their operand)
  launch_b2t_expand(k.v, k.ldv, k.n, b, k.vx, k.taus, s, fused);
  const T one = make_host_el<T>(1.0), zero = make_host_el<T>(0.0);
  for (long jb = 0; jb < jb_end; ++jb) {
    const size_t q0 = (size_t) jb * k.nblk + (size_t) jb;
    const int cnt = (int) (k.nblk - jb);
    {
      GemmArgs<T> g;  // S = V^H V  (fused: vx holds V^T, S = V^T (V^T)^H for the real types of that path)
      g.M = b;
      g.N = b;
      g.K = 2 * b;
      g.a = k.vx + q0 * vblk;
      g.lda = fused ? b : 2 * b;
      g.opa = fused ? 'N' : 'C';
      g.b = k.vx + q0 * vblk;
      g.ldb = fused ? b : 2 * b;
      g.opb = fused ? 'C' : 'N';
      g.c = k.sm + q0 * tblk;
      g.ldc = b;
      g.alpha = one;
      g.beta = zero;
      g.batch = cnt;
      g.sa = (long) vblk;
      g.sb = (long) vblk;
      g.sc = (long) tblk;
      launch_gemm(g, s);
    }
    launch_tfactor(k.sm + q0 * tblk, (long) b, k.taus + q0 * (size_t) b, b, k.tm + q0 * tblk, (long) b, s, cnt, (long) tblk,
                   (long) b, (long) tblk);
    {
      GemmArgs<T> g;  // W = V T
      g.M = 2 * b;
      g.N = b;
      g.K = b;
      g.a = k.vx + q0 * vblk;
      g.lda = fused ? b : 2 * b;
      g.opa = fused ? 'C' : 'N';
      g.b = k.tm + q0 * tblk;
      g.ldb = b;
      g.opb = 'N';
      g.c = k.wx + q0 * vblk;
      g.ldc = 2 * b;
      g.alpha = one;
      g.beta = zero;
      g.batch = cnt;
      g.sa = (long) vblk;
      g.sb = (long) tblk;
      g.sc = (long) vblk;
      launch_gemm(g, s);
    }
  }
  if (!debug_on())
    return;
  // existing blocks only (the others are never written): block row jb, blocks jb .. nblk - 1
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  const struct {
    const char* name;
    const T* base;
    size_t per;
  } sets[3] = {{"vx", k.vx, vblk}, {"wx", k.wx, vblk}, {"tm", k.tm, tblk}};
  for (const auto& set : sets) {
    unsigned long long acc = kFnvSeed;
    for (long jb = 0; jb < jb_end; ++jb)
      acc = fnv1a_device(acc, set.base + ((size_t) jb * k.nblk + (size_t) jb) * set.per,
                         (size_t) (k.nblk - jb) * set.per * sizeof(T));
    debug_print(kBtDebug, set.name, acc);
  }
}

// fused: E -> E^T in a workspace of ws (the kernel streams V^T and works on columns of E^T)
template <class T>
void bt_transpose_in(BtBlocks<T>& k, PoolScope& ws) {
  k.et = nullptr;
  k.ldet = (k.ncols + 63) / 64 * 64;
  if constexpr (std::is_same_v<T, double>) {
    if (k.fused) {
      k.et = ws.get<double>((size_t) k.ldet * k.n);
      launch_bt_transpose(k.e, k.lde, k.n, k.ncols, k.et, k.ldet, k.s);
    }
  }
  if (k.et)
    debug_checksum(kBtDebug, k.s, "et after transpose", k.et, (size_t) k.ldet * k.n * sizeof(double));
}

// The batches of the wavefront schedule (bt_wavefronts.hpp), each one fused launch or W2 = V^H E and E -= W W2 as two
// strided-batch products: from block to block of a batch nblk + 2 slots of the block grid and 2 b rows of E.
template <class T>
void bt_apply_wavefronts(const BtBlocks<T>& k, const BtSchedule& sc) {
  const int b = k.b;
  const long ncols = k.ncols, max_batch = sc.max_batch();
  const long blk_stride = (long) ((k.nblk + 2) * (long) k.vblk);
  const T one = make_host_el<T>(1.0), zero = make_host_el<T>(0.0), mone = make_host_el<T>(-1.0);
  hipStream_t s = k.s;
  for (const BtBatch& w : bt_wavefront_batches(k.n, b, TypeInfo<T>::is_complex)) {
    if (w.count > max_batch)
      fatal("[dlaf_mi355x] bt_band_to_tridiagonal: wavefront of %ld blocks exceeds the workspace (%ld)\n", w.count,
            max_batch);
    const size_t blk = (size_t) (w.jb * k.nblk + w.ib) * k.vblk;
    if (k.fused) {
      if constexpr (std::is_same_v<T, double>)
        launch_bt_apply(k.vx + blk, k.wx + blk, blk_stride, (int) w.count, k.et, k.ldet, ncols, w.r0, (int) w.rows, s);
      continue;
    }
    GemmArgs<T> g;  // W2 = V^H E
    g.M = b;
    g.N = (int) ncols;
    g.K = (int) w.rows;
    g.a = k.vx + blk;
    g.lda = 2 * b;
    g.opa = 'C';
    g.b = k.e + w.r0;
    g.ldb = k.lde;
    g.opb = 'N';
    g.c = k.w2;
    g.ldc = b;
    g.alpha = one;
    g.beta = zero;
    g.batch = (int) w.count;
    g.sa = blk_stride;
    g.sb = 2L * b;
    g.sc = (long) b * ncols;
    launch_gemm(g, s);
    GemmArgs<T> u;  // E -= W W2
    u.M = (int) w.rows;
    u.N = (int) ncols;
    u.K = b;
    u.a = k.wx + blk;
    u.lda = 2 * b;
    u.opa = 'N';
    u.b = k.w2;
    u.ldb = b;
    u.opb = 'N';
    u.c = k.e + w.r0;
    u.ldc = k.lde;
    u.alpha = mone;
    u.beta = one;
    u.batch = (int) w.count;
    u.sa = blk_stride;
    u.sb = (long) b * ncols;
    u.sc = 2L * b;
    launch_gemm(u, s);
  }
  if (k.et)
    debug_checksum(kBtDebug, s, "et after wavefronts", k.et, (size_t) k.ldet * k.n * sizeof(double));
}

template <class T>
void bt_transpose_back(const BtBlocks<T>& k) {
  if constexpr (std::is_same_v<T, double>) {
    if (k.fused)
      launch_bt_transpose(k.et, k.ldet, k.ncols, k.n, k.e, k.lde, k.s);
  }
}
}  // namespace

template <class T>
int bt_band_to_tridiag_device(long n, int band, const T* v, long ldv, T* e, long lde, long ncols, hipStream_t s) {
  const BtSchedule sc(n, band, TypeInfo<T>::is_complex);
  if (sc.nsweeps <= 0 || ncols <= 0)
    return 0;
  if (ncols > 0x7fffffffL || n > 0x7fffffffL)
    fatal("[dlaf_mi355x] bt_band_to_tridiagonal: sizes beyond 32-bit tile counts\n");
  BtPhases phase{s};
  BtBlocks<T> k{};
  k.n = n;
  k.b = band;
  k.nblk = sc.nblk;
  k.vblk = (size_t) 2 * band * band;
  k.v = v;
  k.ldv = ldv;
  k.e = e;
  k.lde = lde;
  k.ncols = ncols;
  k.s = s;
  const size_t nb2 = (size_t) k.nblk * k.nblk;
  PoolScope ws, ws_et;  // (E^T has a scope of its own: it goes back behind W2, which is taken after it)
  k.vx = ws.get<T>(nb2 * k.vblk);
  k.wx = ws.get<T>(nb2 * k.vblk);
  k.sm = ws.get<T>(nb2 * (size_t) band * band);
  k.tm = ws.get<T>(nb2 * (size_t) band * band);
  k.taus = ws.get<T>(nb2 * (size_t) band);
  phase("allocations");
  // DLAF_MI355X_BT_FUSED=0: the two strided-batch products per batch (every type, every band)
  static const bool fused_on = env_flag("DLAF_MI355X_BT_FUSED", true);
  k.fused = fused_on && bt_fused_supported(band, sizeof(T), TypeInfo<T>::is_complex);
  bt_prepare_blocks(k, std::min<long>(k.nblk, sc.jb_last() + 1));
  phase("expand, S, T factors, W");
  bt_transpose_in(k, ws_et);
  phase("transposition");
  k.w2 = ws.get<T>((size_t) sc.max_batch() * band * (size_t) ncols);
  bt_apply_wavefronts(k, sc);
  phase("wavefronts");
  bt_transpose_back(k);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  phase("transposition back");
  ws.release();
  ws_et.release();
  phase("frees");
  return 0;
}

template <class T>
int bt_band_to_tridiag_host(long n, int band, const T* v, long ldv, T* e, long lde, long ncols) {
  if (n <= 0 || ncols <= 0)
    return 0;
  ScratchStream s;
  PoolScope ws;
  T* dv = ws.get<T>((size_t) n * n);
  // row 1 of E on a 16-byte boundary, even leading dimension: the row blocks the reflector blocks act on start at the
  // rows 1 + i b, and the k-contiguous operand loader of the general product wants them aligned
  const long ldd = bt_aligned_ld(n);
  T* de = bt_aligned_base(ws.get<T>((size_t) ldd * ncols + 4));
  DLAF_HIP_CHECK(hipMemcpy2DAsync(dv, (size_t) n * sizeof(T), v, (size_t) ldv * sizeof(T), (size_t) n * sizeof(T), (size_t) n,
                                  hipMemcpyHostToDevice, s));
  DLAF_HIP_CHECK(hipMemcpy2DAsync(de, (size_t) ldd * sizeof(T), e, (size_t) lde * sizeof(T), (size_t) n * sizeof(T),
                                  (size_t) ncols, hipMemcpyHostToDevice, s));
  StageTimer timer(s);
  const int r = bt_band_to_tridiag_device(n, band, dv, n, de, ldd, ncols, s);
  g_stage_ms[3] = timer.stop();
  DLAF_HIP_CHECK(hipMemcpy2DAsync(e, (size_t) lde * sizeof(T), de, (size_t) ldd * sizeof(T), (size_t) n * sizeof(T),
                                  (size_t) ncols, hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  return r;
}

// ------------------------------------------------------------------------------------------------ drivers
// the eigenvalue index range of a partial spectrum and the internal eigenvector matrix that holds it (eigensolver.hpp)
void check_eigenvalues_index(const char* who, long n, long begin, long end) {
  if (begin < 0 || begin > end || end > n)
    fatal("[dlaf_mi355x] %s: eigenvalue index range [%ld, %ld) must satisfy 0 <= begin <= end <= n = %ld\n", who, begin,
          end, n);
}

PartialSpectrumPlan partial_spectrum_plan(long n, int nb, int npcol, int mycol, int z_jsrc, long begin, long end) {
  PartialSpectrumPlan p;
  const long t0 = begin / nb;
  p.b0 = t0 * nb;
  p.jsrc = (int) ((z_jsrc + t0) % npcol);
  p.ncl = Axis{end - p.b0, nb, npcol, mycol, p.jsrc}.local_size();
  p.first = Axis{n, nb, npcol, mycol, z_jsrc}.next_local(t0) * nb;
  p.pad = mycol == p.jsrc ? begin - p.b0 : 0;
  return p;
}

// Eigensolver::call on resident operands, in two halves.  The reductions (stages 1-2) turn A (uplo L; destroyed: band
// + reflectors) into the tridiagonal matrix d, e and the reflector matrix v, all resident; the rest (stages 3-5) takes
// them to the eigenvalues (host array w, all n on every rank) and the eigenvectors of the eigenvalues [begin, end) in
// the resident general matrix Z (A's block size and row source), which covers the global columns [b0, end),
// b0 = (begin / nb) nb: n x (end - b0), the full matrix for [0, n).  Its columns [b0, begin) are padding and stay zero
// through both back-transformations (and the triangular solve of the generalized problem): all three act on the
// columns independently.  Between the halves the eigenvalues-only entries stop (bisection on d, e) and the by-value
// entries turn (vl, vu] into an index range (two Sturm counts), which is why Z is made only then.
namespace {
// a stage's status is made the same on every rank before anybody acts on it: a rank that left alone would leave
// the others inside the next collective
int agreed(Grid* g, int info) {
  if (g->nranks > 1 && g->transport) {
    double v[2] = {info > 0 ? (double) info : 0.0, info < 0 ? 1.0 : 0.0};
    g->transport->allreduce_max(v, 2, g->nprow, g->npcol, g->myrow, g->mycol);
    info = v[1] > 0 ? kInfoSchedulingFailure : (int) v[0];
  }
  return info;
}

// stages 2 and 3 run replicated: say what they need instead of failing inside an allocation
void check_replicated_memory(long n, double need) {
  size_t free_b = 0, total_b = 0;
  DLAF_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  // the idle blocks of the workspace pool count as free: the stages take them again, and pool_malloc gives them back to
  // the driver when an allocation fails
  const size_t idle_b = pool_idle_bytes();
  if (need > 0.95 * (double) (free_b + idle_b))
    fatal("[dlaf_mi355x] eigensolver: n = %ld needs %.1f GiB per rank for the replicated stages (band_to_tridiagonal, "
          "tridiagonal_eigensolver), %.1f GiB are free and %.1f GiB idle in the workspace pool\n", n, need / 1073741824.0,
          (double) free_b / 1073741824.0, (double) idle_b / 1073741824.0);
}
// every rank holds the n x n reflector matrix (T) ...
template <class T>
double reflector_bytes(long n) {
  return (double) n * n * sizeof(T);
}
// ... and, behind the reductions, the n x k real eigenvector matrix, the divide & conquer workspaces (4 n^2 real) and
// its columns of the internal eigenvector matrix
template <class T>
double solver_bytes(long n, int nb, int npcol, long begin, long end) {
  using R = real_t<T>;
  const long b0 = (begin / nb) * nb;
  return (double) n * n * 4.0 * sizeof(R) + (double) n * (end - begin) * sizeof(R) +
         (double) (end - b0) * bt_aligned_ld(n) / npcol * sizeof(T);
}

// what the reductions leave resident
template <class T>
struct Reduced {
  std::vector<T> taus;
  int band = 0;
  real_t<T>* d = nullptr;
  real_t<T>* e = nullptr;
  T* v = nullptr;
  PoolScope tridiag, reflectors;  // d, e | v: an eigenvalues-only call gives the reflectors back early
  void release() {
    tridiag.release();
    reflectors.release();
  }
  ~Reduced() { release(); }
};

// stages 1-2: reduction_to_band, band_to_tridiagonal (n > 0); holds nothing when it fails
template <class T>
int eigensolver_reductions(DeviceMatrix<T>& A, Reduced<T>& r) {
  using R = real_t<T>;
  const long n = A.n;
  Grid* g = A.grid;
  hipStream_t s = A.s_high;
  const DebugWho who = eig_debug(g);
  r.band = get_band_size(A.nb);  // eigensolver/impl.h:41
  r.taus.assign((size_t) std::max<long>(0, n - r.band - 1) + 1, T{});
  int info = agreed(g, reduction_to_band_device(A, r.band, r.taus.data()));
  debug_checksum(who, s, "A after red2band", A.tiles, (size_t) A.ltr * A.ltc * A.tile_elems * sizeof(T));
  {
    double ms = 0, fl = 0;
    red2band_last_profile(&ms, &fl);
    g_stage_ms[0] = ms;
  }
  if (info != 0)
    return info;
  r.d = r.tridiag.template get<R>((size_t) n);
  r.e = r.tridiag.template get<R>((size_t) n);
  r.v = r.reflectors.template get<T>((size_t) n * n);
  info = agreed(g, band_to_tridiag_device(A, r.band, r.d, r.e, r.v, n));
  if (info != 0) {
    r.release();
    return info;
  }
  debug_checksum(who, s, "d", r.d, (size_t) n * sizeof(R));
  debug_checksum(who, s, "e", r.e, (size_t) (n - 1) * sizeof(R));
  debug_checksum(who, s, "v", r.v, (size_t) n * n * sizeof(T));
  return 0;
}

// stages 3-5: tridiagonal_eigensolver, bt_band_to_tridiagonal, bt_reduction_to_band; releases what the reductions left
template <class T>
int eigensolver_back(DeviceMatrix<T>& A, Reduced<T>& r, real_t<T>* w_host, GeneralMatrix<T>& Z, long begin, long end) {
  using R = real_t<T>;
  const long n = A.n;
  const int nb = A.nb;
  Grid* g = A.grid;
  TileMatrix<T>& C = Z.m;
  const long b0 = (begin / nb) * nb, pad = begin - b0, k = end - begin;
  if (C.grid != g || C.nb != nb || C.rows.n != n || C.cols.n != end - b0 || C.rows.src != A.rows.src || C.transposed)
    fatal("[dlaf_mi355x] eigensolver: the eigenvector matrix must be n x %ld with A's block size and row source rank\n",
          end - b0);
  hipStream_t s = A.s_high;
  const DebugWho who = eig_debug(g);
  const int band = r.band;
  PoolScope ws, ws_el;
  R* wd = ws.get<R>((size_t) n);
  R* zr = ws.get<R>((size_t) n * k);
  {
    StageTimer t(s);
    tridiag_solver_device<R>(n, nb, r.d, r.e, wd, zr, n, begin, end, s, g->nranks > 1 ? grid_transport(*g) : nullptr);
    g_stage_ms[2] = t.stop();
  }
  debug_checksum(who, s, "w", wd, (size_t) n * sizeof(R));
  debug_checksum(who, s, "z (tridiagonal)", zr, (size_t) n * k * sizeof(R));
  DLAF_HIP_CHECK(hipMemcpyAsync(w_host, wd, (size_t) n * sizeof(R), hipMemcpyDeviceToHost, s));
  if (k == 0) {
    // no eigenvector is wanted: the eigenvalues are all there is
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    g_stage_ms[3] = g_stage_ms[4] = 0;
    return 0;
  }
  // the columns of this process column, all rows (the back-transformation mixes rows, never columns)
  const long ncl = C.cols.local_size();
  const long lde = bt_aligned_ld(n);
  T* el = bt_aligned_base(ws_el.get<T>((size_t) lde * std::max<long>(ncl, 1) + 4));
  launch_cols_gather_cast<R, T>(zr, n, n, nb, C.cols.P, C.cols.shift(), ncl, pad, el, lde, s);
  {
    StageTimer t(s);
    bt_band_to_tridiag_device(n, band, r.v, n, el, lde, ncl, s);
    g_stage_ms[3] = t.stop();
  }
  debug_checksum(who, s, "E after bt_b2t", el, (size_t) lde * std::max<long>(ncl, 1) * sizeof(T));
  launch_rows_to_tiles(el, lde, n, ncl, nb, C.rows.P, C.rows.shift(), C.ltr, C.ltc, C.tiles, s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  // the last stage takes its own workspaces: everything of the earlier ones goes back first
  ws.release();
  r.release();
  ws_el.release();
  debug_checksum(who, s, "C before bt_red2band", C.tiles, (size_t) C.ltr * C.ltc * C.tile_elems * sizeof(T));
  const int info = agreed(g, bt_reduction_to_band_device(band, C, A, r.taus.data()));
  debug_checksum(who, s, "C after bt_red2band", C.tiles, (size_t) C.ltr * C.ltc * C.tile_elems * sizeof(T));
  {
    double ms = 0, fl = 0;
    red2band_last_profile(&ms, &fl);
    g_stage_ms[4] = ms;
  }
  return info;
}

// (vl, vu] -> [begin, end) = [count(vl), count(vu)): two Sturm counts of the computed tridiagonal matrix in one launch,
// made the same on every rank before anybody acts on them (the replicated stages are deterministic, but a rank that
// disagreed would hang the next collective).  vl >= vu: the empty range at count(vl).
template <class T>
void index_range_of_values(Grid* g, long n, const Reduced<T>& r, real_t<T> vl, real_t<T> vu, hipStream_t s, long& begin,
                           long& end) {
  using R = real_t<T>;
  const R shifts[2] = {vl, vu};
  long counts[2] = {0, 0};
  sturm_count_device<R>(n, r.d, r.e, shifts, 2, counts, s);
  if (g->nranks > 1 && g->transport) {
    double v[2] = {(double) counts[0], (double) counts[1]};
    g->transport->allreduce_max(v, 2, g->nprow, g->npcol, g->myrow, g->mycol);
    counts[0] = (long) v[0];
    counts[1] = (long) v[1];
  }
  if (counts[0] < 0)
    fatal("[dlaf_mi355x] eigensolver: the tridiagonal matrix holds a NaN or an Inf: no eigenvalue can be selected by "
          "value\n");
  begin = counts[0];
  end = vl < vu ? std::max(counts[0], counts[1]) : counts[0];
}

// The eigensolver on the resident A: the index range [begin, end) as given, or, with by_value = {vl, vu}, found
// between the two halves and returned.  zh: the internal eigenvector matrix it creates (see partial_spectrum_plan).
template <class T>
int hermitian_eigensolver_device(DeviceMatrix<T>& A, real_t<T>* w_host, int z_isrc, int z_jsrc, const real_t<T>* by_value,
                                 long& begin, long& end, std::unique_ptr<MatrixBase>& zh, PartialSpectrumPlan& pl) {
  const long n = A.n;
  const int nb = A.nb;
  Grid* g = A.grid;
  if (by_value)
    begin = end = 0;
  else
    check_eigenvalues_index("eigensolver", n, begin, end);
  auto make_z = [&] {
    pl = partial_spectrum_plan(n, nb, g->npcol, g->mycol, z_jsrc, begin, end);
    zh.reset(general_matrix_create(g, TypeInfo<T>::tag, n, end - pl.b0, nb, z_isrc, pl.jsrc));
  };
  if (n == 0) {
    make_z();
    return 0;
  }
  check_replicated_memory(n, reflector_bytes<T>(n) + (by_value ? 0.0 : solver_bytes<T>(n, nb, g->npcol, begin, end)));
  Reduced<T> r;
  int info = eigensolver_reductions(A, r);
  if (info != 0) {
    make_z();
    return info;
  }
  if (by_value) {
    index_range_of_values(g, n, r, by_value[0], by_value[1], A.s_high, begin, end);
    check_replicated_memory(n, solver_bytes<T>(n, nb, g->npcol, begin, end));
  }
  make_z();
  return eigensolver_back(A, r, w_host, static_cast<GeneralMatrix<T>&>(*zh), begin, end);
}

// Eigenvalues only, on the resident A: the reductions, then bisection for [begin, end) on the tridiagonal matrix.  No
// divide & conquer, no back-transformation, no eigenvector matrix; w_host[begin, end) is written and nothing else.
template <class T>
int hermitian_eigenvalues_device(DeviceMatrix<T>& A, real_t<T>* w_host, long begin, long end) {
  using R = real_t<T>;
  const long n = A.n;
  check_eigenvalues_index("eigenvalues", n, begin, end);
  if (n == 0)
    return 0;
  hipStream_t s = A.s_high;
  // what is still allocated: the reflector matrix band_to_tridiagonal writes
  check_replicated_memory(n, reflector_bytes<T>(n));
  Reduced<T> r;
  const int info = eigensolver_reductions(A, r);
  if (info != 0)
    return info;
  r.reflectors.release();  // (the bisection needs d and e alone)
  r.v = nullptr;
  g_stage_ms[2] = g_stage_ms[3] = g_stage_ms[4] = 0;
  if (end > begin) {
    PoolScope ws;
    R* wd = ws.get<R>((size_t) n);
    double* work = ws.get<double>(sturm_work_doubles(n));
    StageTimer t(s);
    tridiag_eigenvalues_device<R>(n, r.d, r.e, wd, begin, end, work, s);
    g_stage_ms[2] = t.stop();
    debug_checksum(eig_debug(A.grid), s, "w (bisection)", wd + begin, (size_t) (end - begin) * sizeof(R));
    DLAF_HIP_CHECK(hipMemcpyAsync(w_host + begin, wd + begin, (size_t) (end - begin) * sizeof(R), hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
  }
  return 0;
}
}  // namespace

// the local columns of the internal eigenvector matrix behind its padding -> their place in the caller's local array
// (for the full spectrum: all of them, from column 0).  Nothing else of z is written.
template <class T>
static void download_eigenvectors(GeneralMatrix<T>& Z, const PartialSpectrumPlan& pl, T* z, long ldz) {
  TileMatrix<T>& C = Z.m;
  const long srows = C.rows.local_size(), scols = C.cols.local_size();
  if (srows == 0 || scols <= pl.pad)
    return;
  ScratchStream s;
  if (!C.staging)
    C.staging = dev_alloc<T>((size_t) srows * scols);
  launch_from_tiles(C.layout(C.staging, srows), s);
  DLAF_HIP_CHECK(hipMemcpy2DAsync(z + (size_t) (pl.first + pl.pad) * ldz, (size_t) ldz * sizeof(T),
                                  C.staging + (size_t) pl.pad * srows, (size_t) srows * sizeof(T),
                                  (size_t) srows * sizeof(T), (size_t) (scols - pl.pad), hipMemcpyDeviceToHost, s));
  s.sync();
}

namespace {
void check_uplo(const char* who, char uplo) {
  if (uplo != 'L' && uplo != 'l')
    fatal("[dlaf_mi355x] %s: uplo = %c is not implemented (neither upstream: eigensolver/impl.h:43-45)\n", who, uplo);
}

template <class T>
int eigensolver_host_impl(Grid* g, char uplo, HostOperand<T> a, real_t<T>* w, HostOperand<T> z, const real_t<T>* by_value,
                          long& begin, long& end) {
  if (!by_value)
    check_eigenvalues_index("eigensolver", a.n, begin, end);
  check_uplo("eigensolver", uplo);
  if (z.isrc != a.isrc)
    fatal("[dlaf_mi355x] eigensolver: the eigenvector matrix must share A's row source rank (%d != %d)\n", z.isrc, a.isrc);
  DeviceMatrix<T> A;
  A.create(g, 'L', a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  std::unique_ptr<MatrixBase> zh;
  PartialSpectrumPlan pl;
  const int r = hermitian_eigensolver_device(A, w, z.isrc, z.jsrc, by_value, begin, end, zh, pl);
  A.download(a.p, a.ld, true);  // (upstream leaves the band + reflectors in A as well)
  download_eigenvectors(static_cast<GeneralMatrix<T>&>(*zh), pl, z.p, z.ld);
  return r;
}

// gen_eigensolver/impl.h:33-60: cholesky_factorization(uplo, B) unless the caller passes the factor,
// generalized_to_standard(uplo, A, B); A, B resident on return (info == 0)
template <class T>
int gen_to_std_resident(const char* who, Grid* g, char uplo, HostOperand<const T> a, HostOperand<const T> b, int z_isrc,
                        bool b_factorized, DeviceMatrix<T>& A, DeviceMatrix<T>& B) {
  check_uplo(who, uplo);
  if (a.isrc != b.isrc || a.jsrc != b.jsrc || z_isrc != a.isrc)
    fatal("[dlaf_mi355x] %s: A, B and the eigenvector matrix must share their source rank\n", who);
  A.create(g, 'L', a.n, a.nb, a.isrc, a.jsrc);
  B.create(g, 'L', b.n, b.nb, b.isrc, b.jsrc);
  A.upload(a.p, a.ld);
  B.upload(b.p, b.ld);
  if (!b_factorized) {
    const int info = B.factorize();
    if (info != 0)
      return info;
  }
  return gen_to_std_device(A, B);
}

template <class T>
int gen_eigensolver_host_impl(Grid* g, char uplo, HostOperand<T> a, HostOperand<T> b, real_t<T>* w, HostOperand<T> z,
                              bool b_factorized, const real_t<T>* by_value, long& begin, long& end) {
  if (!by_value)
    check_eigenvalues_index("gen_eigensolver", a.n, begin, end);
  DeviceMatrix<T> A, B;
  int info = gen_to_std_resident<T>("gen_eigensolver", g, uplo, a, b, z.isrc, b_factorized, A, B);
  if (info != 0)
    return info;
  std::unique_ptr<MatrixBase> zh;
  PartialSpectrumPlan pl;
  info = hermitian_eigensolver_device(A, w, z.isrc, z.jsrc, by_value, begin, end, zh, pl);
  if (info != 0)
    return info;
  // triangular_solver(Left, uplo, ConjTrans, NonUnit, 1, B, Z)
  const T one = make_host_el<T>(1.0);
  B.type = TypeInfo<T>::tag;
  if (end > begin)
    info = triangular_solver_device('L', 'L', 'C', 'N', &one, &B, zh.get());
  A.download(a.p, a.ld, true);
  if (!b_factorized)
    B.download(b.p, b.ld, true);
  download_eigenvectors(static_cast<GeneralMatrix<T>&>(*zh), pl, z.p, z.ld);
  return info;
}
}  // namespace

template <class T>
int hermitian_eigensolver_host(Grid* g, char uplo, HostOperand<T> a, real_t<T>* w, HostOperand<T> z, long begin, long end) {
  return eigensolver_host_impl<T>(g, uplo, a, w, z, nullptr, begin, end);
}

template <class T>
int hermitian_eigensolver_by_value_host(Grid* g, char uplo, HostOperand<T> a, real_t<T>* w, HostOperand<T> z, real_t<T> vl,
                                        real_t<T> vu, long* begin, long* end) {
  const real_t<T> by_value[2] = {vl, vu};
  return eigensolver_host_impl<T>(g, uplo, a, w, z, by_value, *begin, *end);
}

template <class T>
int hermitian_gen_eigensolver_host(Grid* g, char uplo, HostOperand<T> a, HostOperand<T> b, real_t<T>* w, HostOperand<T> z,
                                   bool b_factorized, long begin, long end) {
  return gen_eigensolver_host_impl<T>(g, uplo, a, b, w, z, b_factorized, nullptr, begin, end);
}

template <class T>
int hermitian_gen_eigensolver_by_value_host(Grid* g, char uplo, HostOperand<T> a, HostOperand<T> b, real_t<T>* w,
                                            HostOperand<T> z, bool b_factorized, real_t<T> vl, real_t<T> vu, long* begin,
                                            long* end) {
  const real_t<T> by_value[2] = {vl, vu};
  return gen_eigensolver_host_impl<T>(g, uplo, a, b, w, z, b_factorized, by_value, *begin, *end);
}

template <class T>
int hermitian_eigenvalues_host(Grid* g, char uplo, HostOperand<const T> a, real_t<T>* w, long begin, long end) {
  check_eigenvalues_index("eigenvalues", a.n, begin, end);
  check_uplo("eigenvalues", uplo);
  DeviceMatrix<T> A;
  A.create(g, 'L', a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  return hermitian_eigenvalues_device(A, w, begin, end);
}

template <class T>
int hermitian_gen_eigenvalues_host(Grid* g, char uplo, HostOperand<const T> a, HostOperand<T> b, real_t<T>* w,
                                   bool b_factorized, long begin, long end) {
  check_eigenvalues_index("gen_eigenvalues", a.n, begin, end);
  DeviceMatrix<T> A, B;
  int info = gen_to_std_resident<T>("gen_eigenvalues", g, uplo, a, b, a.isrc, b_factorized, A, B);
  if (info != 0)
    return info;
  info = hermitian_eigenvalues_device(A, w, begin, end);
  if (info == 0 && !b_factorized)
    B.download(b.p, b.ld, true);
  return info;
}

template <class T>
int hermitian_eigensolver_resident(DeviceMatrix<T>& A, real_t<T>* w_host, const real_t<T>* by_value, long& begin, long& end,
                                   std::unique_ptr<MatrixBase>& zh, PartialSpectrumPlan& pl) {
  return hermitian_eigensolver_device(A, w_host, A.rows.src, A.cols.src, by_value, begin, end, zh, pl);
}

#define INST(T)                                                                                                          \
  template int hermitian_eigensolver_resident<T>(DeviceMatrix<T>&, real_t<T>*, const real_t<T>*, long&, long&,           \
                                                 std::unique_ptr<MatrixBase>&, PartialSpectrumPlan&);                    \
  template int hermitian_eigensolver_host<T>(Grid*, char, HostOperand<T>, real_t<T>*, HostOperand<T>, long, long);       \
  template int hermitian_gen_eigensolver_host<T>(Grid*, char, HostOperand<T>, HostOperand<T>, real_t<T>*, HostOperand<T>, \
                                                 bool, long, long);                                                      \
  template int hermitian_eigensolver_by_value_host<T>(Grid*, char, HostOperand<T>, real_t<T>*, HostOperand<T>, real_t<T>, \
                                                      real_t<T>, long*, long*);                                          \
  template int hermitian_gen_eigensolver_by_value_host<T>(Grid*, char, HostOperand<T>, HostOperand<T>, real_t<T>*,       \
                                                          HostOperand<T>, bool, real_t<T>, real_t<T>, long*, long*);     \
  template int hermitian_eigenvalues_host<T>(Grid*, char, HostOperand<const T>, real_t<T>*, long, long);                 \
  template int hermitian_gen_eigenvalues_host<T>(Grid*, char, HostOperand<const T>, HostOperand<T>, real_t<T>*, bool,    \
                                                 long, long);                                                            \
  template int band_to_tridiag_device<T>(DeviceMatrix<T>&, int, real_t<T>*, real_t<T>*, T*, long);                       \
  template int band_to_tridiag_host<T>(Grid*, HostOperand<const T>, int, real_t<T>*, real_t<T>*, T*, long);              \
  template int bt_band_to_tridiag_device<T>(long, int, const T*, long, T*, long, long, hipStream_t);                     \
  template int bt_band_to_tridiag_host<T>(long, int, const T*, long, T*, long, long);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
