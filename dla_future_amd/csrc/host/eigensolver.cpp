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
#include "eigensolver.hpp"

namespace dlaf_mi355x {

namespace {
template <class T>
T* ealloc(size_t elems) {
  T* p = nullptr;
  DLAF_HIP_CHECK(pool_malloc(reinterpret_cast<void**>(&p), std::max<size_t>(elems, 1) * sizeof(T)));
  return p;
}
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
  Transport* tr = grid_transport(*grid);
  const bool dist = grid->nranks > 1;
  if (dist && !tr)
    fatal("[dlaf_mi355x] grid with %d ranks has no transport\n", grid->nranks);
  const long n = A.n;
  hipStream_t s = A.s_high;
  DLAF_HIP_CHECK(hipMemsetAsync(A.info, 0, sizeof(int), s));
  if (n == 0)
    return 0;
  StageTimer timer(s);
  T* bandm = ealloc<T>((size_t) (n + 2) * 2 * band);
  // (the two columns of slack behind the matrix are read, never used: they must hold numbers)
  DLAF_HIP_CHECK(hipMemsetAsync(bandm + (size_t) n * 2 * band, 0, (size_t) 2 * 2 * band * sizeof(T), s));
  unsigned* sync = ealloc<unsigned>(b2t_sync_words(n));
  launch_band_extract(A.tiles, A.ltr, A.nb, A.rows.P, A.rows.shift(), A.cols.P, A.cols.shift(), n, band, bandm, s);
  if (dist)
    tr->allreduce_sum(bandm, (size_t) n * 2 * band, TypeInfo<T>::tag, 'A', s);
  DLAF_HIP_CHECK(hipMemset2DAsync(v, (size_t) ldv * sizeof(T), 0, (size_t) n * sizeof(T), (size_t) n, s));
  // the bulge chase works on 2^-k A, max(|Re|, |Im|) in [1, 2): its unscaled sums of squares neither overflow nor
  // underflow whatever the scale of A (every rank holds the same band after the all-reduce and takes the same k)
  unsigned long long* mx = ealloc<unsigned long long>(1);
  launch_band_normalise(bandm, n, band, mx, s);
  launch_band_to_tridiag(bandm, n, band, v, ldv, sync, A.info, s);
  launch_tridiag_extract(bandm, n, band, mx, d, e, s);
  int h_info = 0;
  DLAF_HIP_CHECK(hipMemcpyAsync(&h_info, A.info, sizeof(int), hipMemcpyDeviceToHost, s));
  g_stage_ms[1] = timer.stop();
  DLAF_HIP_CHECK(pool_free(bandm));
  DLAF_HIP_CHECK(pool_free(sync));
  DLAF_HIP_CHECK(pool_free(mx));
  if (h_info == kInfoSchedulingFailure)
    fatal("[dlaf_mi355x] band_to_tridiagonal: a sweep gave up waiting for its predecessor (the workgroup that owns it "
          "made no progress)\n");
  return h_info;
}

template <class T>
int band_to_tridiag_host(Grid* g, const T* a, long lda, long n, int nb, int isrc, int jsrc, int band, real_t<T>* d,
                         real_t<T>* e, T* v, long ldv) {
  using R = real_t<T>;
  DeviceMatrix<T> A;
  A.create(g, 'L', n, nb, isrc, jsrc);
  A.upload(a, lda);
  R* dd = ealloc<R>((size_t) n);
  R* de = ealloc<R>((size_t) n);
  T* dv = ealloc<T>((size_t) n * n);
  const int r = band_to_tridiag_device(A, band, dd, de, dv, n);
  if (n > 0) {
    DLAF_HIP_CHECK(hipMemcpy(d, dd, (size_t) n * sizeof(R), hipMemcpyDeviceToHost));
    DLAF_HIP_CHECK(hipMemcpy(e, de, (size_t) n * sizeof(R), hipMemcpyDeviceToHost));
    DLAF_HIP_CHECK(hipMemcpy2D(v, (size_t) ldv * sizeof(T), dv, (size_t) n * sizeof(T), (size_t) n * sizeof(T), (size_t) n,
                               hipMemcpyDeviceToHost));
  }
  DLAF_HIP_CHECK(pool_free(dd));
  DLAF_HIP_CHECK(pool_free(de));
  DLAF_HIP_CHECK(pool_free(dv));
  return r;
}

// ------------------------------------------------------------------------------------------------ band <- tridiagonal
template <class T>
int bt_band_to_tridiag_device(long n, int band, const T* v, long ldv, T* e, long lde, long ncols, hipStream_t s) {
  const int b = band;
  const long nsweeps = TypeInfo<T>::is_complex ? n - 1 : n - 2;
  if (nsweeps <= 0 || ncols <= 0)
    return 0;
  if (ncols > 0x7fffffffL || n > 0x7fffffffL)
    fatal("[dlaf_mi355x] bt_band_to_tridiagonal: sizes beyond 32-bit tile counts\n");
  const long nblk = (n + b - 1) / b;
  const size_t vblk = (size_t) 2 * b * b;
  const size_t nb2 = (size_t) nblk * nblk;
  // DLAF_MI355X_BT_VERBOSE=1: wall time of the phases of this stage (synchronising: diagnosis only)
  static const bool verbose = [] {
    const char* e = std::getenv("DLAF_MI355X_BT_VERBOSE");
    return e && std::atoi(e) != 0;
  }();
  auto t_last = std::chrono::steady_clock::now();
  auto phase = [&](const char* what) {
    if (!verbose)
      return;
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[dlaf_mi355x] bt_band_to_tridiagonal: %-28s %8.2f ms\n", what,
                 std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  static const bool dbg = [] {
    const char* e_ = std::getenv("DLAF_MI355X_EIG_DEBUG");
    return e_ && std::atoi(e_) != 0;
  }();
  auto checksum = [&](const char* what, const void* dev, size_t bytes) {
    if (!dbg)
      return;
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<unsigned long long> h((bytes + 7) / 8, 0ull);
    DLAF_HIP_CHECK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
    unsigned long long acc = 1469598103934665603ull;
    for (unsigned long long x : h)
      acc = (acc ^ x) * 1099511628211ull;
    std::fprintf(stderr, "[dlaf_mi355x] bt debug %-22s %016llx\n", what, acc);
  };
  T* vx = ealloc<T>(nb2 * vblk);
  T* wx = ealloc<T>(nb2 * vblk);
  T* sm = ealloc<T>(nb2 * (size_t) b * b);
  T* tm = ealloc<T>(nb2 * (size_t) b * b);
  T* taus = ealloc<T>(nb2 * (size_t) b);
  // (no memsets: the expansion writes every block (jb <= ib) in full, zeros included, and nothing reads the others)
  phase("allocations");
  // fp64, band 128: the fused kernel (kernels_bt.hip) applies a block to a column strip in one go, on E transposed, and
  // streams V^T: the expansion writes that image directly (S = V^H V and W = V T take it as their operand);
  // DLAF_MI355X_BT_FUSED=0: the two strided-batch products per wavefront (every type, every band)
  static const bool fused_on = [] {
    const char* e = std::getenv("DLAF_MI355X_BT_FUSED");
    return e ? std::atoi(e) != 0 : true;
  }();
  const bool fused = fused_on && bt_fused_supported(b, sizeof(T), TypeInfo<T>::is_complex);
  launch_b2t_expand(v, ldv, n, b, vx, taus, s, fused);
  const T one = make_host_el<T>(1.0), zero = make_host_el<T>(0.0), mone = make_host_el<T>(-1.0);
  // Block (jb, ib) -- sweep group jb, rows 1 + ib b -- exists for jb <= ib only (ib = jb + step): the strided-batch
  // launches below take one row of the block grid at a time, the blocks ib = jb .. nblk - 1 of sweep group jb, instead
  // of all nblk^2 slots (half of which hold zeros: 28 ms of T factors alone at n = 20480)
  const long jb_end = std::min<long>(nblk, (nsweeps - 1) / b + 1);
  for (long jb = 0; jb < jb_end; ++jb) {
    const size_t q0 = (size_t) jb * nblk + (size_t) jb;
    const int cnt = (int) (nblk - jb);
    {
      GemmArgs<T> g;  // S = V^H V  (fused: vx holds V^T, S = V^T (V^T)^H for the real types of that path)
      g.M = b;
      g.N = b;
      g.K = 2 * b;
      g.a = vx + q0 * vblk;
      g.lda = fused ? b : 2 * b;
      g.opa = fused ? 'N' : 'C';
      g.b = vx + q0 * vblk;
      g.ldb = fused ? b : 2 * b;
      g.opb = fused ? 'C' : 'N';
      g.c = sm + q0 * (size_t) b * b;
      g.ldc = b;
      g.alpha = one;
      g.beta = zero;
      g.batch = cnt;
      g.sa = (long) vblk;
      g.sb = (long) vblk;
      g.sc = (long) b * b;
      launch_gemm(g, s);
    }
    launch_tfactor(sm + q0 * (size_t) b * b, (long) b, taus + q0 * (size_t) b, b, tm + q0 * (size_t) b * b, (long) b, s, cnt,
                   (long) b * b, (long) b, (long) b * b);
    {
      GemmArgs<T> g;  // W = V T
      g.M = 2 * b;
      g.N = b;
      g.K = b;
      g.a = vx + q0 * vblk;
      g.lda = fused ? b : 2 * b;
      g.opa = fused ? 'C' : 'N';
      g.b = tm + q0 * (size_t) b * b;
      g.ldb = b;
      g.opb = 'N';
      g.c = wx + q0 * vblk;
      g.ldc = 2 * b;
      g.alpha = one;
      g.beta = zero;
      g.batch = cnt;
      g.sa = (long) vblk;
      g.sb = (long) b * b;
      g.sc = (long) vblk;
      launch_gemm(g, s);
    }
  }
  if (dbg) {
    // existing blocks only (the others are never written): block row jb, blocks jb .. nblk - 1
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    for (const char* nm : {"vx", "wx", "tm"}) {
      unsigned long long acc = 1469598103934665603ull;
      for (long jb = 0; jb < jb_end; ++jb) {
        const size_t q0 = (size_t) jb * nblk + (size_t) jb, cnt = (size_t) (nblk - jb);
        const bool is_t = nm[0] == 't';
        const size_t per = is_t ? (size_t) b * b : vblk;
        const T* base = (nm[0] == 'v' ? vx : (nm[0] == 'w' ? wx : tm)) + q0 * per;
        std::vector<unsigned long long> h(cnt * per * sizeof(T) / 8);
        DLAF_HIP_CHECK(hipMemcpy(h.data(), base, cnt * per * sizeof(T), hipMemcpyDeviceToHost));
        for (unsigned long long x : h)
          acc = (acc ^ x) * 1099511628211ull;
      }
      std::fprintf(stderr, "[dlaf_mi355x] bt debug %-22s %016llx\n", nm, acc);
    }
  }
  phase("expand, S, T factors, W");
  double* et = nullptr;
  const long ldet = (ncols + 63) / 64 * 64;
  if constexpr (std::is_same_v<T, double>) {
    if (fused) {
      et = ealloc<double>((size_t) ldet * n);
      launch_bt_transpose(e, lde, n, ncols, et, ldet, s);
    }
  }
  if (et)
    checksum("et after transpose", et, (size_t) ldet * n * sizeof(double));
  phase("transposition");
  // steps of sweep group jb (its first sweep has the most)
  auto steps_of = [&](long jb) -> long {
    const long sw = jb * b;
    if (sw >= nsweeps)
      return 0;
    if (TypeInfo<T>::is_complex && sw == n - 2)
      return 1;
    return (n - sw - 2 + b - 1) / b;
  };
  const long jb_last = (nsweeps - 1) / b;
  const long max_batch = nblk / 2 + 2;
  T* w2 = ealloc<T>((size_t) max_batch * b * (size_t) ncols);
  // wavefront t = step - jb, from the last sweep group's first step to the first group's last step
  const long t_lo = -jb_last, t_hi = steps_of(0) - 1;
  for (long t = t_lo; t <= t_hi; ++t) {
    const long jb0 = std::max<long>(0, -t);
    // blocks (jb, st = t + jb), jb = jb0 ...: valid while st < steps_of(jb)
    long cnt = 0, full = 0;
    for (long jb = jb0; jb <= jb_last; ++jb) {
      const long st = t + jb;
      if (st >= steps_of(jb))
        break;
      const long r0 = 1 + (jb + st) * b;
      if (r0 >= n)
        break;
      ++cnt;
      if (r0 + 2 * b <= n)
        ++full;
    }
    if (cnt == 0)
      continue;
    if (cnt > max_batch)
      fatal("[dlaf_mi355x] bt_band_to_tridiagonal: wavefront of %ld blocks exceeds the workspace (%ld)\n", cnt, max_batch);
    // the blocks of a wavefront: block index (jb, ib = 2 jb + t) -> stride nblk + 2 blocks; rows 1 + (2 jb + t) b ->
    // stride 2 b rows of E
    auto run = [&](long first, long count, long rows) {
      if (count <= 0)
        return;
      const long jb = jb0 + first;
      const long ib = 2 * jb + t;
      const long blk = jb * nblk + ib;
      const long r0 = 1 + ib * b;
      if (fused) {
        if constexpr (std::is_same_v<T, double>)
          launch_bt_apply(vx + (size_t) blk * vblk, wx + (size_t) blk * vblk, (long) ((nblk + 2) * (long) vblk), (int) count, et,
                          ldet, ncols, r0, (int) rows, s);
        return;
      }
      GemmArgs<T> g;  // W2 = V^H E
      g.M = b;
      g.N = (int) ncols;
      g.K = (int) rows;
      g.a = vx + (size_t) blk * vblk;
      g.lda = 2 * b;
      g.opa = 'C';
      g.b = e + r0;
      g.ldb = lde;
      g.opb = 'N';
      g.c = w2;
      g.ldc = b;
      g.alpha = one;
      g.beta = zero;
      g.batch = (int) count;
      g.sa = (long) ((nblk + 2) * (long) vblk);
      g.sb = 2L * b;
      g.sc = (long) b * ncols;
      launch_gemm(g, s);
      GemmArgs<T> u;  // E -= W W2
      u.M = (int) rows;
      u.N = (int) ncols;
      u.K = b;
      u.a = wx + (size_t) blk * vblk;
      u.lda = 2 * b;
      u.opa = 'N';
      u.b = w2;
      u.ldb = b;
      u.opb = 'N';
      u.c = e + r0;
      u.ldc = lde;
      u.alpha = mone;
      u.beta = one;
      u.batch = (int) count;
      u.sa = (long) ((nblk + 2) * (long) vblk);
      u.sb = (long) b * ncols;
      u.sc = 2L * b;
      launch_gemm(u, s);
    };
    run(0, full, 2L * b);
    for (long q = full; q < cnt; ++q) {
      const long ib = 2 * (jb0 + q) + t;
      run(q, 1, n - (1 + ib * b));
    }
  }
  if (et)
    checksum("et after wavefronts", et, (size_t) ldet * n * sizeof(double));
  phase("wavefronts");
  if constexpr (std::is_same_v<T, double>) {
    if (fused)
      launch_bt_transpose(et, ldet, ncols, n, e, lde, s);
  }
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  phase("transposition back");
  for (T* q : {vx, wx, sm, tm, taus, w2})
    DLAF_HIP_CHECK(pool_free(q));
  if (et)
    DLAF_HIP_CHECK(pool_free(et));
  phase("frees");
  return 0;
}

template <class T>
int bt_band_to_tridiag_host(long n, int band, const T* v, long ldv, T* e, long lde, long ncols) {
  if (n <= 0 || ncols <= 0)
    return 0;
  hipStream_t s;
  DLAF_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  T* dv = ealloc<T>((size_t) n * n);
  // row 1 of E on a 16-byte boundary, even leading dimension: the row blocks the reflector blocks act on start at the
  // rows 1 + i b, and the k-contiguous operand loader of the general product wants them aligned
  const long ldd = bt_aligned_ld(n);
  T* de_alloc = ealloc<T>((size_t) ldd * ncols + 4);
  T* de = bt_aligned_base(de_alloc);
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
  DLAF_HIP_CHECK(pool_free(dv));
  DLAF_HIP_CHECK(pool_free(de_alloc));
  DLAF_HIP_CHECK(hipStreamDestroy(s));
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

// DLAF_MI355X_EIG_DEBUG=1: a checksum of every stage's output per rank (diagnosis: each stage is deterministic)
void debug_checksum(Grid* g, hipStream_t s, const char* what, const void* dev, size_t bytes) {
  static const bool dbg = [] {
    const char* e_ = std::getenv("DLAF_MI355X_EIG_DEBUG");
    return e_ && std::atoi(e_) != 0;
  }();
  if (!dbg)
    return;
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  std::vector<unsigned long long> h((bytes + 7) / 8, 0ull);
  DLAF_HIP_CHECK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
  unsigned long long acc = 1469598103934665603ull;
  for (unsigned long long x : h)
    acc = (acc ^ x) * 1099511628211ull;
  std::fprintf(stderr, "[dlaf_mi355x] eig debug rank (%d,%d) %-24s %016llx\n", g->myrow, g->mycol, what, acc);
}

// stages 2 and 3 run replicated: say what they need instead of failing inside an allocation
void check_replicated_memory(long n, double need) {
  size_t free_b = 0, total_b = 0;
  DLAF_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (need > 0.95 * (double) free_b)
    fatal("[dlaf_mi355x] eigensolver: n = %ld needs %.1f GiB per rank for the replicated stages (band_to_tridiagonal, "
          "tridiagonal_eigensolver), %.1f GiB are free\n", n, need / 1073741824.0, (double) free_b / 1073741824.0);
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
  Reduced() = default;
  Reduced(const Reduced&) = delete;
  Reduced& operator=(const Reduced&) = delete;
  void release() {
    for (real_t<T>* q : {d, e})
      if (q)
        DLAF_HIP_CHECK(pool_free(q));
    if (v)
      DLAF_HIP_CHECK(pool_free(v));
    d = e = nullptr;
    v = nullptr;
  }
  ~Reduced() { release(); }
};

// stages 1-2: reduction_to_band, band_to_tridiagonal (n > 0)
template <class T>
int eigensolver_reductions(DeviceMatrix<T>& A, Reduced<T>& r) {
  using R = real_t<T>;
  const long n = A.n;
  Grid* g = A.grid;
  hipStream_t s = A.s_high;
  r.band = get_band_size(A.nb);  // eigensolver/impl.h:41
  r.taus.assign((size_t) std::max<long>(0, n - r.band - 1) + 1, T{});
  int info = agreed(g, reduction_to_band_device(A, r.band, r.taus.data()));
  debug_checksum(g, s, "A after red2band", A.tiles, (size_t) A.ltr * A.ltc * A.tile_elems * sizeof(T));
  {
    double ms = 0, fl = 0;
    red2band_last_profile(&ms, &fl);
    g_stage_ms[0] = ms;
  }
  if (info != 0)
    return info;
  r.d = ealloc<R>((size_t) n);
  r.e = ealloc<R>((size_t) n);
  r.v = ealloc<T>((size_t) n * n);
  info = agreed(g, band_to_tridiag_device(A, r.band, r.d, r.e, r.v, n));
  if (info != 0) {
    r.release();
    return info;
  }
  debug_checksum(g, s, "d", r.d, (size_t) n * sizeof(R));
  debug_checksum(g, s, "e", r.e, (size_t) (n - 1) * sizeof(R));
  debug_checksum(g, s, "v", r.v, (size_t) n * n * sizeof(T));
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
  const int band = r.band;
  R* wd = ealloc<R>((size_t) n);
  R* zr = ealloc<R>((size_t) n * k);
  {
    StageTimer t(s);
    tridiag_solver_device<R>(n, nb, r.d, r.e, wd, zr, n, begin, end, s, g->nranks > 1 ? grid_transport(*g) : nullptr);
    g_stage_ms[2] = t.stop();
  }
  debug_checksum(g, s, "w", wd, (size_t) n * sizeof(R));
  debug_checksum(g, s, "z (tridiagonal)", zr, (size_t) n * k * sizeof(R));
  DLAF_HIP_CHECK(hipMemcpyAsync(w_host, wd, (size_t) n * sizeof(R), hipMemcpyDeviceToHost, s));
  if (k == 0) {
    // no eigenvector is wanted: the eigenvalues are all there is
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    for (R* q : {wd, zr})
      DLAF_HIP_CHECK(pool_free(q));
    r.release();
    g_stage_ms[3] = g_stage_ms[4] = 0;
    return 0;
  }
  // the columns of this process column, all rows (the back-transformation mixes rows, never columns)
  const long ncl = C.cols.local_size();
  const long lde = bt_aligned_ld(n);
  T* el_alloc = ealloc<T>((size_t) lde * std::max<long>(ncl, 1) + 4);
  T* el = bt_aligned_base(el_alloc);
  launch_cols_gather_cast<R, T>(zr, n, n, nb, C.cols.P, C.cols.shift(), ncl, pad, el, lde, s);
  {
    StageTimer t(s);
    bt_band_to_tridiag_device(n, band, r.v, n, el, lde, ncl, s);
    g_stage_ms[3] = t.stop();
  }
  debug_checksum(g, s, "E after bt_b2t", el, (size_t) lde * std::max<long>(ncl, 1) * sizeof(T));
  launch_rows_to_tiles(el, lde, n, ncl, nb, C.rows.P, C.rows.shift(), C.ltr, C.ltc, C.tiles, s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  for (R* q : {wd, zr})
    DLAF_HIP_CHECK(pool_free(q));
  r.release();
  DLAF_HIP_CHECK(pool_free(el_alloc));
  debug_checksum(g, s, "C before bt_red2band", C.tiles, (size_t) C.ltr * C.ltc * C.tile_elems * sizeof(T));
  const int info = agreed(g, bt_reduction_to_band_device(band, C, A, r.taus.data()));
  debug_checksum(g, s, "C after bt_red2band", C.tiles, (size_t) C.ltr * C.ltc * C.tile_elems * sizeof(T));
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
  DLAF_HIP_CHECK(pool_free(r.v));
  r.v = nullptr;
  g_stage_ms[2] = g_stage_ms[3] = g_stage_ms[4] = 0;
  if (end > begin) {
    R* wd = ealloc<R>((size_t) n);
    double* work = ealloc<double>(sturm_work_doubles(n));
    StageTimer t(s);
    tridiag_eigenvalues_device<R>(n, r.d, r.e, wd, begin, end, work, s);
    g_stage_ms[2] = t.stop();
    debug_checksum(A.grid, s, "w (bisection)", wd + begin, (size_t) (end - begin) * sizeof(R));
    DLAF_HIP_CHECK(hipMemcpyAsync(w_host + begin, wd + begin, (size_t) (end - begin) * sizeof(R), hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    DLAF_HIP_CHECK(pool_free(wd));
    DLAF_HIP_CHECK(pool_free(work));
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
  hipStream_t s = nullptr;
  DLAF_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  if (!C.staging)
    C.staging = dev_alloc<T>((size_t) srows * scols);
  launch_from_tiles(C.layout(C.staging, srows), s);
  DLAF_HIP_CHECK(hipMemcpy2DAsync(z + (size_t) (pl.first + pl.pad) * ldz, (size_t) ldz * sizeof(T),
                                  C.staging + (size_t) pl.pad * srows, (size_t) srows * sizeof(T),
                                  (size_t) srows * sizeof(T), (size_t) (scols - pl.pad), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  DLAF_HIP_CHECK(hipStreamDestroy(s));
}

namespace {
void check_uplo(const char* who, char uplo) {
  if (uplo != 'L' && uplo != 'l')
    fatal("[dlaf_mi355x] %s: uplo = %c is not implemented (neither upstream: eigensolver/impl.h:43-45)\n", who, uplo);
}

template <class T>
int eigensolver_host_impl(Grid* g, char uplo, T* a, long lda, long n, int nb, int isrc, int jsrc, real_t<T>* w, T* z,
                          long ldz, int z_isrc, int z_jsrc, const real_t<T>* by_value, long& begin, long& end) {
  if (!by_value)
    check_eigenvalues_index("eigensolver", n, begin, end);
  check_uplo("eigensolver", uplo);
  if (z_isrc != isrc)
    fatal("[dlaf_mi355x] eigensolver: the eigenvector matrix must share A's row source rank (%d != %d)\n", z_isrc, isrc);
  DeviceMatrix<T> A;
  A.create(g, 'L', n, nb, isrc, jsrc);
  A.upload(a, lda);
  std::unique_ptr<MatrixBase> zh;
  PartialSpectrumPlan pl;
  const int r = hermitian_eigensolver_device(A, w, z_isrc, z_jsrc, by_value, begin, end, zh, pl);
  A.download(a, lda, true);  // (upstream leaves the band + reflectors in A as well)
  download_eigenvectors(static_cast<GeneralMatrix<T>&>(*zh), pl, z, ldz);
  return r;
}

// gen_eigensolver/impl.h:33-60: cholesky_factorization(uplo, B) unless the caller passes the factor,
// generalized_to_standard(uplo, A, B); A, B resident on return (info == 0)
template <class T>
int gen_to_std_resident(const char* who, Grid* g, char uplo, const T* a, long lda, T* b, long ldb, long n, int nb, int a_isrc,
                        int a_jsrc, int b_isrc, int b_jsrc, int z_isrc, bool b_factorized, DeviceMatrix<T>& A,
                        DeviceMatrix<T>& B) {
  check_uplo(who, uplo);
  if (a_isrc != b_isrc || a_jsrc != b_jsrc || z_isrc != a_isrc)
    fatal("[dlaf_mi355x] %s: A, B and the eigenvector matrix must share their source rank\n", who);
  A.create(g, 'L', n, nb, a_isrc, a_jsrc);
  B.create(g, 'L', n, nb, b_isrc, b_jsrc);
  A.upload(a, lda);
  B.upload(b, ldb);
  if (!b_factorized) {
    const int info = B.factorize();
    if (info != 0)
      return info;
  }
  return gen_to_std_device(A, B);
}

template <class T>
int gen_eigensolver_host_impl(Grid* g, char uplo, T* a, long lda, T* b, long ldb, long n, int nb, int a_isrc, int a_jsrc,
                              int b_isrc, int b_jsrc, real_t<T>* w, T* z, long ldz, int z_isrc, int z_jsrc,
                              bool b_factorized, const real_t<T>* by_value, long& begin, long& end) {
  if (!by_value)
    check_eigenvalues_index("gen_eigensolver", n, begin, end);
  DeviceMatrix<T> A, B;
  int info = gen_to_std_resident("gen_eigensolver", g, uplo, a, lda, b, ldb, n, nb, a_isrc, a_jsrc, b_isrc, b_jsrc, z_isrc,
                                 b_factorized, A, B);
  if (info != 0)
    return info;
  std::unique_ptr<MatrixBase> zh;
  PartialSpectrumPlan pl;
  info = hermitian_eigensolver_device(A, w, z_isrc, z_jsrc, by_value, begin, end, zh, pl);
  if (info != 0)
    return info;
  // triangular_solver(Left, uplo, ConjTrans, NonUnit, 1, B, Z)
  const T one = make_host_el<T>(1.0);
  B.type = TypeInfo<T>::tag;
  if (end > begin)
    info = triangular_solver_device('L', 'L', 'C', 'N', &one, &B, zh.get());
  A.download(a, lda, true);
  if (!b_factorized)
    B.download(b, ldb, true);
  download_eigenvectors(static_cast<GeneralMatrix<T>&>(*zh), pl, z, ldz);
  return info;
}
}  // namespace

template <class T>
int hermitian_eigensolver_host(Grid* g, char uplo, T* a, long lda, long n, int nb, int isrc, int jsrc, real_t<T>* w, T* z,
                               long ldz, int z_isrc, int z_jsrc, long begin, long end) {
  return eigensolver_host_impl<T>(g, uplo, a, lda, n, nb, isrc, jsrc, w, z, ldz, z_isrc, z_jsrc, nullptr, begin, end);
}

template <class T>
int hermitian_eigensolver_by_value_host(Grid* g, char uplo, T* a, long lda, long n, int nb, int isrc, int jsrc,
                                        real_t<T>* w, T* z, long ldz, int z_isrc, int z_jsrc, real_t<T> vl, real_t<T> vu,
                                        long* begin, long* end) {
  const real_t<T> by_value[2] = {vl, vu};
  return eigensolver_host_impl<T>(g, uplo, a, lda, n, nb, isrc, jsrc, w, z, ldz, z_isrc, z_jsrc, by_value, *begin, *end);
}

template <class T>
int hermitian_gen_eigensolver_host(Grid* g, char uplo, T* a, long lda, T* b, long ldb, long n, int nb, int a_isrc,
                                   int a_jsrc, int b_isrc, int b_jsrc, real_t<T>* w, T* z, long ldz, int z_isrc,
                                   int z_jsrc, bool b_factorized, long begin, long end) {
  return gen_eigensolver_host_impl<T>(g, uplo, a, lda, b, ldb, n, nb, a_isrc, a_jsrc, b_isrc, b_jsrc, w, z, ldz, z_isrc,
                                      z_jsrc, b_factorized, nullptr, begin, end);
}

template <class T>
int hermitian_gen_eigensolver_by_value_host(Grid* g, char uplo, T* a, long lda, T* b, long ldb, long n, int nb, int a_isrc,
                                            int a_jsrc, int b_isrc, int b_jsrc, real_t<T>* w, T* z, long ldz, int z_isrc,
                                            int z_jsrc, bool b_factorized, real_t<T> vl, real_t<T> vu, long* begin,
                                            long* end) {
  const real_t<T> by_value[2] = {vl, vu};
  return gen_eigensolver_host_impl<T>(g, uplo, a, lda, b, ldb, n, nb, a_isrc, a_jsrc, b_isrc, b_jsrc, w, z, ldz, z_isrc,
                                      z_jsrc, b_factorized, by_value, *begin, *end);
}

template <class T>
int hermitian_eigenvalues_host(Grid* g, char uplo, const T* a, long lda, long n, int nb, int isrc, int jsrc, real_t<T>* w,
                               long begin, long end) {
  check_eigenvalues_index("eigenvalues", n, begin, end);
  check_uplo("eigenvalues", uplo);
  DeviceMatrix<T> A;
  A.create(g, 'L', n, nb, isrc, jsrc);
  A.upload(a, lda);
  return hermitian_eigenvalues_device(A, w, begin, end);
}

template <class T>
int hermitian_gen_eigenvalues_host(Grid* g, char uplo, const T* a, long lda, T* b, long ldb, long n, int nb, int a_isrc,
                                   int a_jsrc, int b_isrc, int b_jsrc, real_t<T>* w, bool b_factorized, long begin,
                                   long end) {
  check_eigenvalues_index("gen_eigenvalues", n, begin, end);
  DeviceMatrix<T> A, B;
  int info = gen_to_std_resident("gen_eigenvalues", g, uplo, a, lda, b, ldb, n, nb, a_isrc, a_jsrc, b_isrc, b_jsrc, a_isrc,
                                 b_factorized, A, B);
  if (info != 0)
    return info;
  info = hermitian_eigenvalues_device(A, w, begin, end);
  if (info == 0 && !b_factorized)
    B.download(b, ldb, true);
  return info;
}

#define INST(T)                                                                                                          \
  template int hermitian_eigensolver_host<T>(Grid*, char, T*, long, long, int, int, int, real_t<T>*, T*, long, int, int, \
                                             long, long);                                                                \
  template int hermitian_gen_eigensolver_host<T>(Grid*, char, T*, long, T*, long, long, int, int, int, int, int,         \
                                                 real_t<T>*, T*, long, int, int, bool, long, long);                      \
  template int hermitian_eigensolver_by_value_host<T>(Grid*, char, T*, long, long, int, int, int, real_t<T>*, T*, long, \
                                                      int, int, real_t<T>, real_t<T>, long*, long*);                     \
  template int hermitian_gen_eigensolver_by_value_host<T>(Grid*, char, T*, long, T*, long, long, int, int, int, int,     \
                                                          int, real_t<T>*, T*, long, int, int, bool, real_t<T>,          \
                                                          real_t<T>, long*, long*);                                      \
  template int hermitian_eigenvalues_host<T>(Grid*, char, const T*, long, long, int, int, int, real_t<T>*, long, long);  \
  template int hermitian_gen_eigenvalues_host<T>(Grid*, char, const T*, long, T*, long, long, int, int, int, int, int,   \
                                                 real_t<T>*, bool, long, long);                                          \
  template int band_to_tridiag_device<T>(DeviceMatrix<T>&, int, real_t<T>*, real_t<T>*, T*, long);                       \
  template int band_to_tridiag_host<T>(Grid*, const T*, long, long, int, int, int, int, real_t<T>*, real_t<T>*, T*, long); \
  template int bt_band_to_tridiag_device<T>(long, int, const T*, long, T*, long, long, hipStream_t);                     \
  template int bt_band_to_tridiag_host<T>(long, int, const T*, long, T*, long, long);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
