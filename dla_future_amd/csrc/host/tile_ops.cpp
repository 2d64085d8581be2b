// tile_ops.cpp -- single-tile operations with host operands (dlaf_mi355x_tile_*): the tests of the tile kernels
// through the C ABI.  The kernels see every operand in "device orientation": as it is for uplo L, transposed for uplo U
// (the factorization of the upper triangle runs as the lower one of the transposed view).
#include <algorithm>

#include "device_matrix.hpp"
#include "direct.hpp"
#include "launch_args.hpp"
#include "pool.hpp"

namespace dlaf_mi355x {

namespace {
// A host array (rows x cols) and its image on the device in device orientation (transposed when tr), leading
// dimension ld.  An image larger than the array (ld, image_cols) is padded with zeros.
template <class T>
struct Staged {
  int rows, cols;  // of the host array
  bool tr;
  int ld;
  DevBuf<T> raw, dev;  // the caller's image (ld rows), the device orientation
  Staged(int rows_, int cols_, bool tr_, hipStream_t s, int ld_ = 0, int image_cols = 0)
      : rows(rows_), cols(cols_), tr(tr_), ld(std::max(ld_, tr_ ? cols_ : rows_)), raw((size_t) rows_ * cols_) {
    const int irows = tr ? cols : rows, icols = std::max(image_cols, tr ? rows : cols);
    dev.alloc((size_t) ld * icols);
    if (ld > irows || image_cols > 0)
      DLAF_HIP_CHECK(hipMemsetAsync(dev.p, 0, (size_t) ld * icols * sizeof(T), s));
  }
  void upload(const T* host, int ldh, hipStream_t s) {
    if (rows == 0 || cols == 0)
      return;
    DLAF_HIP_CHECK(hipMemcpy2DAsync(raw.p, (size_t) rows * sizeof(T), host, (size_t) ldh * sizeof(T),
                                    (size_t) rows * sizeof(T), (size_t) cols, hipMemcpyHostToDevice, s));
    launch_copy2d(dev.p, (long) ld, raw.p, (long) rows, tr ? cols : rows, tr ? rows : cols, tr ? 1 : 0, 0, s);
  }
  // mask (of the host array): 0 all of it, 1 its lower, 2 its upper triangle -- the rest of the array keeps what
  // upload() read
  void download(T* host, int ldh, int mask, hipStream_t s) {
    if (rows == 0 || cols == 0)
      return;
    launch_copy2d(raw.p, (long) rows, dev.p, (long) ld, rows, cols, tr ? 1 : 0, mask, s);
    DLAF_HIP_CHECK(hipMemcpy2DAsync(host, (size_t) ldh * sizeof(T), raw.p, (size_t) rows * sizeof(T),
                                    (size_t) rows * sizeof(T), (size_t) cols, hipMemcpyDeviceToHost, s));
  }
};
}  // namespace

template <class T>
int tile_potrf(char uplo, int n, T* a, int lda) {
  runtime_init();
  if (n == 0)
    return 0;
  const bool tr = (uplo == 'U' || uplo == 'u');
  hipStream_t s = nullptr;
  Staged<T> da(n, n, tr, s);
  DevBuf<T> w((size_t) ((n + kDiagBlock - 1) / kDiagBlock) * kDiagBlock * kDiagBlock);
  DevBuf<int> info(1);
  DevBuf<unsigned> sync(potrf_coop_sync_words(n));
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  DLAF_HIP_CHECK(hipMemsetAsync(sync.p, 0, sizeof(unsigned) * potrf_coop_sync_words(n), s));
  da.upload(a, lda, s);
  potrf_tile(da.dev.p, n, n, w.p, info.p, 0, sync.p, s);
  da.download(a, lda, tr ? 2 : 1, s);
  int h = 0;
  DLAF_HIP_CHECK(hipMemcpyAsync(&h, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  if (h == kInfoSchedulingFailure)
    fatal("[dlaf_mi355x] cooperative POTRF: a bounded inter-workgroup wait expired; the result is invalid\n");
  return h;
}

// uplo L: B(m x n) <- B A^-H, A n x n lower.   uplo U: B(m x n) <- A^-H B, A m x m upper.
// (the two variants the factorization issues: cholesky/impl.h:56-67 and :110-121)
template <class T>
void tile_trsm(char uplo, int m, int n, const T* a, int lda, T* b, int ldb) {
  runtime_init();
  if (m == 0 || n == 0)
    return;
  const bool tr = (uplo == 'U' || uplo == 'u');
  const int na = tr ? m : n;             // order of the triangular matrix
  const int br = tr ? n : m, bc = na;    // device-orientation extents of B
  hipStream_t s = nullptr;
  const size_t wel = (size_t) ((na + kDiagBlock - 1) / kDiagBlock) * kDiagBlock * kDiagBlock;
  Staged<T> da(na, na, tr, s), db(m, n, tr, s);
  DevBuf<T> w(wel);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  da.upload(a, lda, s);
  db.upload(b, ldb, s);
  // inverted diagonal blocks of the (already triangular) factor: invert-only mode of the diag kernel
  for (int j0 = 0; j0 < na; j0 += kDiagBlock) {
    const int jb = std::min(kDiagBlock, na - j0);
    launch_potrf_diag(da.dev.p + j0 + (size_t) j0 * na, na, jb, w.p + (size_t) (j0 / kDiagBlock) * kDiagBlock * kDiagBlock,
                      info.p, 0, s, false);
  }
  TrsmArgs<T> ta = tile_batch_args<TrsmArgs<T>>(db.dev.p, 0, br, 1, br, (const T*) da.dev.p, na, bc);
  ta.winv = w.p;
  ta.info = info.p;
  launch_trsm(ta, s);
  db.download(b, ldb, 0, s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
}

// uplo L: lower(C) -= A A^H, A n x k.   uplo U: upper(C) -= A^H A, A k x n.   (impl.h:70-80, :124-134)
template <class T>
void tile_herk(char uplo, int n, int k, const T* a, int lda, T* c, int ldc) {
  runtime_init();
  if (n == 0)
    return;
  const bool tr = (uplo == 'U' || uplo == 'u');
  hipStream_t s = nullptr;
  Staged<T> da(tr ? k : n, tr ? n : k, tr, s), dc(n, n, tr, s);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  da.upload(a, lda, s);
  dc.upload(c, ldc, s);
  launch_update(single_tile_update_args<T>(dc.dev.p, da.dev.p, da.dev.p, n, k, false, info.p), s, 2);
  dc.download(c, ldc, tr ? 2 : 1, s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
}

// uplo L: C(m x n) -= A B^H, A m x k, B n x k.   uplo U: C -= A^H B, A k x m, B k x n.
// (impl.h:83-94, :137-147)
template <class T>
void tile_gemm(char uplo, int m, int n, int k, const T* a, int lda, const T* b, int ldb, T* c, int ldc) {
  runtime_init();
  if (m == 0 || n == 0)
    return;
  const bool tr = (uplo == 'U' || uplo == 'u');
  hipStream_t s = nullptr;
  // device orientation: C' = C (L) or C^T (U), extents cm x cn; row operand A' (cm x k), column
  // operand B' (cn x k).  For U:  C^T -= B^T conj(A) = B' A'^H with B' = B^T as ROW operand.
  // The update kernel works on square tiles: the single tile is padded to sq x sq with zero rows.
  const int sq = std::max(m, n), kk = std::max(k, 1);
  Staged<T> row_op(tr ? k : m, tr ? n : k, tr, s, sq, kk), col_op(tr ? k : n, tr ? m : k, tr, s, sq, kk);
  Staged<T> dc(m, n, tr, s, sq, sq);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  row_op.upload(tr ? b : a, tr ? ldb : lda, s);
  col_op.upload(tr ? a : b, tr ? lda : ldb, s);
  dc.upload(c, ldc, s);
  // a tile strictly below the diagonal: plain gemm
  launch_update(single_tile_update_args<T>(dc.dev.p, row_op.dev.p, col_op.dev.p, sq, k, true, info.p), s, 2);
  dc.download(c, ldc, 0, s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
}

#define INST(T)                                                                                     \
  template int tile_potrf<T>(char, int, T*, int);                                                   \
  template void tile_trsm<T>(char, int, int, const T*, int, T*, int);                               \
  template void tile_herk<T>(char, int, int, const T*, int, T*, int);                               \
  template void tile_gemm<T>(char, int, int, int, const T*, int, const T*, int, T*, int);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
