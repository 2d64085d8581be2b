// eigenvalues.cpp -- eigenvalues of a symmetric tridiagonal matrix by bisection on Sturm counts, and the counts
// themselves (kernels_sturm.hip): what the eigenvalues-only and the by-value entries of the
// Hermitian eigensolver stand on.
//
// Reference: none (the reference library computes eigenvalues with its divide & conquer solver only); LAPACK's dstebz.
#include <algorithm>
#include <vector>

#include "../device/tridiag_api.hpp"
#include "eigensolver.hpp"
#include "pool.hpp"

namespace dlaf_mi355x {

namespace {
static_assert(sizeof(long) == sizeof(long long), "the counts are 64-bit on both sides of the C ABI");
}  // namespace

template <class R>
void tridiag_eigenvalues_device(long n, const R* d, const R* e, R* w, long begin, long end, double* work, hipStream_t s) {
  if (n <= 0 || end <= begin)
    return;
  launch_sturm_prepare<R>(d, e, n, work, s);
  launch_sturm_bisect<R>(work, n, begin, end, w, s);
}

template <class R>
void sturm_count_device(long n, const R* d, const R* e, const R* shifts_host, long nshifts, long* counts_host,
                        hipStream_t s) {
  if (nshifts <= 0)
    return;
  if (n <= 0) {
    std::fill(counts_host, counts_host + nshifts, 0L);
    return;
  }
  PoolScope ws;
  double* work = ws.get<double>(sturm_work_doubles(n));
  R* dsh = ws.get<R>((size_t) nshifts);
  long long* dcn = ws.get<long long>((size_t) nshifts);
  DLAF_HIP_CHECK(hipMemcpyAsync(dsh, shifts_host, (size_t) nshifts * sizeof(R), hipMemcpyHostToDevice, s));
  launch_sturm_prepare<R>(d, e, n, work, s);
  launch_sturm_count<R>(work, n, dsh, nshifts, dcn, s);
  DLAF_HIP_CHECK(hipMemcpyAsync(counts_host, dcn, (size_t) nshifts * sizeof(long long), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
}

template <class R>
void upload_tridiag(PoolScope& ws, long n, const R* d, const R* e, R*& dd, R*& de, hipStream_t s) {
  dd = ws.get<R>((size_t) n);
  de = ws.get<R>((size_t) n);
  DLAF_HIP_CHECK(hipMemsetAsync(de, 0, (size_t) n * sizeof(R), s));
  DLAF_HIP_CHECK(hipMemcpyAsync(dd, d, (size_t) n * sizeof(R), hipMemcpyHostToDevice, s));
  if (n > 1)
    DLAF_HIP_CHECK(hipMemcpyAsync(de, e, (size_t) (n - 1) * sizeof(R), hipMemcpyHostToDevice, s));
}

template <class R>
int tridiag_eigenvalues_host(long n, const R* d, const R* e, R* w, long begin, long end) {
  check_eigenvalues_index("tridiagonal_eigenvalues", n, begin, end);
  if (n <= 0 || end <= begin)
    return 0;
  ScratchStream s;
  PoolScope ws;
  R *dd, *de;
  upload_tridiag(ws, n, d, e, dd, de, s);
  R* dw = ws.get<R>((size_t) n);
  double* work = ws.get<double>(sturm_work_doubles(n));
  tridiag_eigenvalues_device<R>(n, dd, de, dw, begin, end, work, s);
  DLAF_HIP_CHECK(hipMemcpyAsync(w + begin, dw + begin, (size_t) (end - begin) * sizeof(R), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  return 0;
}

template <class R>
int sturm_count_host(long n, const R* d, const R* e, long nshifts, const R* shifts, long* counts) {
  if (n < 0 || nshifts < 0)
    fatal("[dlaf_mi355x] tridiagonal_sturm_count: n = %ld and nshifts = %ld must not be negative\n", n, nshifts);
  if (nshifts == 0)
    return 0;
  if (n == 0) {
    std::fill(counts, counts + nshifts, 0L);
    return 0;
  }
  ScratchStream s;
  PoolScope ws;
  R *dd, *de;
  upload_tridiag(ws, n, d, e, dd, de, s);
  sturm_count_device<R>(n, dd, de, shifts, nshifts, counts, s);
  return 0;
}

#define INST(R)                                                                                                    \
  template void tridiag_eigenvalues_device<R>(long, const R*, const R*, R*, long, long, double*, hipStream_t);     \
  template void sturm_count_device<R>(long, const R*, const R*, const R*, long, long*, hipStream_t);               \
  template void upload_tridiag<R>(PoolScope&, long, const R*, const R*, R*&, R*&, hipStream_t);                    \
  template int tridiag_eigenvalues_host<R>(long, const R*, const R*, R*, long, long);                              \
  template int sturm_count_host<R>(long, const R*, const R*, long, const R*, long*);
INST(float)
INST(double)
#undef INST

}  // namespace dlaf_mi355x
