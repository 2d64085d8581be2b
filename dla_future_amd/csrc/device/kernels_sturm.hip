// kernels_sturm.hip -- Sturm counts and bisection on a symmetric tridiagonal matrix: the
// eigenvalues [begin, end) of T = tridiag(e, d, e) in O(n (end - begin)) work and O(n) memory, and the number of
// eigenvalues <= sigma for an array of shifts.  No eigenvector, no n^2 workspace, no divide & conquer.
//
// Reference: the reference library has no such stage (its eigenvalues come out of the divide & conquer solver only);
// the algorithm is LAPACK's dstebz / dlaebz (Kahan 1966): the pivots of the LDL^T factorization of T - sigma I,
//   q_0 = d_0 - sigma,   q_i = (d_i - sigma) - e_{i-1}^2 / q_{i-1},
// guarded by |q| < pivmin -> q = -pivmin; the number of pivots q <= pivmin is the number of eigenvalues <= sigma.
//
// Three kernels.  prepare (one workgroup): T -> 2^-k T with max(|d|, |e|) in [1, 2) (exact), written as DOUBLE pairs
// (d_i, e_{i-1}^2), the widened Gershgorin interval, pivmin, a flag for NaN / Inf and the iteration cap.  count: one
// thread per shift.  bisect: one thread per wanted eigenvalue index.  Every thread evaluates the same deterministic
// function count(sigma) in IEEE double arithmetic (true division, no contraction): count is then monotone enough for
// the computed eigenvalues to come out ascending, and a range call returns the bits of the full call.
//
// Operand staging: all lanes of a wave walk the same i, so the pairs go through LDS in chunks of kSturmChunk and every
// lane reads the same 16-byte address (a broadcast read, no bank conflict); the next chunk's global loads are in
// flight under the current chunk's division chain.  One wave per workgroup: the chain is bound by the latency of the
// dependent fp64 divisions, not by throughput, so the waves want to be spread over as many SIMDs as there are.
#include <cfloat>
#include <cmath>

#include "tridiag_api.hpp"

namespace dlaf_mi355x {

namespace {
constexpr int kPrepThreads = 1024;
constexpr int kPairsPerLane = kSturmChunk / kSturmThreads;
static_assert(kSturmChunk % kSturmThreads == 0, "a chunk is loaded in whole rounds of the workgroup");
// dstebz: FUDGE = 2.1; ulp of the arithmetic the recurrence runs in (double, whatever the type of d and e)
constexpr double kFudge = 2.1;
constexpr double kUlp = DBL_EPSILON;

// ---------------------------------------------------------------------------------------------- preparation
__device__ inline double block_max(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int s = kPrepThreads / 2; s > 0; s >>= 1) {
    if (t < s)
      sh[t] = fmax(sh[t], sh[t + s]);
    __syncthreads();
  }
  return sh[0];
}

template <class R>
__global__ __launch_bounds__(kPrepThreads) void sturm_prepare_kernel(const R* __restrict__ d, const R* __restrict__ e,
                                                                     long n, double* __restrict__ prm,
                                                                     double2* __restrict__ de) {
#pragma clang fp contract(off)
  __shared__ double sh[kPrepThreads];
  const int t = threadIdx.x;
  double mx = 0.0, bad = 0.0;
  for (long i = t; i < n; i += kPrepThreads) {
    const double x = (double) d[i];
    const double y = i + 1 < n ? (double) e[i] : 0.0;
    if (!isfinite(x) || !isfinite(y))
      bad = 1.0;
    else
      mx = fmax(mx, fmax(fabs(x), fabs(y)));
  }
  mx = block_max(mx, sh);
  bad = block_max(bad, sh);
  const int k = (bad != 0.0 || mx == 0.0) ? 0 : ilogb(mx);
  double gl = DBL_MAX, gu = -DBL_MAX, e2max = 0.0;
  for (long i = t; i < n; i += kPrepThreads) {
    const double ds = ldexp((double) d[i], -k);
    const double el = i > 0 ? ldexp((double) e[i - 1], -k) : 0.0;
    const double er = i + 1 < n ? ldexp((double) e[i], -k) : 0.0;
    const double e2 = el * el;
    de[i] = make_double2(ds, e2);
    const double r = fabs(el) + fabs(er);
    gl = fmin(gl, ds - r);
    gu = fmax(gu, ds + r);
    e2max = fmax(e2max, e2);
  }
  gl = -block_max(-gl, sh);
  gu = block_max(gu, sh);
  e2max = block_max(e2max, sh);
  if (t == 0) {
    const double pivmin = DBL_MIN * fmax(1.0, e2max);
    const double tnorm = fmax(fabs(gl), fabs(gu));
    const double t1 = kFudge * tnorm;
    const double t2 = t1 * kUlp;
    const double t3 = t2 * (double) n;
    const double t4 = (2.0 * kFudge) * pivmin;
    const double wd = t3 + t4;
    gl = gl - wd;
    gu = gu + wd;
    // halvings from the widened interval down to pivmin, and room for the last split: a NaN shift or a degenerate
    // interval ends there
    int cap = ilogb(gu - gl) - ilogb(pivmin) + 3;
    cap = cap < 1 ? 1 : (cap > kSturmMaxIterations ? kSturmMaxIterations : cap);
    prm[kSturmGl] = gl;
    prm[kSturmGu] = gu;
    prm[kSturmPivmin] = pivmin;
    prm[kSturmK] = (double) k;
    prm[kSturmBad] = bad;
    prm[kSturmCap] = bad != 0.0 ? 0.0 : (double) cap;
  }
}

// ---------------------------------------------------------------------------------------------- count
// count(sigma) of the scaled matrix, sigma per lane; called by every thread of the workgroup together (barriers
// inside).  sh: 2 * kSturmChunk pairs.
__device__ inline int sturm_count(const double2* __restrict__ de, long n, double sigma, double pivmin, double2* sh) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  double2 nxt[kPairsPerLane];
  auto fetch = [&](long base) {
#pragma unroll
    for (int r = 0; r < kPairsPerLane; ++r) {
      const long i = base + r * kSturmThreads + t;
      nxt[r] = i < n ? de[i] : make_double2(0.0, 0.0);
    }
  };
  auto stash = [&](double2* buf) {
#pragma unroll
    for (int r = 0; r < kPairsPerLane; ++r)
      buf[r * kSturmThreads + t] = nxt[r];
  };
  fetch(0);
  __syncthreads();  // (the previous call's readers are done with the buffers)
  stash(sh);
  __syncthreads();
  double q = 1.0;  // e_{-1}^2 = 0: q_0 = (d_0 - sigma) - 0 / 1
  int cnt = 0, cur = 0;
  for (long base = 0; base < n; base += kSturmChunk) {
    const bool more = base + kSturmChunk < n;
    if (more)
      fetch(base + kSturmChunk);
    const double2* buf = sh + cur * kSturmChunk;
    const int len = (int) (n - base < kSturmChunk ? n - base : kSturmChunk);
#pragma unroll 8
    for (int i = 0; i < len; ++i) {
      const double2 p = buf[i];
      const double tmp = p.x - sigma;
      q = tmp - p.y / q;
      if (fabs(q) < pivmin)
        q = -pivmin;
      cnt += q <= pivmin ? 1 : 0;
    }
    if (more) {
      stash(sh + (cur ^ 1) * kSturmChunk);
      __syncthreads();
      cur ^= 1;
    }
  }
  return cnt;
}

template <class R>
__global__ __launch_bounds__(kSturmThreads) void sturm_count_kernel(const double2* __restrict__ de,
                                                                    const double* __restrict__ prm, long n,
                                                                    const R* __restrict__ shifts, long nshifts,
                                                                    long long* __restrict__ counts) {
  __shared__ double2 sh[2 * kSturmChunk];
  const long s = (long) blockIdx.x * kSturmThreads + threadIdx.x;
  const bool bad = prm[kSturmBad] != 0.0;
  if (bad) {
    if (s < nshifts)
      counts[s] = -1;
    return;
  }
  const int k = (int) prm[kSturmK];
  const double sigma = s < nshifts ? ldexp((double) shifts[s], -k) : 0.0;
  const int c = sturm_count(de, n, sigma, prm[kSturmPivmin], sh);
  if (s < nshifts)
    counts[s] = c;
}

// ---------------------------------------------------------------------------------------------- bisection
template <class R>
__global__ __launch_bounds__(kSturmThreads) void sturm_bisect_kernel(const double2* __restrict__ de,
                                                                     const double* __restrict__ prm, long n, long begin,
                                                                     long end, R* __restrict__ w) {
#pragma clang fp contract(off)
  __shared__ double2 sh[2 * kSturmChunk];
  const long j = begin + (long) blockIdx.x * kSturmThreads + threadIdx.x;
  const bool wanted = j < end;
  if (prm[kSturmBad] != 0.0) {
    if (wanted)
      w[j] = (R) NAN;
    return;
  }
  const double pivmin = prm[kSturmPivmin];
  const int k = (int) prm[kSturmK];
  const int cap = (int) prm[kSturmCap];
  double lo = prm[kSturmGl], hi = prm[kSturmGu];
  bool active = wanted;
  double mid = lo + (hi - lo) * 0.5;
  for (int it = 0; it < cap; ++it) {
    if (active) {
      const double tol = fmax(pivmin, (2.0 * kUlp) * fmax(fabs(lo), fabs(hi)));
      if (mid == lo || mid == hi || hi - lo <= tol)
        active = false;
    }
    if (!__syncthreads_or(active ? 1 : 0))
      break;
    const int c = sturm_count(de, n, mid, pivmin, sh);
    if (active) {
      if (c > j)
        hi = mid;
      else
        lo = mid;
      mid = lo + (hi - lo) * 0.5;
    }
  }
  if (wanted)
    w[j] = (R) ldexp(mid, k);
}
}  // namespace

// ---------------------------------------------------------------------------------------------- launchers
template <class R>
void launch_sturm_prepare(const R* d, const R* e, long n, double* work, hipStream_t stream) {
  if (n <= 0)
    return;
  hipLaunchKernelGGL((sturm_prepare_kernel<R>), dim3(1), dim3(kPrepThreads), 0, stream, d, e, n, work,
                     reinterpret_cast<double2*>(work + kSturmHeader));
}

template <class R>
void launch_sturm_count(const double* work, long n, const R* shifts, long nshifts, long long* counts,
                        hipStream_t stream) {
  if (n <= 0 || nshifts <= 0)
    return;
  const unsigned g = (unsigned) ((nshifts + kSturmThreads - 1) / kSturmThreads);
  hipLaunchKernelGGL((sturm_count_kernel<R>), dim3(g), dim3(kSturmThreads), 0, stream,
                     reinterpret_cast<const double2*>(work + kSturmHeader), work, n, shifts, nshifts, counts);
}

template <class R>
void launch_sturm_bisect(const double* work, long n, long begin, long end, R* w, hipStream_t stream) {
  if (n <= 0 || end <= begin)
    return;
  const unsigned g = (unsigned) ((end - begin + kSturmThreads - 1) / kSturmThreads);
  hipLaunchKernelGGL((sturm_bisect_kernel<R>), dim3(g), dim3(kSturmThreads), 0, stream,
                     reinterpret_cast<const double2*>(work + kSturmHeader), work, n, begin, end, w);
}

#define INST(R)                                                                                           \
  template void launch_sturm_prepare<R>(const R*, const R*, long, double*, hipStream_t);                   \
  template void launch_sturm_count<R>(const double*, long, const R*, long, long long*, hipStream_t);       \
  template void launch_sturm_bisect<R>(const double*, long, long, long, R*, hipStream_t);
INST(float)
INST(double)
#undef INST

}  // namespace dlaf_mi355x
