// norm_stream.hip -- the read-rate yardstick of tools/norm_bench.py: a read-only streaming kernel with 16-byte loads and
// one add per element, no structure, over an allocation the caller names.  Built by the tool into tools/norm_stream.so.
#include <hip/hip_runtime.h>

#include <cstddef>

namespace {
constexpr int kThreads = 256, kUnroll = 4;

__global__ __launch_bounds__(kThreads) void stream_read_kernel(const double2* __restrict__ p, size_t n16,
                                                               double* __restrict__ partial) {
  double acc = 0.0;
  const size_t stride = (size_t) gridDim.x * kThreads;
  size_t i = (size_t) blockIdx.x * kThreads + threadIdx.x;
  for (; i + (kUnroll - 1) * stride < n16; i += kUnroll * stride) {
    double2 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      v[u] = p[i + u * stride];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      acc += v[u].x + v[u].y;
  }
  for (; i < n16; i += stride)
    acc += p[i].x + p[i].y;
  // one slot per thread: plain stores, nothing shared
  partial[(size_t) blockIdx.x * kThreads + threadIdx.x] = acc;
}
}  // namespace

// median-free: returns the device time in ms of each of `reps` launches in ms_out (after `warmup` launches); 0 on success
extern "C" int norm_stream_read(const void* p, size_t bytes, int blocks, int warmup, int reps, float* ms_out) {
  double* partial = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&partial), sizeof(double) * (size_t) blocks * kThreads) != hipSuccess)
    return 1;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return 2;
  int rc = 0;
  for (int r = 0; r < warmup + reps && rc == 0; ++r) {
    (void) hipEventRecord(e0, nullptr);
    hipLaunchKernelGGL(stream_read_kernel, dim3((unsigned) blocks), dim3(kThreads), 0, nullptr,
                       static_cast<const double2*>(p), bytes / 16, partial);
    (void) hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) != hipSuccess)
      rc = 3;
    float ms = 0;
    (void) hipEventElapsedTime(&ms, e0, e1);
    if (r >= warmup)
      ms_out[r - warmup] = ms;
  }
  (void) hipEventDestroy(e0);
  (void) hipEventDestroy(e1);
  (void) hipFree(partial);
  return rc;
}
