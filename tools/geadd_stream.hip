// geadd_stream.hip -- the yardstick of tools/geadd_bench.py: a structure-free streaming copy with 16-byte loads and stores
// between two allocations the caller names.  Built by the tool into tools/geadd_stream.so.
#include <hip/hip_runtime.h>

#include <cstddef>

namespace {
constexpr int kThreads = 256, kUnroll = 4;

__global__ __launch_bounds__(kThreads) void stream_copy_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src,
                                                               size_t n16) {
  const size_t stride = (size_t) gridDim.x * kThreads;
  size_t i = (size_t) blockIdx.x * kThreads + threadIdx.x;
  for (; i + (kUnroll - 1) * stride < n16; i += kUnroll * stride) {
    uint4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      v[u] = src[i + u * stride];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      dst[i + u * stride] = v[u];
  }
  for (; i < n16; i += stride)
    dst[i] = src[i];
}
}  // namespace

// the device time in ms of each of `reps` launches in ms_out (after `warmup` launches); 0 on success
extern "C" int geadd_stream_copy(void* dst, const void* src, size_t bytes, int blocks, int warmup, int reps, float* ms_out) {
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return 2;
  int rc = 0;
  for (int r = 0; r < warmup + reps && rc == 0; ++r) {
    (void) hipEventRecord(e0, nullptr);
    hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned) blocks), dim3(kThreads), 0, nullptr, static_cast<uint4*>(dst),
                       static_cast<const uint4*>(src), bytes / 16);
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
  return rc;
}
