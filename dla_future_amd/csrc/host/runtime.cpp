// runtime.cpp -- fatal() and the initialisation of the device.
#include "runtime.hpp"
#include "pool.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <exception>

namespace dlaf_mi355x {

void fatal(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
  std::fflush(stderr);
  std::terminate();  // same failure mode as DLAF_ASSERT (include/dlaf/common/assert.h:58-77)
}

static bool g_initialized = false;

void runtime_init() {
  if (g_initialized)
    return;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    fatal("[dlaf_mi355x] no HIP device available: this library has no CPU fallback\n");
  // one process per GPU: honour LOCAL_RANK the way torch.distributed launchers export it
  int dev = 0;
  if (const char* lr = std::getenv("LOCAL_RANK"))
    dev = std::atoi(lr) % ndev;
  if (const char* d = std::getenv("DLAF_MI355X_DEVICE"))
    dev = std::atoi(d) % ndev;
  DLAF_HIP_CHECK(hipSetDevice(dev));
  device_kernels_init();
  g_initialized = true;
}

void runtime_finalize() {
  if (!g_initialized)
    return;
  (void) hipDeviceSynchronize();
  pool_release();
  g_initialized = false;
}

bool runtime_initialized() {
  return g_initialized;
}

}  // namespace dlaf_mi355x
