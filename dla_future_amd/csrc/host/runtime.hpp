// runtime.hpp -- what every host file stands on: fatal() and the HIP error check, initialisation of the device, and the
// type letter of a C-ABI handle.  The owners of everything else have headers of their own: pool.hpp (workspaces),
// transport.hpp (grid + broadcasts), device_matrix.hpp (the tile-layout matrix and its executor), drivers.hpp (the
// algorithms on top), direct.hpp (kernel test entries).
#pragma once
#include <hip/hip_runtime.h>

#include "../device/device_api.hpp"

namespace dlaf_mi355x {

[[noreturn]] void fatal(const char* fmt, ...);

#define DLAF_HIP_CHECK(expr)                                                                     \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      ::dlaf_mi355x::fatal("[dlaf_mi355x] HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, \
                           __LINE__, #expr);                                                     \
  } while (0)

void runtime_init();
void runtime_finalize();
bool runtime_initialized();

// what a C-ABI matrix handle points to
struct MatrixBase {
  virtual ~MatrixBase() = default;
  char type = 'd';
};

// f((T*) nullptr) with T the element type the letter names (s, d, c, z); bad() for any other letter
template <class F, class Bad>
auto dispatch_type(char type, F&& f, Bad&& bad) -> decltype(f((float*) nullptr)) {
  switch (type) {
    case 's': return f((float*) nullptr);
    case 'd': return f((double*) nullptr);
    case 'c': return f((cfloat*) nullptr);
    case 'z': return f((cdouble*) nullptr);
    default: return bad();
  }
}
// the same for the type letter of a handle, where any other letter is a broken handle
template <class F>
auto dispatch_type(char type, F&& f) -> decltype(f((float*) nullptr)) {
  return dispatch_type(type, f, []() -> decltype(f((float*) nullptr)) { fatal("[dlaf_mi355x] bad matrix type\n"); });
}

}  // namespace dlaf_mi355x
