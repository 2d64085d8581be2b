// c_api_internal.hpp -- what the three files of the extern "C" surface share: the grid registry's accessors (the
// registry itself is private to c_api.cpp), the argument checks, the host-to-device element type map, and host_operand,
// which makes a driver's operand from a caller's pointer and descriptor.
//   c_api.cpp         grid registry, dlaf_initialize / dlaf_finalize, grid entries, MPI shim forwarders, dlaf_c Cholesky
//   c_api_host.cpp    descriptor and ScaLAPACK entries on host memory
//   c_api_device.cpp  device-resident handles, profiles, direct kernel hooks
#pragma once
#include <complex>

#include "api_checks.hpp"
#include "runtime.hpp"
#include "transport.hpp"

namespace dlaf_mi355x {

#pragma GCC visibility push(hidden)  // between the three files only: not exported
Grid* find_grid(int ctx);          // nullptr for a context that names no grid
Grid& grid_from_context(int ctx);  // terminates like upstream (src/c_api/utils.cpp:55-68)
#pragma GCC visibility pop

template <class T>
struct DevType {
  using type = T;
};
template <>
struct DevType<std::complex<float>> {
  using type = cfloat;
};
template <>
struct DevType<std::complex<double>> {
  using type = cdouble;
};
// The one place a caller's pointer and descriptor become a driver's operand (host_operand.hpp): HT is the API's element
// type, const-qualified for a matrix that is only read; the operand points to the device element type.
template <class HT>
auto host_operand(HT* p, const DLAF_descriptor& d) {
  using DT = typename DevType<std::remove_const_t<HT>>::type;
  using PT = std::conditional_t<std::is_const_v<HT>, const DT, DT>;
  return HostOperand<PT>(operand_desc(d), reinterpret_cast<PT*>(p), d.ld);
}

template <class HT>
struct RealOf {
  using type = HT;
};
template <class R>
struct RealOf<std::complex<R>> {
  using type = R;
};

}  // namespace dlaf_mi355x
