// c_api_internal.hpp -- what the three files of the extern "C" surface share: the grid registry's accessors (the
// registry itself is private to c_api.cpp), the argument checks, the host-to-device element type map, and host_operand,
// which makes a driver's operand from a caller's pointer and descriptor.
//   c_api.cpp         grid registry, dlaf_initialize / dlaf_finalize, grid entries, MPI shim forwarders, dlaf_c Cholesky
//   c_api_host.cpp    descriptor and ScaLAPACK entries on host memory
//   c_api_device.cpp  device-resident handles, profiles, direct kernel hooks
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <limits>

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

// ---- functions of a Hermitian matrix (matrix_function.cpp), shared by the host and the resident entries ----
// the caller's typed weights callback behind the driver's untyped one
template <class R>
struct SpectralWeightsCall {
  void (*fn)(long, const R*, long, long, R*, void*);
  void* user;
  static void call(long n, const void* w, long begin, long end, void* g, void* self) {
    auto* c = static_cast<SpectralWeightsCall*>(self);
    c->fn(n, static_cast<const R*>(w), begin, end, static_cast<R*>(g), c->user);
  }
};
// hermitian_power's weights: lambda^exponent, evaluated in double
template <class R>
struct SpectralPower {
  double exponent;
  static void call(long, const void* w, long begin, long end, void* g, void* self) {
    const double e = static_cast<SpectralPower*>(self)->exponent;
    for (long j = begin; j < end; ++j)
      static_cast<R*>(g)[j] = (R) std::pow((double) static_cast<const R*>(w)[j], e);
  }
};
// The selection of an entry: index_range {begin, end} or value_interval {vl, vu} (both null: all n; both given is
// refused by require_hermitian_function).  Infinite ends of the interval become the largest finite value of R, which
// no eigenvalue exceeds: the Sturm count takes finite shifts.
template <class R>
struct SpectralSelection {
  bool by_value = false;
  R values[2] = {0, 0};
  long begin = 0, end = 0;
  SpectralSelection(long n, const long* index_range, const R* value_interval) {
    by_value = value_interval != nullptr;
    end = n;
    if (by_value) {
      const R big = std::numeric_limits<R>::max();
      values[0] = std::max(-big, std::min(big, value_interval[0]));
      values[1] = std::max(-big, std::min(big, value_interval[1]));
    }
    else if (index_range) {
      begin = index_range[0];
      end = index_range[1];
    }
  }
};

}  // namespace dlaf_mi355x
