// trsm_path.hpp -- which kernel a panel TRSM launch runs (launch_trsm, kernels_trsm.hip), decided on the host from the
// launch's arguments alone.  Plain C++ and nothing from HIP, so that a host program can sweep the decision over every
// argument set (tests/trsm_path/sweep.cpp).  `Args` is TrsmArgs<T> (device_api.hpp) or anything with its fields b b_ts
// ldb l ldl winv nb last_rows n upper.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace dlaf_mi355x {

enum class TrsmPath : int {
  strips = 0,     // trsm_kernel<T, VEC, UPPER>: 128-row strips, every type, every shape
  rows256 = 1,    // trsm_rows_kernel<256, 2>: fp64, 256-column macro blocks
  rows128 = 2,    // trsm_rows_kernel<128, 2>: fp64, widths that are whole 128s but not whole 256s
  rows_z128 = 3,  // trsm_rows_z_kernel<128, 3>: complex double
};

struct TrsmChoice {
  TrsmPath path;
  bool vec;  // strips only: the 16-byte loaders (VEC) may be used
};

// tuning knob DLAF_MI355X_TRSM=strips selects the strips kernel everywhere (A/B runs, fallback); read once per process
inline bool trsm_rows_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("DLAF_MI355X_TRSM");
    return !(e && std::strcmp(e, "strips") == 0);
  }();
  return on;
}

// ELEM_BYTES = sizeof(T), COMPLEX: T is complex.  The row-owner kernels exist for double and complex double only and
// want: whole 64-row strips in every tile (nb and last_rows multiples of 64), n a whole number of macro blocks, L lower,
// and 16-byte aligned bases and strides of B, L and winv (direct-to-LDS 16-byte loads).
template <int ELEM_BYTES, bool COMPLEX, class Args>
inline TrsmChoice trsm_path(const Args& a, bool rows_enabled) {
  auto aligned16 = [](const void* ptr, long stride_elems) {
    return (reinterpret_cast<std::uintptr_t>(ptr) % 16 == 0) && ((stride_elems * (long) ELEM_BYTES) % 16 == 0);
  };
  const bool vec = aligned16(a.b, a.ldb) && aligned16(a.b, a.b_ts) && aligned16(a.l, a.ldl);
  const bool rows = vec && !a.upper && rows_enabled && a.nb % 64 == 0 && a.last_rows % 64 == 0 && aligned16(a.winv, 0);
  if (ELEM_BYTES == 8 && !COMPLEX && rows) {
    // (a 512-column macro block -- 256 accumulator registers per lane -- does not survive the register allocator:
    // spills inside the loops; 256 columns run at two waves per SIMD without any)
    if (a.n % 256 == 0)
      return {TrsmPath::rows256, vec};
    // the tall-skinny solves of the blocked panel factorization of reduction_to_band: n = band = 128
    if (a.n % 128 == 0)
      return {TrsmPath::rows128, vec};
  }
  if (ELEM_BYTES == 16 && COMPLEX && rows && a.n % 128 == 0)
    return {TrsmPath::rows_z128, vec};
  return {TrsmPath::strips, vec};
}

template <int ELEM_BYTES, bool COMPLEX, class Args>
inline TrsmChoice trsm_path(const Args& a) {
  return trsm_path<ELEM_BYTES, COMPLEX>(a, trsm_rows_enabled());
}

}  // namespace dlaf_mi355x
