// host_operand.hpp -- how a matrix is named between the C API and the grid-level drivers.  Host only: no HIP header
// (api_checks.hpp judges these descriptions in a plain g++ program).
#pragma once
#include <type_traits>

namespace dlaf_mi355x {

// A distributed matrix AS STORED: rows, columns, row block, column block, source process.  What the require_* functions
// of api_checks.hpp judge, whether the matrix is a caller's host array or a resident handle.
struct OperandDesc {
  long m, n;
  int mb, nb;
  int isrc, jsrc;
};

// A caller's host matrix: its description and this process's local column-major part (p, leading dimension ld).
// T is const-qualified for an operand that is only read; an operand converts to its read-only form.
template <class T>
struct HostOperand : OperandDesc {
  T* p;
  long ld;
  HostOperand(const OperandDesc& d, T* p_, long ld_) : OperandDesc(d), p(p_), ld(ld_) {}
  template <class U, class = std::enable_if_t<std::is_same_v<const U, T>>>
  HostOperand(const HostOperand<U>& o) : OperandDesc(o), p(o.p), ld(o.ld) {}
};

}  // namespace dlaf_mi355x
