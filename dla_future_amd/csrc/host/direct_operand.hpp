// direct_operand.hpp -- how update_direct.cpp, trsm_direct.cpp and potrf_direct.cpp place a host operand on the device.
#pragma once
#include <vector>

#include "pool.hpp"

namespace dlaf_mi355x {

// an operand's host array `off` elements into a device allocation of its own
template <class T>
struct Operand {
  static constexpr int kBeforeByte = 0xA5;
  DevBuf<T> buf;
  T* p = nullptr;
  size_t before = 0;  // guarded bytes in front of the host array
  // guard: the `off` elements in front of the array hold a byte pattern that before_changed() looks for again -- a
  // store in front of the buffer shows
  void put(const void* host, long elems, long off, hipStream_t s, bool guard = false) {
    buf.alloc((size_t) (elems + off));
    p = buf.p + off;
    before = guard ? (size_t) off * sizeof(T) : 0;
    if (before > 0)
      DLAF_HIP_CHECK(hipMemsetAsync(buf.p, kBeforeByte, before, s));
    if (elems > 0)
      DLAF_HIP_CHECK(hipMemcpyAsync(p, host, (size_t) elems * sizeof(T), hipMemcpyHostToDevice, s));
  }
  // this operand and, behind it in the SAME allocation (16 elements apart at least in alignment), `hi`: p < hi.p
  void put_below(const void* host, long elems, long off, Operand& hi, const void* hi_host, long hi_elems, long hi_off,
                 hipStream_t s) {
    const long span = (off + elems + 15) / 16 * 16;
    buf.alloc((size_t) (span + hi_off + hi_elems));
    p = buf.p + off;
    hi.p = buf.p + span + hi_off;
    DLAF_HIP_CHECK(hipMemcpyAsync(p, host, (size_t) elems * sizeof(T), hipMemcpyHostToDevice, s));
    DLAF_HIP_CHECK(hipMemcpyAsync(hi.p, hi_host, (size_t) hi_elems * sizeof(T), hipMemcpyHostToDevice, s));
  }
  // guarded bytes that no longer hold the pattern (synchronises the stream)
  int before_changed(hipStream_t s) const {
    std::vector<unsigned char> h(before);
    if (before > 0)
      DLAF_HIP_CHECK(hipMemcpyAsync(h.data(), buf.p, before, hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    int n = 0;
    for (unsigned char b : h)
      n += b != kBeforeByte;
    return n;
  }
};

}  // namespace dlaf_mi355x
