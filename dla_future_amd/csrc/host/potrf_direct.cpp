// potrf_direct.cpp -- ONE factorization of one diagonal tile on host operands, every field given by the caller
// (dlaf_mi355x_potrf_direct_*): the entry the tests compare the tile POTRF kernels with a reference through, on either
// path, at leading dimensions, placements, info words and hand-off states no driver happens to produce.  Upload,
// factor once, download.
#include <dlaf_mi355x/dlaf_mi355x.h>

#include "device_matrix.hpp"
#include "direct.hpp"
#include "direct_operand.hpp"

namespace dlaf_mi355x {

namespace {

// Every element the launches may touch lies inside its buffer?  The extents the contract names (launch_potrf_coop and
// launch_potrf_diag in device_api.hpp): the kb x kb tile with leading dimension ld, ceil(kb / 64) dense 64 x 64 blocks.
bool in_bounds(const dlaf_mi355x_potrf_desc& d) {
  if (d.kb < 1 || d.ld < d.kb || d.path < 0 || d.path > 1 || d.sync_zeroed_by < 0 || d.sync_zeroed_by > 1)
    return false;
  if ((long) (d.kb - 1) + (long) (d.kb - 1) * d.ld >= d.t_elems)
    return false;
  const long nblk = (d.kb + kDiagBlock - 1) / kDiagBlock;
  return nblk * kDiagBlock * kDiagBlock <= d.w_elems;
}

}  // namespace

template <class T>
int potrf_direct(dlaf_mi355x_potrf_desc& d, void* tile, void* winv) {
  runtime_init();
  if (d.t_elems < 1 || d.w_elems < 1 || d.t_off < 0 || d.w_off < 0 || ((size_t) d.w_off * sizeof(T)) % 16 != 0 ||
      !in_bounds(d))
    return -3;
  hipStream_t s = nullptr;
  Operand<T> dt, dw;
  dt.put(tile, d.t_elems, d.t_off, s, true);
  dw.put(winv, d.w_elems, d.w_off, s, true);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemcpyAsync(info.p, &d.info, sizeof(int), hipMemcpyHostToDevice, s));

  DevBuf<unsigned> sync;  // (lives until the stream has drained)
  if (d.path == 0) {
    const size_t words = potrf_coop_sync_words(d.kb);
    sync.alloc(words);
    if (d.sync_zeroed_by == 0)
      DLAF_HIP_CHECK(hipMemsetAsync(sync.p, 0xFF, sizeof(unsigned) * words, s));  // a launcher that forgets shows
    else
      DLAF_HIP_CHECK(zero_device_now(sync.p, sizeof(unsigned) * words));
    potrf_tile_coop(dt.p, d.ld, d.kb, dw.p, info.p, d.info_base, sync.p, s, d.sync_zeroed_by == 1, d.count_strips != 0);
  }
  else {
    potrf_tile_chain(dt.p, d.ld, d.kb, dw.p, info.p, d.info_base, s);
  }
  DLAF_HIP_CHECK(hipGetLastError());
  DLAF_HIP_CHECK(hipMemcpyAsync(tile, dt.p, (size_t) d.t_elems * sizeof(T), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipMemcpyAsync(winv, dw.p, (size_t) d.w_elems * sizeof(T), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipMemcpyAsync(&d.info_out, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  d.t_before_changed = dt.before_changed(s);
  d.w_before_changed = dw.before_changed(s);
  return 0;
}

#define INST(T) template int potrf_direct<T>(dlaf_mi355x_potrf_desc&, void*, void*);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
