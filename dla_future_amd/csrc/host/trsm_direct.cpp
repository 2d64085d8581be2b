// trsm_direct.cpp -- ONE launch of the panel TRSM on host operands, every field of the launch given by the caller
// (dlaf_mi355x_trsm_direct_*): the entry the tests compare the TRSM kernels and the diagonal-block inversion that feeds
// them with a reference through, at geometries no driver happens to produce.  Upload, prepare winv, launch_trsm once,
// download.
#include <algorithm>

#include <dlaf_mi355x/dlaf_mi355x.h>

#include "../device/trsm_path.hpp"
#include "direct.hpp"
#include "direct_operand.hpp"

namespace dlaf_mi355x {

namespace {

// Every element the launches may touch lies inside its operand?  Walks the tiles and extents the contract names
// (TrsmArgs, launch_potrf_diag and launch_invert_diag_blocks in device_api.hpp), not the kernels' blocks.
bool in_bounds(const dlaf_mi355x_trsm_desc& d) {
  if (d.pr < 1 || d.ri < 0 || d.ri >= d.pr || d.il0 < 0 || d.il1 < d.il0 || d.nb < 1 || d.nt < 1 || d.last_rows < 1 ||
      d.last_rows > d.nb || d.ldb < 1 || d.ldl < 1 || d.n < 1 || d.n > d.ldl || d.b_ts < 0 || d.winv_source < 0 ||
      d.winv_source > 2)
    return false;
  auto inside = [](long first, long last, long elems) { return first >= 0 && last < elems; };
  for (long il = d.il0; il < d.il1; ++il) {
    const long gi = il * d.pr + d.ri;
    if (gi >= d.nt)
      return false;
    const long rows = gi == d.nt - 1 ? d.last_rows : d.nb;
    if (rows > d.ldb)
      return false;
    const long t0 = (il - d.il0) * d.b_ts;
    if (!inside(t0, t0 + rows - 1 + (long) (d.n - 1) * d.ldb, d.b_elems))
      return false;
  }
  // L: n x n (both triangles lie inside, whichever is read); winv: ceil(n / 64) dense 64 x 64 blocks
  if (!inside(0, (long) (d.n - 1) + (long) (d.n - 1) * d.ldl, d.l_elems))
    return false;
  const long nblk = (d.n + kDiagBlock - 1) / kDiagBlock;
  return nblk * kDiagBlock * kDiagBlock <= d.w_elems;
}

}  // namespace

template <class T>
int trsm_direct(dlaf_mi355x_trsm_desc& d, void* b, const void* l, void* winv) {
  runtime_init();
  if (d.b_elems < 1 || d.l_elems < 1 || d.w_elems < 1 || d.b_off < 0 || d.l_off < 0 || d.w_off < 0 ||
      ((size_t) d.w_off * sizeof(T)) % 16 != 0 || !in_bounds(d))
    return -3;
  hipStream_t s = nullptr;
  Operand<T> db, dl, dw;
  db.put(b, d.b_elems, d.b_off, s);
  dl.put(l, d.l_elems, d.l_off, s);
  dw.put(winv, d.w_elems, d.w_off, s);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemcpyAsync(info.p, &d.info, sizeof(int), hipMemcpyHostToDevice, s));

  if (d.winv_source == 0) {
    launch_invert_diag_blocks<T>(dl.p, d.ldl, d.n, dw.p, info.p, s, d.upper != 0, d.unit != 0);
  }
  else if (d.winv_source == 1) {
    for (int j0 = 0; j0 < d.n; j0 += kDiagBlock)
      launch_potrf_diag<T>(dl.p + j0 + (size_t) j0 * d.ldl, d.ldl, std::min(kDiagBlock, d.n - j0),
                           dw.p + (size_t) (j0 / kDiagBlock) * kDiagBlock * kDiagBlock, info.p, 0, s, false, d.upper != 0,
                           d.unit != 0);
  }

  TrsmArgs<T> ta;
  ta.b = db.p;
  ta.b_ts = d.b_ts;
  ta.ldb = d.ldb;
  ta.il0 = d.il0;
  ta.il1 = d.il1;
  ta.pr = d.pr;
  ta.ri = d.ri;
  ta.nb = d.nb;
  ta.nt = d.nt;
  ta.last_rows = d.last_rows;
  ta.l = dl.p;
  ta.ldl = d.ldl;
  ta.winv = dw.p;
  ta.n = d.n;
  ta.info = info.p;
  ta.upper = d.upper;
  ta.prio = d.prio;
  const TrsmChoice ch = trsm_path<(int) sizeof(T), TypeInfo<T>::is_complex>(ta);
  d.path = (int) ch.path;
  d.vec = ch.vec ? 1 : 0;
  launch_trsm(ta, s);
  DLAF_HIP_CHECK(hipMemcpyAsync(b, db.p, (size_t) d.b_elems * sizeof(T), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipMemcpyAsync(winv, dw.p, (size_t) d.w_elems * sizeof(T), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipMemcpyAsync(&d.info_out, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  return 0;
}

#define INST(T) template int trsm_direct<T>(dlaf_mi355x_trsm_desc&, void*, const void*, void*);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
