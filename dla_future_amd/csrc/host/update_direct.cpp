// update_direct.cpp -- ONE launch of the grouped update kernel on host operands, every field of the launch given by
// the caller (dlaf_mi355x_update_direct_*): the entry the tests compare the kernel itself with a reference through,
// at geometries no driver happens to produce.  Upload, launch_update once, download.
#include <algorithm>
#include <vector>

#include <dlaf_mi355x/dlaf_mi355x.h>

#include "device_matrix.hpp"
#include "direct.hpp"
#include "direct_operand.hpp"
#include "launch_args.hpp"

namespace dlaf_mi355x {

namespace {

// what update_args / rect_update_args read of a matrix
template <class T>
struct TileGrid {
  T* tiles;
  size_t tile_elems;
  long ltr, ltc;
  int nb;
  Axis rows, cols;
};

// Every element the launch may touch lies inside its operand?  Walks the tiles the kernel's contract names
// (device_api.hpp), not the kernel's blocks.
template <class T>
bool in_bounds(const UpdateArgs<T>& ua, const dlaf_mi355x_update_desc& d) {
  if (ua.pr < 1 || ua.pc < 1 || ua.ri < 0 || ua.ri >= ua.pr || ua.ci < 0 || ua.ci >= ua.pc || ua.il0 < 0 || ua.jl0 < 0 ||
      ua.nb < 1 || ua.K < 1 || ua.nt < 1 || ua.last_rows < 1 || ua.last_rows > ua.nb || ua.ldc < 1 || ua.lda < 1 ||
      ua.ldb < 1 || ua.b_period < 1 || ua.K1 < 0 || ua.K1 >= ua.K || (ua.her2k && ua.K1 == 0) ||
      (ua.rect && (ua.nt_c < 1 || ua.last_cols < 1 || ua.last_cols > ua.nb)) || (ua.rect && ua.her2k))
    return false;
  const int bj0 = ua.b_jl0 >= 0 ? ua.b_jl0 : ua.jl0;
  if (bj0 > ua.jl0)
    return false;
  // columns of each panel the kernel reads
  const long k2 = ua.K - ua.K1;
  const long ka = ua.K1 > 0 ? (ua.her2k ? std::max<long>(ua.K1, k2) : ua.K1) : ua.K;
  const long ka2 = ua.her2k ? std::max<long>(ua.K1, k2) : k2;
  const long kb = ua.K1 > 0 ? ua.K1 : ua.K;
  auto inside = [](long first, long last, long elems) { return first >= 0 && last < elems; };
  for (long il = ua.il0; il < ua.il1; ++il) {
    const long gi = il * ua.pr + ua.ri;
    if (gi >= ua.nt)
      return false;
    const long rows = gi == ua.nt - 1 ? ua.last_rows : ua.nb;
    if (rows > ua.lda || rows > ua.ldc)
      return false;
    const long a0 = (il - ua.il0) * ua.a_ts;
    bool row_used = false;
    for (long jl = ua.jl0; jl < ua.jl1; ++jl) {
      const long gj = jl * ua.pc + ua.ci;
      if (!ua.rect && gi < gj)
        continue;
      if (gj >= (ua.rect ? ua.nt_c : ua.nt))
        return false;
      row_used = true;
      const long cols = ua.rect ? (gj == ua.nt_c - 1 ? ua.last_cols : ua.nb) : (gj == ua.nt - 1 ? ua.last_rows : ua.nb);
      const long c0 = il * ua.c_tsr + jl * ua.c_tsc;
      if (!inside(c0, c0 + rows - 1 + (cols - 1) * ua.ldc, d.c_elems))
        return false;
      if (!ua.rect && gi == gj)
        continue;  // the column operand of a diagonal tile is the row panel
      if (cols > ua.ldb)
        return false;
      const long jt = jl - bj0;
      const long b0 = (jt % ua.b_period) * ua.b_ts2 + (jt / ua.b_period) * ua.b_ts;
      if (!inside(b0, b0 + cols - 1 + (kb - 1) * ua.ldb, d.b_elems))
        return false;
      if (ua.K1 > 0 && !inside(b0, b0 + cols - 1 + (k2 - 1) * ua.ldb, d.b2_elems))
        return false;
    }
    if (!row_used)
      continue;
    if (!inside(a0, a0 + rows - 1 + (ka - 1) * ua.lda, d.a_elems))
      return false;
    if (ua.K1 > 0 && !inside(a0, a0 + rows - 1 + (ka2 - 1) * ua.lda, d.a2_elems))
      return false;
  }
  return true;
}

}  // namespace

template <class T>
int update_direct(dlaf_mi355x_update_desc& d, void* c, const void* a, const void* b, const void* a2, const void* b2,
                  void* c_again) {
  runtime_init();
  if (d.role < 0 || d.role > 4)
    return -1;
  if (d.c_elems < 1 || d.a_elems < 1 || d.b_elems < 1 || d.c_off < 0 || d.a_off < 0 || d.b_off < 0 || d.a2_off < 0 ||
      d.b2_off < 0 || d.excl_rounds < 0 || (d.K1 > 0 && (d.a2_elems < 1 || d.b2_elems < 1 || !a2 || !b2)))
    return -3;
  hipStream_t s = nullptr;
  Operand<T> dc, da, db, da2, db2;
  dc.put(c, d.c_elems, d.c_off, s);
  if (d.K1 > 0 && d.second_below) {
    da2.put_below(a2, d.a2_elems, d.a2_off, da, a, d.a_elems, d.a_off, s);
    db2.put_below(b2, d.b2_elems, d.b2_off, db, b, d.b_elems, d.b_off, s);
  }
  else {
    da.put(a, d.a_elems, d.a_off, s);
    db.put(b, d.b_elems, d.b_off, s);
    if (d.K1 > 0) {
      da2.put(a2, d.a2_elems, d.a2_off, s);
      db2.put(b2, d.b2_elems, d.b2_off, s);
    }
  }
  DevBuf<int> info(1);
  DevBuf<unsigned> counters(16);
  DLAF_HIP_CHECK(hipMemcpyAsync(info.p, &d.info, sizeof(int), hipMemcpyHostToDevice, s));
  DLAF_HIP_CHECK(hipMemsetAsync(counters.p, 0, 16 * sizeof(unsigned), s));

  UpdateArgs<T> ua{};
  if (d.tile_layout) {
    if (d.ltr < 1 || d.ltc < 1 || d.nb < 1 || d.pr < 1 || d.pc < 1 || d.nt < 1)
      return -3;
    TileGrid<T> m;
    m.tiles = dc.p;
    m.tile_elems = (size_t) d.nb * d.nb;
    m.ltr = d.ltr;
    m.ltc = d.ltc;
    m.nb = d.nb;
    m.rows = Axis{(long) (d.nt - 1) * d.nb + d.last_rows, d.nb, d.pr, d.ri, 0};
    m.cols = d.rect ? Axis{(long) (d.nt_c - 1) * d.nb + d.last_cols, d.nb, d.pc, d.ci, 0}
                    : Axis{m.rows.n, d.nb, d.pc, d.ci, 0};
    const T* ap = da.p;
    const T* bp = db.p;
    ua = d.rect ? rect_update_args(m, d.il0, d.il1, d.jl0, d.jl1, ap, bp, d.b_ts, d.K, info.p)
                : update_args(m, d.il0, d.il1, d.jl0, d.jl1, ap, bp, d.b_ts, d.K, info.p);
  }
  else {
    ua.c = dc.p;
    ua.c_tsr = d.c_tsr;
    ua.c_tsc = d.c_tsc;
    ua.ldc = d.ldc;
    ua.a = da.p;
    ua.a_ts = d.a_ts;
    ua.lda = d.lda;
    ua.b = db.p;
    ua.b_ts = d.b_ts;
    ua.ldb = d.ldb;
    ua.il0 = d.il0;
    ua.il1 = d.il1;
    ua.jl0 = d.jl0;
    ua.jl1 = d.jl1;
    ua.nb = d.nb;
    ua.K = d.K;
    ua.pr = d.pr;
    ua.ri = d.ri;
    ua.pc = d.pc;
    ua.ci = d.ci;
    ua.nt = d.nt;
    ua.last_rows = d.last_rows;
    ua.info = info.p;
    ua.rect = d.rect;
    ua.nt_c = d.nt_c;
    ua.last_cols = d.last_cols;
  }
  // what is particular to a launch (launch_args.hpp)
  ua.b_period = d.b_period;
  ua.b_ts2 = d.b_ts2;
  ua.b_jl0 = d.b_jl0;
  ua.K1 = d.K1;
  ua.her2k = d.her2k;
  if (d.K1 > 0) {
    ua.a2 = da2.p;
    ua.b2 = db2.p;
  }
  if (!in_bounds(ua, d))
    return -3;

  d.bulk_slots = update_bulk_slots<T>();
  const long max_blocks = d.max_blocks < 0 ? d.bulk_slots : d.max_blocks;
  const long excl_slots = (long) d.excl_rounds * update_exclusive_round<T>();
  long p0, x0, p1, x1;
  update_launch_stats(&p0, &x0);
  launch_update(ua, s, d.role, max_blocks, counters.p, true, excl_slots);
  DLAF_HIP_CHECK(hipMemcpyAsync(c_again ? c_again : c, dc.p, (size_t) d.c_elems * sizeof(T), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  if (c_again) {
    // the same launch once more, on the original C, with the counter words as the first launch left them
    std::vector<T> first((size_t) d.c_elems);
    std::copy_n(static_cast<const T*>(c_again), (size_t) d.c_elems, first.begin());
    DLAF_HIP_CHECK(hipMemcpyAsync(dc.p, c, (size_t) d.c_elems * sizeof(T), hipMemcpyHostToDevice, s));
    launch_update(ua, s, d.role, max_blocks, counters.p, false, excl_slots);
    DLAF_HIP_CHECK(hipMemcpyAsync(c_again, dc.p, (size_t) d.c_elems * sizeof(T), hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    std::copy_n(first.begin(), (size_t) d.c_elems, static_cast<T*>(c));
  }
  update_launch_stats(&p1, &x1);
  d.persistent = p1 - p0;
  d.exclusive = x1 - x0;
  return 0;
}

#define INST(T) \
  template int update_direct<T>(dlaf_mi355x_update_desc&, void*, const void*, const void*, const void*, const void*, void*);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
