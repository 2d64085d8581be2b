// bt_wavefronts.hpp -- the wavefront schedule of bt_band_to_tridiagonal (eigensolver.cpp): which reflector blocks run in
// one batched launch, and in which order.  Host arithmetic only (no HIP header: tests/bt_wavefronts/sweep.cpp compiles
// it with a plain host compiler and checks it against a model of its own).
//
// Sweep group jb holds the sweeps jb b .. jb b + b - 1 of the bulge chase; its block of step st, (jb, ib = jb + st), acts
// on the rows [1 + ib b, + 2b) of E (fewer at the bottom edge).  Applied one by one the blocks go jb descending, st
// ascending: a block must follow (jb, st - 1) and the blocks of group jb + 1 that overlap it.  All blocks with the same
// t = st - jb touch disjoint rows and have their predecessors in earlier wavefronts, so wavefront t runs as batches:
// block q of a batch is (jb + q, ib + 2 q) at the rows r0 + 2 b q -- one block stride (nblk + 2 slots of the block grid)
// and one row stride for a strided-batch launch.
#pragma once
#include <algorithm>
#include <vector>

namespace dlaf_mi355x {

struct BtSchedule {
  long n, b, nsweeps, nblk;
  bool is_complex;
  BtSchedule(long n_, long b_, bool is_complex_)
      : n(n_), b(b_), nsweeps(is_complex_ ? n_ - 1 : n_ - 2), nblk((n_ + b_ - 1) / b_), is_complex(is_complex_) {}
  // steps of sweep group jb (its first sweep has the most)
  long steps_of(long jb) const {
    const long sw = jb * b;
    if (sw >= nsweeps)
      return 0;
    if (is_complex && sw == n - 2)
      return 1;
    return (n - sw - 2 + b - 1) / b;
  }
  long jb_last() const { return (nsweeps - 1) / b; }
  // wavefront t = step - jb, from the last sweep group's first step to the first group's last step
  long t_lo() const { return -jb_last(); }
  long t_hi() const { return steps_of(0) - 1; }
  // the most blocks a batch may hold (what the W2 workspace of the strided-batch path is sized for)
  long max_batch() const { return nblk / 2 + 2; }
};

struct BtBatch {
  long jb, ib;  // the first block: sweep group, block row
  long r0;      // its first row of E, 1 + ib b
  long count;   // blocks in the batch
  long rows;    // rows each of them touches
};

// The batches in issue order.  Per wavefront: the blocks with all their 2b rows in one batch, then the ragged ones at the
// bottom edge one by one.
inline std::vector<BtBatch> bt_wavefront_batches(long n, long b, bool is_complex) {
  std::vector<BtBatch> out;
  const BtSchedule sc(n, b, is_complex);
  if (sc.nsweeps <= 0)
    return out;
  const long jb_last = sc.jb_last();
  for (long t = sc.t_lo(); t <= sc.t_hi(); ++t) {
    const long jb0 = std::max<long>(0, -t);
    // blocks (jb, st = t + jb), jb = jb0 ...: valid while st < steps_of(jb)
    long cnt = 0, full = 0;
    for (long jb = jb0; jb <= jb_last; ++jb) {
      const long st = t + jb;
      if (st >= sc.steps_of(jb))
        break;
      const long r0 = 1 + (jb + st) * b;
      if (r0 >= n)
        break;
      ++cnt;
      if (r0 + 2 * b <= n)
        ++full;
    }
    auto batch = [&](long first, long count, long rows) {
      const long jb = jb0 + first, ib = 2 * jb + t;
      if (count > 0)
        out.push_back(BtBatch{jb, ib, 1 + ib * b, count, rows});
    };
    batch(0, full, 2 * b);
    for (long q = full; q < cnt; ++q)
      batch(q, 1, n - (1 + (2 * (jb0 + q) + t) * b));
  }
  return out;
}

}  // namespace dlaf_mi355x
