// Sweep of the wavefront schedule of bt_band_to_tridiagonal (csrc/host/bt_wavefronts.hpp) on the host, against a model
// written here from the stage's definition, not from the header's helpers.
//
// The bulge chase makes nsweeps = n - 1 (complex) or n - 2 (real) sweeps.  Step st of sweep sw leaves a reflector on
// the rows from 1 + sw + st b, at most b of them; a reflector of one row is the identity for the real types and is kept
// for the complex ones only where it is the first of the last sweep (it makes the last off-diagonal element real).
// Sweep group jb holds the sweeps jb b .., has as many steps as its first sweep, and its block of step st acts on the
// rows [1 + (jb + st) b, + 2b) of E, cut at row n.  Applied one by one, the blocks go jb descending, st ascending.
// Checked per case (b in {2, 3, 4, 5, 8, 16} x n = 0 .. 6b + 3, and n = 20480 with b = 128; real and complex):
//   coverage      the batches issue exactly the blocks (jb, st), 0 <= jb <= jb_last, 0 <= st < steps(jb),
//                 1 + (jb + st) b < n, each once;
//   row ranges    a block's rows are [r0, r0 + min(2b, n - r0)), inside [1, n);
//   disjointness  the blocks of one batch touch pairwise disjoint rows;
//   order         two blocks whose rows intersect are issued in different batches, in their one-by-one order;
//   workspace     no batch holds more than ceil(n / b) / 2 + 2 blocks;
// and the header's steps_of / jb_last agree with the model's.
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "bt_wavefronts.hpp"

using namespace dlaf_mi355x;

static long g_cases = 0, g_blocks = 0, g_batches = 0, g_failures = 0;

static void fail(long n, long b, bool cplx, const char* what, long x, long y) {
  if (++g_failures <= 20)
    std::fprintf(stderr, "FAIL n=%ld b=%ld %s: %s (%ld, %ld)\n", n, b, cplx ? "complex" : "real", what, x, y);
}

// ---- the model
static long model_nsweeps(long n, bool cplx) {
  return cplx ? n - 1 : n - 2;
}
// reflectors of sweep sw that do something
static long model_steps_of_sweep(long n, long b, bool cplx, long sw) {
  if (sw < 0 || sw >= model_nsweeps(n, cplx))
    return 0;
  long steps = 0;
  for (long st = 0; 1 + sw + st * b < n; ++st) {
    const long len = std::min(b, n - (1 + sw + st * b));
    if (len >= 2 || (cplx && st == 0 && sw == n - 2))
      ++steps;
  }
  return steps;
}

struct Block {
  long jb, st, r0, rows, batch, seq;
};

static void check_case(long n, long b, bool cplx) {
  ++g_cases;
  const long nsweeps = model_nsweeps(n, cplx);
  long jb_last = -1;  // the last group that holds a sweep
  while ((jb_last + 1) * b < nsweeps)
    ++jb_last;
  long max_steps = 0;
  for (long jb = 0; jb <= jb_last; ++jb)
    max_steps = std::max(max_steps, model_steps_of_sweep(n, b, cplx, jb * b));

  const BtSchedule sc(n, b, cplx);
  if (nsweeps > 0 && sc.jb_last() != jb_last)
    fail(n, b, cplx, "jb_last", sc.jb_last(), jb_last);
  for (long jb = 0; jb <= jb_last + 2; ++jb)
    if (sc.steps_of(jb) != model_steps_of_sweep(n, b, cplx, jb * b))
      fail(n, b, cplx, "steps_of", jb, sc.steps_of(jb));

  const std::vector<BtBatch> batches = bt_wavefront_batches(n, b, cplx);
  g_batches += (long) batches.size();
  const long bound = (n + b - 1) / b / 2 + 2;
  std::vector<Block> blocks;
  std::vector<int> seen((size_t) (jb_last + 1) * (size_t) std::max<long>(max_steps, 1), 0);
  for (size_t q = 0; q < batches.size(); ++q) {
    const BtBatch& w = batches[q];
    if (w.count < 1 || w.count > bound)
      fail(n, b, cplx, "batch size beyond the workspace bound", w.count, bound);
    for (long i = 0; i < w.count; ++i) {
      Block k;
      k.jb = w.jb + i;
      k.st = w.ib + 2 * i - k.jb;
      k.r0 = w.r0 + 2 * b * i;
      k.rows = w.rows;
      k.batch = (long) q;
      if (k.jb < 0 || k.jb > jb_last || k.st < 0 || k.st >= model_steps_of_sweep(n, b, cplx, k.jb * b)) {
        fail(n, b, cplx, "a block that does not exist", k.jb, k.st);
        continue;
      }
      if (k.r0 != 1 + (k.jb + k.st) * b || k.r0 < 1 || k.r0 >= n)
        fail(n, b, cplx, "first row", k.r0, 1 + (k.jb + k.st) * b);
      if (k.rows != std::min(2 * b, n - k.r0) || k.r0 + k.rows > n)
        fail(n, b, cplx, "row count", k.rows, std::min(2 * b, n - k.r0));
      ++seen[(size_t) k.jb * max_steps + k.st];
      // place in the one-by-one order: jb descending, then st ascending
      k.seq = (jb_last - k.jb) * max_steps + k.st;
      blocks.push_back(k);
    }
  }
  g_blocks += (long) blocks.size();
  for (long jb = 0; jb <= jb_last; ++jb)
    for (long st = 0; st < model_steps_of_sweep(n, b, cplx, jb * b); ++st) {
      const int want = 1 + (jb + st) * b < n ? 1 : 0;
      if (seen[(size_t) jb * max_steps + st] != want)
        fail(n, b, cplx, "coverage", jb, st);
    }
  for (size_t x = 0; x < blocks.size(); ++x)
    for (size_t y = x + 1; y < blocks.size(); ++y) {
      const Block &p = blocks[x], &q = blocks[y];
      const bool meet = p.r0 < q.r0 + q.rows && q.r0 < p.r0 + p.rows;
      if (!meet)
        continue;
      if (p.batch == q.batch)
        fail(n, b, cplx, "overlapping blocks in one batch", p.batch, p.r0);
      else if ((p.batch < q.batch) != (p.seq < q.seq))
        fail(n, b, cplx, "order of overlapping blocks", p.seq, q.seq);
    }
}

int main() {
  for (long b : {2, 3, 4, 5, 8, 16})
    for (long n = 0; n <= 6 * b + 3; ++n)
      for (bool cplx : {false, true})
        check_case(n, b, cplx);
  for (bool cplx : {false, true})
    check_case(20480, 128, cplx);
  std::printf("cases %ld blocks %ld batches %ld failures %ld\n", g_cases, g_blocks, g_batches, g_failures);
  return g_failures == 0 ? 0 : 1;
}
