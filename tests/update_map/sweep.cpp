// Sweep of the grouped update kernel's work-item map (csrc/device/update_map.hpp) on the host: for every geometry,
// every block the kernel's contract (device_api.hpp) says is updated must lie in a patch the map enumerates (a patch
// is (1 << ps) block rows x (1 << psc) block columns; patch column pj holds the LAST colstart[pj+1] - colstart[pj]
// patch rows), the work-item count must be that of the enumerated patches, and the XCD remap of a
// one-block-per-workgroup launch must be a permutation of the work items.  The expected set is enumerated here from
// the contract, tile by tile.  (The decode of a work item lives in the kernel and is compared on the GPU.)
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "update_map.hpp"

using namespace dlaf_mi355x;

struct Geom {
  int il0, il1, jl0, jl1, nb;
  int pr, ri, pc, ci;
  int nt, last_rows;
  int rect, nt_c, last_cols;
};

static long g_geoms = 0, g_items = 0, g_failures = 0;

static void fail(const Geom& g, int BM, int BN, const char* what, long w) {
  if (++g_failures <= 20)
    std::fprintf(stderr,
                 "FAIL %s (w=%ld): BM=%d BN=%d nb=%d pr=%d ri=%d pc=%d ci=%d nt=%d last_rows=%d rect=%d nt_c=%d "
                 "last_cols=%d il=[%d,%d) jl=[%d,%d)\n",
                 what, w, BM, BN, g.nb, g.pr, g.ri, g.pc, g.ci, g.nt, g.last_rows, g.rect, g.nt_c, g.last_cols, g.il0,
                 g.il1, g.jl0, g.jl1);
}

template <int BM, int BN>
static void check(const Geom& g) {
  ++g_geoms;
  // the contract: local tiles (il, jl) of the range, global (gi, gj); nothing above the block-cyclic diagonal unless
  // rect; the tile's extent; on a diagonal tile only blocks that reach the lower triangle
  const int bm = (g.nb + BM - 1) / BM, bn = (g.nb + BN - 1) / BN;
  std::vector<std::pair<int, int>> blocks;  // (block row, block column) of the domain
  for (int il = g.il0; il < g.il1; ++il)
    for (int jl = g.jl0; jl < g.jl1; ++jl) {
      const int gi = il * g.pr + g.ri, gj = jl * g.pc + g.ci;
      if (!g.rect && gi < gj)
        continue;
      const int rows = gi == g.nt - 1 ? g.last_rows : g.nb;
      const int cols = g.rect ? (gj == g.nt_c - 1 ? g.last_cols : g.nb) : (gj == g.nt - 1 ? g.last_rows : g.nb);
      const bool diag = !g.rect && gi == gj;
      for (int m0 = 0; m0 < rows; m0 += BM)
        for (int n0 = 0; n0 < cols; n0 += BN) {
          const int mrows = rows - m0 < BM ? rows - m0 : BM;
          if (diag && m0 + mrows - 1 < n0)
            continue;  // every element of the block lies strictly above the diagonal
          blocks.emplace_back((il - g.il0) * bm + m0 / BM, (jl - g.jl0) * bn + n0 / BN);
        }
    }
  const long wanted = (long) blocks.size();
  UpdateMap mp;
  if (!build_update_map<BM, BN>(g, mp)) {
    if (wanted != 0)
      fail(g, BM, BN, "empty map for a domain with blocks", -1);
    return;
  }
  if (mp.total <= 0 || (mp.xcd && mp.total % 8 != 0)) {
    fail(g, BM, BN, "total", mp.total);
    return;
  }
  g_items += mp.total;
  std::vector<unsigned char> hit((size_t) mp.total, 0);
  for (long v = 0; v < mp.total; ++v) {
    const long w = update_xcd_remap(mp, v);
    if (w < 0 || w >= mp.total || hit[(size_t) w]++) {
      fail(g, BM, BN, "xcd remap is no permutation", v);
      return;
    }
  }
  if (mp.bpt_m != bm || mp.bpt_n != bn || mp.RB != (g.il1 - g.il0) * bm || mp.CB != (g.jl1 - g.jl0) * bn ||
      mp.PR != (mp.RB + (1 << mp.ps) - 1) >> mp.ps || mp.PC != (mp.CB + (1 << mp.psc) - 1) >> mp.psc) {
    fail(g, BM, BN, "domain extents", -1);
    return;
  }
  long npatch = (long) mp.PR * mp.PC;
  if (mp.tri) {
    for (int pj = 0; pj < mp.PC; ++pj) {
      const int cnt = mp.colstart[pj + 1] - mp.colstart[pj];
      if (mp.colstart[0] != 0 || cnt < 0 || cnt > mp.PR) {
        fail(g, BM, BN, "colstart", pj);
        return;
      }
    }
    npatch = mp.colstart[mp.PC];
  }
  if (mp.total != npatch << (mp.ps + mp.psc)) {
    fail(g, BM, BN, "work items != enumerated patches", mp.total);
    return;
  }
  for (const auto& b : blocks) {
    const int pi = b.first >> mp.ps, pj = b.second >> mp.psc;
    if (pi >= mp.PR || pj >= mp.PC || (mp.tri && pi < mp.PR - (mp.colstart[pj + 1] - mp.colstart[pj]))) {
      fail(g, BM, BN, "block of the contract in no enumerated patch", (long) b.first * mp.CB + b.second);
      return;
    }
  }
}

template <int BM, int BN>
static void sweep() {
  for (int mult = 1; mult <= 3; ++mult) {
    const int nb = mult * BM;
    for (int pr = 1; pr <= 4; ++pr)
      for (int pc = 1; pc <= 4; ++pc)
        for (int ri = 0; ri < pr; ++ri)
          for (int ci = 0; ci < pc; ++ci)
            for (int nt = 1; nt <= 40; ++nt) {
              const int ltr = (nt - ri + pr - 1) / pr;  // local tile rows: global tiles ri, ri + pr, ... < nt
              if (ltr <= 0)
                continue;
              const int lasts[3] = {1, nb, nb > 37 + BN ? BN + 37 : 37};
              const int last_rows = lasts[nt % 3];
              for (int rect = 0; rect <= 1; ++rect) {
                const int nt_c = !rect ? nt : ((nt & 1) ? nt + 3 : (nt + 1) / 2);
                const int last_cols = !rect ? last_rows : lasts[(nt + 1) % 3];
                const int ltc = (nt_c - ci + pc - 1) / pc;
                if (ltc <= 0)
                  continue;
                // the whole domain, a domain that starts below the top, a single column (lookahead), a window in the
                // middle, and a column range that starts right of where the row range does (first patch column
                // starts below row il0)
                const int ranges[6][4] = {{0, ltr, 0, ltc},
                                          {ltr / 3, ltr, 0, ltc},
                                          {0, ltr, ltc / 2, ltc / 2 + 1},
                                          {ltr / 4, ltr - ltr / 5, ltc / 3, ltc - ltc / 4},
                                          {ltr / 2, ltr, ltc / 2, ltc},
                                          {1, ltr, ltc - 1, ltc}};
                for (const auto& r : ranges) {
                  if (r[0] >= r[1] || r[2] >= r[3])
                    continue;
                  check<BM, BN>(Geom{r[0], r[1], r[2], r[3], nb, pr, ri, pc, ci, nt, last_rows, rect, nt_c, last_cols});
                }
              }
            }
  }
  // tile sizes that are no multiple of the block
  for (int nb : {1, 37, BM + 1, 2 * BM - 1})
    for (int nt : {1, 2, 17, 40})
      for (int pr = 1; pr <= 2; ++pr)
        for (int ri = 0; ri < pr; ++ri) {
          const int ltr = (nt - ri + pr - 1) / pr;
          if (ltr > 0)
            check<BM, BN>(Geom{0, ltr, 0, nt, nb, pr, ri, 1, 0, nt, (nb + 1) / 2, 0, 0, 0});
        }
}

int main() {
  sweep<128, 128>();
  sweep<128, 64>();
  std::printf("geometries %ld work items %ld failures %ld\n", g_geoms, g_items, g_failures);
  return g_failures == 0 ? 0 : 1;
}
