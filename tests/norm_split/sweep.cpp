// Sweep of the norm kernels' work split and partial-buffer layout (csrc/device/norm_split.hpp) on the host.  For every
// geometry the loops of pass 1 are replayed unit by unit, wave by wave, load by load, exactly as kernels_norm.hip runs
// them, and the loops of pass 2 as its kernels run them:
//   * every referenced element (inside the tile's extent; on and below the diagonal of a diagonal tile for the
//     Hermitian / triangular structure) is covered exactly once, nothing else is covered, and every 16-byte load stays
//     inside its tile;
//   * every scalar, column and row partial slot has at most one writer and lies inside its buffer;
//   * pass 2 reads written slots only, and reads every written column / row slot exactly once.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "norm_split.hpp"

using namespace dlaf_mi355x;

static long g_geoms = 0, g_units = 0, g_failures = 0;

struct Case {
  long m, n;  // global extents
  int nb, pr, ri, pc, ci, structure, elem_bytes, aligned;
};

static void fail(const Case& c, const char* what, long where) {
  if (++g_failures <= 20)
    std::fprintf(stderr, "FAIL %s (%ld): m=%ld n=%ld nb=%d pr=%d ri=%d pc=%d ci=%d structure=%d bytes=%d aligned=%d\n", what,
                 where, c.m, c.n, c.nb, c.pr, c.ri, c.pc, c.ci, c.structure, c.elem_bytes, c.aligned);
}

// local tiles and local extent of one axis: global tiles shift, shift + P, ...
static void local_axis(long n, int nb, int P, int shift, int& lt, long& local) {
  const long nt = n > 0 ? (n + nb - 1) / nb : 0;
  lt = 0;
  local = 0;
  for (long g = shift; g < nt; g += P) {
    ++lt;
    local += (g == nt - 1) ? n - g * nb : nb;
  }
}

static void check(const Case& c) {
  ++g_geoms;
  NormGeom g{};
  g.nb = c.nb;
  g.pr = c.pr;
  g.ri = c.ri;
  g.pc = c.pc;
  g.ci = c.ci;
  g.structure = c.structure;
  local_axis(c.m, c.nb, c.pr, c.ri, g.ltr, g.rows);
  local_axis(c.n, c.nb, c.pc, c.ci, g.ltc, g.cols);
  const bool aligned = c.aligned && ((long) c.nb * c.elem_bytes) % 16 == 0;
  const NormSplit s = norm_split(c.nb, c.elem_bytes, aligned, norm_referenced_tiles(g));
  if (s.ve < 1 || s.slab_rows != kNormSlabLoads * kNormLanes * s.ve || s.nsl * s.slab_rows < c.nb || s.cw < 1 ||
      (long) s.nch * s.cw < c.nb || (s.nch - 1) * s.cw >= c.nb || (s.nsl - 1) * s.slab_rows >= c.nb ||
      s.ve * c.elem_bytes > 16 || (s.ve > 1 && c.nb % s.ve != 0))
    return fail(c, "split", 0);
  const long units = norm_unit_count(g, s), ncol = norm_colp_elems(g, s), nrow = norm_rowp_elems(g, s);
  const long ldr = (long) g.ltr * g.nb, ldc = (long) g.ltc * g.nb;
  std::vector<unsigned char> hit((size_t) (ldr * ldc), 0), wsc((size_t) units, 0), wcol((size_t) ncol, 0),
      wrow((size_t) nrow, 0);
  for (int jl = 0; jl < g.ltc; ++jl)
    for (int il = 0; il < g.ltr; ++il)
      for (int ch = 0; ch < s.nch; ++ch)
        for (int sl = 0; sl < s.nsl; ++sl) {
          ++g_units;
          const long u = norm_unit_index(g, s, il, jl, sl, ch);
          if (u < 0 || u >= units)
            return fail(c, "unit index", u);
          if (wsc[(size_t) u]++)
            return fail(c, "two writers of a scalar slot", u);
          if (!norm_unit_live(g, s, il, jl, sl, ch))
            continue;
          const int rt = norm_tile_rows(g, il), ct = norm_tile_cols(g, jl);
          const bool dtile = g.structure != 0 && (long) il * g.pr + g.ri == (long) jl * g.pc + g.ci;
          const int c0 = ch * s.cw, c1 = ct < c0 + s.cw ? ct : c0 + s.cw;
          for (int w = 0; w < kNormWaves; ++w)
            for (int col = c0 + w; col < c1; col += kNormWaves) {
              const long cs = norm_colp_slot(g, s, il, sl, jl, col);
              if (cs < 0 || cs >= ncol)
                return fail(c, "column slot", cs);
              if (wcol[(size_t) cs]++)
                return fail(c, "two writers of a column slot", cs);
              for (int q = 0; q < kNormSlabLoads; ++q)
                for (int lane = 0; lane < kNormLanes; ++lane) {
                  const int r = norm_row_of(s, sl, q, lane, 0);
                  if (r < rt && r + s.ve > g.nb)
                    return fail(c, "load leaves the tile", r);
                  for (int e = 0; e < s.ve; ++e) {
                    const int rr = norm_row_of(s, sl, q, lane, e);
                    if (rr < rt && (!dtile || rr >= col))
                      ++hit[(size_t) ((long) il * g.nb + rr + ((long) jl * g.nb + col) * ldr)];
                  }
                }
            }
          const int r0 = sl * s.slab_rows;
          for (int idx = 0; idx < s.slab_rows && r0 + idx < rt; ++idx) {
            const long rs = norm_rowp_slot(g, s, jl, ch, il, r0 + idx);
            if (rs < 0 || rs >= nrow)
              return fail(c, "row slot", rs);
            if (wrow[(size_t) rs]++)
              return fail(c, "two writers of a row slot", rs);
          }
        }
  // coverage
  for (int jl = 0; jl < g.ltc; ++jl)
    for (int il = 0; il < g.ltr; ++il) {
      const long gi = (long) il * g.pr + g.ri, gj = (long) jl * g.pc + g.ci;
      const int rt = norm_tile_rows(g, il), ct = norm_tile_cols(g, jl);
      for (int col = 0; col < g.nb; ++col)
        for (int r = 0; r < g.nb; ++r) {
          const bool want = r < rt && col < ct && (g.structure == 0 || gi > gj || (gi == gj && r >= col));
          if (hit[(size_t) ((long) il * g.nb + r + ((long) jl * g.nb + col) * ldr)] != (want ? 1 : 0))
            return fail(c, "coverage", (long) il * g.nb + r);
        }
    }
  // pass 2 (norm_vector_kernel): every slot it reads was written, and every written slot is read once
  const long len = c.m > c.n ? c.m : c.n;
  for (long x = 0; x < len; ++x) {
    const long gt = x / g.nb;
    const int off = (int) (x % g.nb);
    if (gt % g.pc == g.ci && gt / g.pc < g.ltc) {
      const int jl = (int) (gt / g.pc);
      if (off < norm_tile_cols(g, jl))
        for (int il = 0; il < g.ltr; ++il)
          for (int sl = 0; sl < s.nsl; ++sl)
            if (norm_unit_live(g, s, il, jl, sl, off / s.cw)) {
              unsigned char& wr = wcol[(size_t) norm_colp_slot(g, s, il, sl, jl, off)];
              if (wr != 1)
                return fail(c, "column slot read but not written once", x);
              wr = 2;
            }
    }
    if (gt % g.pr == g.ri && gt / g.pr < g.ltr) {
      const int il = (int) (gt / g.pr);
      if (off < norm_tile_rows(g, il))
        for (int jl = 0; jl < g.ltc; ++jl)
          for (int ch = 0; ch < s.nch; ++ch)
            if (norm_unit_live(g, s, il, jl, off / s.slab_rows, ch)) {
              unsigned char& wr = wrow[(size_t) norm_rowp_slot(g, s, jl, ch, il, off)];
              if (wr != 1)
                return fail(c, "row slot read but not written once", x);
              wr = 2;
            }
    }
  }
  for (long i = 0; i < ncol; ++i)
    if (wcol[(size_t) i] == 1)
      return fail(c, "column slot written but never read", i);
  for (long i = 0; i < nrow; ++i)
    if (wrow[(size_t) i] == 1)
      return fail(c, "row slot written but never read", i);
  for (long i = 0; i < units; ++i)
    if (wsc[(size_t) i] != 1)
      return fail(c, "scalar slot without a writer", i);
}

static void all_types_and_structures(long m, long n, int nb, int pr, int ri, int pc, int ci) {
  for (int bytes : {4, 8, 16})
    for (int aligned = 0; aligned <= 1; ++aligned) {
      check(Case{m, n, nb, pr, ri, pc, ci, 0, bytes, aligned});
      if (m == n)
        for (int st = 1; st <= 2; ++st)
          check(Case{m, n, nb, pr, ri, pc, ci, st, bytes, aligned});
    }
}

int main() {
  // the shapes of the GPU tests, one process
  const long shapes[][3] = {{64, 64, 64},   {130, 67, 64},     {67, 130, 64},    {1, 300, 64},   {300, 1, 64},  {333, 333, 100},
                            {130, 130, 50}, {1100, 1100, 256}, {1100, 900, 256}, {600, 600, 256}, {700, 300, 128},
                            {1100, 1100, 300}, {2100, 2100, 1050}};
  for (const auto& sh : shapes)
    all_types_and_structures(sh[0], sh[1], (int) sh[2], 1, 0, 1, 0);
  // the grids of the distributed tests, every rank
  for (const auto& pq : {std::pair<int, int>{2, 3}, std::pair<int, int>{3, 2}})
    for (int ri = 0; ri < pq.first; ++ri)
      for (int ci = 0; ci < pq.second; ++ci) {
        all_types_and_structures(400, 400, 128, pq.first, ri, pq.second, ci);
        all_types_and_structures(100, 100, 64, pq.first, ri, pq.second, ci);
        all_types_and_structures(400, 130, 128, pq.first, ri, pq.second, ci);
      }
  // up to 64 x 64 tiles of small blocks, ragged and not, on grids up to 3 x 3
  for (int nb : {1, 3, 8, 50})
    for (int nt : {1, 2, 3, 7, 16, 64}) {
      if (nb == 50 && nt > 16)
        continue;
      for (int last : {1, nb / 2 + 1, nb})
        for (const auto& pq : {std::pair<int, int>{1, 1}, std::pair<int, int>{2, 3}, std::pair<int, int>{3, 3}})
          for (int ri = 0; ri < pq.first; ++ri)
            for (int ci = 0; ci < pq.second; ++ci) {
              const long n = (long) (nt - 1) * nb + last;
              all_types_and_structures(n, n, nb, pq.first, ri, pq.second, ci);
              if (nb == 8)
                all_types_and_structures(n, (n + 1) / 2, nb, pq.first, ri, pq.second, ci);
            }
    }
  std::printf("geometries %ld units %ld failures %ld\n", g_geoms, g_units, g_failures);
  return g_failures == 0 ? 0 : 1;
}
