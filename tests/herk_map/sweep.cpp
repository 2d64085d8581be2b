// Sweep of the index arithmetic of the Hermitian rank-k / rank-2k update kernel (csrc/device/herk_map.hpp) on the
// host, against brute-force models:
//   * coverage: the kernel's own decisions (herk_tile_runs, the ragged-block return, herk_block_runs,
//     herk_element_stored, herk_element_diagonal) replayed for every process of a grid, every local tile, every block
//     and every element of it must store every element of the lower triangle of the n x n view exactly once and no
//     element above it, flag exactly the diagonal, and run no block that stores nothing -- for every nb in 1 .. 170 on
//     one process and for a list of tile sizes on grids up to 2 x 3 with every source process, ragged last tiles, and
//     both block shapes (128 x 128 and the 128 x 64 of complex double, whose blocks straddle the diagonal);
//   * forms: herk_form_x / herk_form_y must address, in a stored tile, the elements that under gemm_acc's convention
//     acc += x' * conj(y')  (x', y' the operands after a set flag has conjugated them) give the term of
//     A A^H (trans N) / A^H A (trans C), conjugated for a conj_view, and name the vector loader whose stride is 1;
//   * panel offsets: herk_panel_offset must be the place the grouped transposed-panel broadcast puts a tile.
#include <complex>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "herk_map.hpp"

using namespace dlaf_mi355x;

static long g_elements = 0, g_blocks = 0, g_forms = 0, g_failures = 0;

static void fail(const char* what, long a, long b, long c, long d) {
  if (++g_failures <= 20)
    std::fprintf(stderr, "FAIL %s: %ld %ld %ld %ld\n", what, a, b, c, d);
}

// n x n view in nb tiles on a prow x pcol grid with source (isrc, jsrc), BM x BN blocks
static void check_coverage(int n, int nb, int prow, int pcol, int isrc, int jsrc, int BM, int BN) {
  const int nt = (n + nb - 1) / nb, last = n - (nt - 1) * nb;
  const int bpr = (nb + BM - 1) / BM, bpc = (nb + BN - 1) / BN;
  std::vector<unsigned char> count((size_t) n * n, 0);
  for (int myr = 0; myr < prow; ++myr)
    for (int myc = 0; myc < pcol; ++myc) {
      const int ri = (myr + prow - isrc) % prow, ci = (myc + pcol - jsrc) % pcol;  // Axis::shift
      const int ltr = nt > ri ? (nt - ri + prow - 1) / prow : 0, ltc = nt > ci ? (nt - ci + pcol - 1) / pcol : 0;
      for (int jl = 0; jl < ltc; ++jl)
        for (int il = 0; il < ltr; ++il) {
          const int gi = il * prow + ri, gj = jl * pcol + ci;
          if (!herk_tile_runs(gi, gj))
            continue;
          const int rows_tile = gi == nt - 1 ? last : nb, cols_tile = gj == nt - 1 ? last : nb;
          for (int bn = 0; bn < bpc; ++bn)
            for (int bm = 0; bm < bpr; ++bm) {
              const int m0 = bm * BM, n0 = bn * BN;
              if (m0 >= rows_tile || n0 >= cols_tile)
                continue;
              const int mrows = rows_tile - m0 < BM ? rows_tile - m0 : BM, ncols = cols_tile - n0 < BN ? cols_tile - n0 : BN;
              if (!herk_block_runs(gi, gj, m0, mrows, n0, ncols))
                continue;
              ++g_blocks;
              long stored = 0;
              for (int c = 0; c < ncols; ++c)
                for (int r = 0; r < mrows; ++r) {
                  const long row = (long) gi * nb + m0 + r, col = (long) gj * nb + n0 + c;
                  const bool st = herk_element_stored(gi, gj, m0 + r, n0 + c);
                  const bool dg = herk_element_diagonal(gi, gj, m0 + r, n0 + c);
                  if (dg != (row == col))
                    fail("diagonal flag", row, col, nb, BN);
                  if (dg && !st)
                    fail("diagonal element not stored", row, col, nb, BN);
                  if (st) {
                    ++stored;
                    ++count[(size_t) row + (size_t) col * n];
                  }
                }
              if (stored == 0)
                fail("a block that runs stores nothing", gi, gj, m0, n0);
            }
        }
    }
  for (int c = 0; c < n; ++c)
    for (int r = 0; r < n; ++r) {
      ++g_elements;
      if (count[(size_t) r + (size_t) c * n] != (r >= c ? 1 : 0))
        fail(r >= c ? "triangle element not stored exactly once" : "element above the diagonal stored", r, c, nb, BN);
    }
}

using Z = std::complex<double>;

static void check_forms(int ld) {
  std::vector<Z> tile((size_t) ld * ld);
  for (int j = 0; j < ld; ++j)
    for (int i = 0; i < ld; ++i)
      tile[(size_t) i + (size_t) j * ld] = Z((double) (i + 1000 * j), (double) (1 + i - 2 * j));
  for (char trans : {'N', 'n', 'C', 'c', 'T'})
    for (int cv = 0; cv < 2; ++cv)
      for (int m0 : {0, 1, 7, 64, 128})
        for (int n0 : {0, 3, 64})
          for (int r = 0; m0 + r < ld && n0 + r < ld; r += (r < 3 ? 1 : 5))
            for (int k = 0; k < ld; k += (k < 3 ? 1 : 7)) {
              ++g_forms;
              const GemmForm fx = herk_form_x(trans, cv, ld, m0), fy = herk_form_y(trans, cv, ld, n0);
              const long ix = fx.off + r * fx.rs + k * fx.ks, iy = fy.off + r * fy.rs + k * fy.ks;
              if (ix < 0 || ix >= (long) ld * ld || iy < 0 || iy >= (long) ld * ld) {
                fail("address outside the tile", trans, ld, r, k);
                continue;
              }
              const bool tn = herk_trans_is_n(trans);
              // the model: row m0 + r / n0 + r of the stored n x k tile (trans N), column of the k x n tile (trans C)
              const Z ai = tn ? tile[(size_t) (m0 + r) + (size_t) k * ld] : tile[(size_t) k + (size_t) (m0 + r) * ld];
              const Z aj = tn ? tile[(size_t) (n0 + r) + (size_t) k * ld] : tile[(size_t) k + (size_t) (n0 + r) * ld];
              Z want = tn ? ai * std::conj(aj) : std::conj(ai) * aj;
              if (cv)
                want = std::conj(want);
              const Z x1 = fx.conj ? std::conj(tile[(size_t) ix]) : tile[(size_t) ix];
              const Z y1 = fy.conj ? std::conj(tile[(size_t) iy]) : tile[(size_t) iy];
              if (x1 * std::conj(y1) != want)
                fail("term of the update", trans, cv, r, k);
              const int vm = herk_vector_mode(trans);
              if (fx.vmode != vm || fy.vmode != vm || (vm == 0 ? (fx.rs != 1 || fy.rs != 1) : (fx.ks != 1 || fy.ks != 1)))
                fail("vector loader of the trans", trans, cv, ld, vm);
            }
}

// the grouped broadcast: class c = tiles c, c + period, ... packed from c * ts2, ts2 = ceil(ncols / period) tiles
static void check_panel_offsets() {
  const long ts = 9;
  for (int ncols = 1; ncols <= 13; ++ncols)
    for (int period = 1; period <= 4; ++period) {
      const long cap = (ncols + period - 1) / period, ts2 = cap * ts;
      std::vector<int> at((size_t) ((ncols + period) * ts), -1);
      for (int c = 0; c < period && c < ncols; ++c) {
        long pos = c * ts2;
        for (int jl = c; jl < ncols; jl += period, pos += ts)
          at[(size_t) pos] = jl;
      }
      for (int jl = 0; jl < ncols; ++jl) {
        const long o = herk_panel_offset(jl, period, ts, ts2);
        if (o < 0 || o >= (long) at.size() || at[(size_t) o] != jl)
          fail("panel offset", jl, period, ncols, o);
      }
    }
}

int main() {
  for (int nb = 1; nb <= 170; ++nb)
    for (int lastw : {nb, 1 + nb / 3})
      for (int BN : {128, 64})
        check_coverage(2 * nb + lastw, nb, 1, 1, 0, 0, 128, BN);
  const int grids[5][2] = {{1, 2}, {2, 1}, {2, 2}, {2, 3}, {3, 2}};
  for (int nb : {1, 2, 33, 48, 64, 65, 128, 129, 160})
    for (int lastw : {nb, 1 + nb / 2})
      for (int BN : {128, 64})
        for (const auto& g : grids)
          for (int isrc = 0; isrc < g[0]; ++isrc)
            for (int jsrc = 0; jsrc < g[1]; ++jsrc)
              check_coverage(4 * nb + lastw, nb, g[0], g[1], isrc, jsrc, 128, BN);
  for (int ld : {1, 2, 5, 33, 48, 64, 160, 200})
    check_forms(ld);
  check_panel_offsets();
  std::printf("elements %ld blocks %ld forms %ld failures %ld\n", g_elements, g_blocks, g_forms, g_failures);
  return g_failures == 0 ? 0 : 1;
}
