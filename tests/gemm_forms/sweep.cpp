// Sweep of the general multiplication kernel's operand forms (csrc/device/gemm_forms.hpp) on the host, over every op
// pair, tile size and ragged extent, every block origin, aligned and unaligned tile addresses and the four types:
//   * for every (m, k) and (n, k) of a block, the description gemm_form_a / gemm_form_b gives must address exactly the
//     element of op(A) / op(B) a brute-force model names -- every tile element holds its own (row, column) --, and the
//     conjugation flag must be the one that, under gemm_acc's convention  acc += a' * conj(b')  (a', b' the operands
//     AFTER a set flag has conjugated them), gives  a * op(B)(k, n)  with a = op(A)(m, k);
//   * gemm_loader_mode may name a vector loader only when every promise that loader relies on holds: the first element
//     of the block and every column of the tile on a 16-byte boundary, a whole block of rows, a whole number of BK
//     slabs -- and then it must be the loader of the form (rows contiguous for a stored row operand, k contiguous for a
//     stored k operand), whose 16-byte loads must stay inside the tile.
#include <complex>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "gemm_forms.hpp"

using namespace dlaf_mi355x;

static long g_elems = 0, g_modes = 0, g_vec = 0, g_failures = 0;

static void fail(const char* what, char op, int ld, int origin, int r, int k) {
  if (++g_failures <= 20)
    std::fprintf(stderr, "FAIL %s: op %c ld %d origin %d r %d k %d\n", what, op, ld, origin, r, k);
}

// a tile whose element (i, j) holds i + j * 1000 in the real part and 1 in the imaginary part
using Z = std::complex<double>;
static Z tile_value(int i, int j) {
  return Z((double) (i + 1000 * j), 1.0);
}

// what gemm_acc makes of the two operands: a' * conj(b') with the flagged ones conjugated first
static Z acc_term(Z a, int conj_a, Z b, int conj_b) {
  const Z a1 = conj_a ? std::conj(a) : a, b1 = conj_b ? std::conj(b) : b;
  return a1 * std::conj(b1);
}

static void check_addresses(int ld) {
  std::vector<Z> ta((size_t) ld * ld), tb((size_t) ld * ld);
  for (int j = 0; j < ld; ++j)
    for (int i = 0; i < ld; ++i) {
      ta[(size_t) i + (size_t) j * ld] = tile_value(i, j);
      tb[(size_t) i + (size_t) j * ld] = tile_value(j, i) * Z(0.5, -2.0);  // something else, not Hermitian to ta
    }
  auto opv = [&](const std::vector<Z>& t, char op, int i, int j) {  // op(T)(i, j)
    if (gemm_op_is_n(op))
      return t[(size_t) i + (size_t) j * ld];
    const Z v = t[(size_t) j + (size_t) i * ld];
    return gemm_op_is_c(op) ? std::conj(v) : v;
  };
  for (char opa : {'N', 'T', 'C', 'n', 't', 'c'})
    for (char opb : {'N', 'T', 'C', 'n', 't', 'c'})
      for (int origin : {0, 1, 7, 16, 64, 128})
        for (int r = 0; origin + r < ld; r += (r < 3 ? 1 : 5))
          for (int k = 0; k < ld; k += (k < 3 ? 1 : 7)) {
            ++g_elems;
            const GemmForm fa = gemm_form_a(opa, ld, origin), fb = gemm_form_b(opb, ld, origin);
            const long ia = fa.off + r * fa.rs + k * fa.ks, ib = fb.off + r * fb.rs + k * fb.ks;
            if (ia < 0 || ia >= (long) ld * ld || ib < 0 || ib >= (long) ld * ld) {
              fail("address outside the tile", opa, ld, origin, r, k);
              continue;
            }
            // op(A)(origin + r, k) and op(B)(k, origin + r) as the model names them
            const Z a_want = opv(ta, opa, origin + r, k), b_want = opv(tb, opb, k, origin + r);
            const Z a_got = fa.conj ? std::conj(ta[(size_t) ia]) : ta[(size_t) ia];
            if (a_got != a_want)
              fail("A element or flag", opa, ld, origin, r, k);
            if (acc_term(ta[(size_t) ia], fa.conj, tb[(size_t) ib], fb.conj) != a_want * b_want)
              fail("B element or flag", opb, ld, origin, r, k);
            // the loader of the form: the unit stride it names
            if ((fa.vmode == 0 && fa.rs != 1) || (fa.vmode == 1 && fa.ks != 1) || (fb.vmode == 0 && fb.rs != 1) ||
                (fb.vmode == 1 && fb.ks != 1) || fa.vmode < 0 || fa.vmode > 1 || fb.vmode < 0 || fb.vmode > 1)
              fail("vector loader of the form", opa, ld, origin, r, k);
          }
}

alignas(64) static char g_arena[64];

template <int BYTES>
static void check_modes() {
  constexpr int VE = 16 / BYTES;
  for (int ld : {1, 2, 3, 8, 16, 33, 48, 64, 128, 130, 160, 256})
    for (int rows_block : {64, 128})
      for (int BK : {8, 16})
        for (int origin = 0; origin < ld; origin += rows_block)
          for (int rows_valid : {1, 31, 32, 63, 64, 127, 128})
            for (int K : {0, 1, 7, 8, 15, 16, 24, 32, 33, ld})
              for (int shift = 0; shift < 4; ++shift)
                for (char op : {'N', 'T', 'C'})
                  for (int side = 0; side < 2; ++side) {
                    if (rows_valid > rows_block || origin + rows_valid > ld || K > ld)
                      continue;
                    ++g_modes;
                    const char* tile = g_arena + shift * BYTES;  // shift elements off a 64-byte boundary
                    const GemmForm f = side == 0 ? gemm_form_a(op, ld, origin) : gemm_form_b(op, ld, origin);
                    const int mode = gemm_loader_mode<BYTES>(f, tile, ld, rows_valid, rows_block, K, BK);
                    const std::uintptr_t first = reinterpret_cast<std::uintptr_t>(tile) + (std::uintptr_t) f.off * BYTES;
                    const bool promises = first % 16 == 0 && ((long) ld * BYTES) % 16 == 0 && rows_valid == rows_block &&
                                          K > 0 && K % BK == 0;
                    if (mode != (promises ? f.vmode : 2)) {
                      fail("loader mode", op, ld, origin, rows_valid, K);
                      continue;
                    }
                    if (mode == 2)
                      continue;
                    ++g_vec;
                    // every 16-byte load of the vector loader: aligned and inside the ld x ld tile
                    for (int r = 0; r < rows_valid; r += (mode == 0 ? VE : 1))
                      for (int k = 0; k < K; k += (mode == 1 ? VE : 1)) {
                        const long e = f.off + r * f.rs + k * f.ks;
                        const std::uintptr_t at = reinterpret_cast<std::uintptr_t>(tile) + (std::uintptr_t) e * BYTES;
                        if (at % 16 != 0 || e < 0 || e + VE > (long) ld * ld)
                          fail("vector load misaligned or outside the tile", op, ld, origin, r, k);
                      }
                  }
}

int main() {
  for (int ld : {1, 2, 5, 33, 48, 64, 160, 200})
    check_addresses(ld);
  check_modes<4>();
  check_modes<8>();
  check_modes<16>();
  std::printf("elements %ld modes %ld vector %ld failures %ld\n", g_elems, g_modes, g_vec, g_failures);
  return g_failures == 0 ? 0 : 1;
}
