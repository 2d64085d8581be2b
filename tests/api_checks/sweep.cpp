// Sweep of the non-terminating parts of the C API's argument checks (csrc/host/api_checks.hpp) on the host, against a
// brute-force model written here from their definitions, not from the header's helpers:
//   letters   in_set and the is_* predicates over all 256 characters: c is in a set exactly when it is not NUL and equals
//             one of the set's letters, compared one by one;
//   sources   source_in_grid, both forms, over the grids 1 x 1 .. 3 x 3 and source coordinates in [-1, 3]: inside
//             exactly when (isrc, jsrc) is one of the grid's nprow x npcol coordinates, enumerated;
//   names     the offset list and the operand list a ScaLAPACK prologue composes for one, two and three operands.
// The terminating helpers (require_*) are pinned through the library by tests/test_c_api_preconditions.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "api_checks.hpp"

using namespace dlaf_mi355x;

// the header's fatal lives in the library (runtime.cpp); nothing swept here may reach it
void dlaf_mi355x::fatal(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
  std::abort();
}

static long g_letters = 0, g_sources = 0, g_names = 0, g_failures = 0;

static void fail(const char* what, long x, long y) {
  if (++g_failures <= 20)
    std::fprintf(stderr, "FAIL %s (%ld, %ld)\n", what, x, y);
}

static bool model_in_set(int c, const char* set, int len) {
  if (c == 0)
    return false;
  for (int k = 0; k < len; ++k)
    if ((unsigned char) set[k] == c)
      return true;
  return false;
}

struct LetterSet {
  const char* set;
  int len;
  bool (*pred)(char);
};

static void sweep_letters() {
  const LetterSet sets[] = {{"LlUu", 4, is_uplo}, {"Ll", 2, is_lower}, {"Uu", 2, is_upper}, {"LlRr", 4, is_side},
                            {"Ll", 2, is_left},   {"NnTtCc", 6, is_op}, {"NnUu", 4, is_diag}, {"HhSsTt", 6, nullptr},
                            {"Cc", 2, nullptr},   {"Tt", 2, nullptr},   {"", 0, nullptr}};
  for (const LetterSet& s : sets)
    for (int c = 0; c < 256; ++c) {
      const bool want = model_in_set(c, s.set, s.len);
      ++g_letters;
      if (in_set((char) c, s.set) != want)
        fail("in_set", c, s.len);
      if (s.pred && s.pred((char) c) != want)
        fail("predicate", c, s.len);
    }
}

struct ModelGrid {
  int nprow, npcol;
};

static void sweep_sources() {
  for (int nprow = 1; nprow <= 3; ++nprow)
    for (int npcol = 1; npcol <= 3; ++npcol)
      for (int isrc = -1; isrc <= 3; ++isrc)
        for (int jsrc = -1; jsrc <= 3; ++jsrc) {
          bool want = false;
          for (int r = 0; r < nprow; ++r)
            for (int c = 0; c < npcol; ++c)
              want = want || (r == isrc && c == jsrc);
          const DLAF_descriptor d = {6, 6, 2, 2, isrc, jsrc, 0, 0, 6};
          ++g_sources;
          if (source_in_grid(nprow, npcol, isrc, jsrc) != want)
            fail("source_in_grid(nprow, npcol, isrc, jsrc)", isrc, jsrc);
          if (source_in_grid(ModelGrid{nprow, npcol}, d) != want)
            fail("source_in_grid(grid, desc)", isrc, jsrc);
        }
}

static void expect(const std::string& got, const char* want) {
  ++g_names;
  if (got != want) {
    std::fprintf(stderr, "got '%s', want '%s'\n", got.c_str(), want);
    fail("composed names", (long) got.size(), 0);
  }
}

static void sweep_names() {
  const int desc[9] = {1, 7, 6, 6, 2, 2, 0, 0, 6};
  const ScalapackOperand a{'A', desc, 1, 1}, b{'B', desc, 1, 1}, c{'C', desc, 1, 1}, z{'Z', desc, 1, 1};
  expect(offset_names({a}), "ia, ja");
  expect(offset_names({a, b}), "ia, ja, ib, jb");
  expect(offset_names({a, z}), "ia, ja, iz, jz");
  expect(offset_names({a, b, c}), "ia, ja, ib, jb, ic, jc");
  expect(offset_names({a, b, z}), "ia, ja, ib, jb, iz, jz");
  expect(operand_names({a}), "A");
  expect(operand_names({a, z}), "A and Z");
  expect(operand_names({a, b, c}), "A, B and C");
  // a well-formed argument list passes the prologue and gives back its context
  ++g_names;
  if (require_scalapack_args({a, b, z}) != 7 || require_scalapack_args({a}, "routine") != 7)
    fail("require_scalapack_args context", 7, 0);
}

int main() {
  sweep_letters();
  sweep_sources();
  sweep_names();
  std::printf("letters %ld sources %ld names %ld failures %ld\n", g_letters, g_sources, g_names, g_failures);
  return g_failures == 0 ? 0 : 1;
}
