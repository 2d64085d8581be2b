// Sweep of the panel TRSM's kernel choice (csrc/device/trsm_path.hpp) on the host: over nb, last_rows, n, the alignment
// of the three base pointers and of the strides, upper, the DLAF_MI355X_TRSM=strips switch and the four types, a
// row-owner kernel must be chosen only when every promise its comments rely on holds -- every tile a whole number of
// 64-row strips, n a whole number of macro blocks, L lower, every base and stride of B, L and winv 16-byte aligned, the
// type the kernel is written for -- and the strips kernel otherwise; the VEC flag of the strips kernel only when the
// bases and strides of B and L are 16-byte aligned.  The expectation is worked out here in bytes, promise by promise.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "trsm_path.hpp"

using namespace dlaf_mi355x;

struct Args {
  const char* b;
  long b_ts;
  int ldb;
  int nb, last_rows;
  const char* l;
  int ldl;
  const char* winv;
  int n;
  int upper;
};

static long g_sets = 0, g_rows = 0, g_failures = 0;
alignas(64) static char g_arena[256];

template <int BYTES, bool CX>
static void check(const Args& a, bool enabled) {
  ++g_sets;
  const TrsmChoice got = trsm_path<BYTES, CX>(a, enabled);
  auto a16 = [](const void* p) { return reinterpret_cast<std::uintptr_t>(p) % 16 == 0; };
  auto s16 = [](long stride) { return (stride * BYTES) % 16 == 0; };
  const bool vec = a16(a.b) && s16(a.ldb) && s16(a.b_ts) && a16(a.l) && s16(a.ldl);
  // every tile of the panel has nb rows or, the last global one, last_rows
  const bool strips64 = a.nb % 64 == 0 && a.last_rows % 64 == 0;
  const bool rows_ok = vec && a16(a.winv) && strips64 && !a.upper && enabled;
  TrsmPath want = TrsmPath::strips;
  if (rows_ok && BYTES == 8 && !CX && a.n % 256 == 0)
    want = TrsmPath::rows256;
  else if (rows_ok && BYTES == 8 && !CX && a.n % 128 == 0)
    want = TrsmPath::rows128;
  else if (rows_ok && BYTES == 16 && CX && a.n % 128 == 0)
    want = TrsmPath::rows_z128;
  if (want != TrsmPath::strips)
    ++g_rows;
  if (got.path != want || got.vec != vec) {
    if (++g_failures <= 20)
      std::fprintf(stderr,
                   "FAIL bytes=%d cx=%d nb=%d last_rows=%d n=%d ldb=%d b_ts=%ld ldl=%d upper=%d enabled=%d b%%16=%d "
                   "l%%16=%d w%%16=%d: got path %d vec %d, expected path %d vec %d\n",
                   BYTES, (int) CX, a.nb, a.last_rows, a.n, a.ldb, a.b_ts, a.ldl, a.upper, (int) enabled,
                   (int) (reinterpret_cast<std::uintptr_t>(a.b) % 16), (int) (reinterpret_cast<std::uintptr_t>(a.l) % 16),
                   (int) (reinterpret_cast<std::uintptr_t>(a.winv) % 16), (int) got.path, (int) got.vec, (int) want,
                   (int) vec);
  }
}

template <int BYTES, bool CX>
static void sweep() {
  for (int nb : {1, 17, 63, 64, 65, 128, 192, 200, 256, 320})
    for (int last_rows : {1, 37, 64, 65, 128, 192, nb}) {
      if (last_rows > nb)
        continue;
      for (int n : {1, 17, 64, 65, 127, 128, 130, 192, 256, 320, 384, 512, 640, 768})
        for (int boff = 0; boff < 3; ++boff)
          for (int loff = 0; loff < 3; ++loff)
            for (int woff = 0; woff < 3; ++woff)
              for (int dldb : {0, 1, 2, 4})
                for (int dts : {-1, 0, 1, 2})
                  for (int dldl : {0, 1, 2})
                    for (int upper = 0; upper <= 1; ++upper)
                      for (int enabled = 0; enabled <= 1; ++enabled) {
                        Args a;
                        a.b = g_arena + boff * BYTES;
                        a.l = g_arena + 64 + loff * BYTES;
                        a.winv = g_arena + 128 + woff * BYTES;
                        a.nb = nb;
                        a.last_rows = last_rows;
                        a.n = n;
                        a.ldb = nb + dldb;
                        a.b_ts = dts < 0 ? 0 : (long) a.ldb * n + dts;
                        a.ldl = n + dldl;
                        a.upper = upper;
                        check<BYTES, CX>(a, enabled != 0);
                      }
    }
}

int main() {
  sweep<4, false>();
  sweep<8, false>();
  sweep<8, true>();
  sweep<16, true>();
  std::printf("argument sets %ld row-owner %ld failures %ld\n", g_sets, g_rows, g_failures);
  return g_failures == 0 ? 0 : 1;
}
