// Sweep of the address arithmetic of the direct-to-LDS K loop (csrc/device/glds_addr.hpp) on the host.  The loop forms
// the address of a load as  operand pointer of the slab's segment + base(wave, slab) + step(1) + .. + step(idx) + the
// lane's 32-bit offset; here every such address is compared with the closed form written from the LDS image: lane l of
// piece (wave N + idx) holds element e = (wave N + idx) EPP + l PER of the image [k][ROWS], which is row e % ROWS of
// column k0 + e / ROWS, byte 8 ((k0 + e / ROWS) ld + e % ROWS) of the operand, worked out in 128-bit integers.
//   * geometries: both operands of the update kernel (128 rows, 4 pieces per wave, different leading dimensions) and
//     the 64-row operand of the panel TRMM (a piece holds two columns: the lane offset carries ld);
//   * K = BK, 2 BK, 3 BK, 128 BK; every iteration kt of the loop, so every slab and the re-fetch of the last one;
//     the start slab s0 = 0 .. nk - 1 with wrap-around; one segment and two with K1 = BK, 3 BK, the second panel at a
//     LOWER address than the first and passed shifted back by K1 columns, as gemm_nt_block takes it;
//   * ld from 128 to 2^31 elements: byte offsets past 2^31 and 2^32 are counted and must occur.
// Pointers are plain 64-bit numbers, nothing is dereferenced.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "glds_addr.hpp"

using namespace dlaf_mi355x;

static long g_checks = 0, g_past31 = 0, g_past32 = 0, g_slabs = 0, g_failures = 0;
constexpr int BK = 16, NWAVES = 4, EPP = 128;

// the slab iteration kt loads, from the loop's contract: `ahead` slabs past the one it consumes, the last slab again
// once that is past the end, counted from s0 modulo nk
static int slab_expected(int kt, int ahead, int nk, int s0) {
  int t = kt + ahead;
  if (t > nk - 1)
    t = nk - 1;
  return (s0 + t) % nk;
}

template <int ROWS, int N>
static void check_slab(int kn, int K1, long long ld, std::uint64_t p1, std::uint64_t p2, bool all_lanes) {
  using P = GldsPieces<ROWS, EPP, N, 8>;
  if (!P::lane_fits(ld))
    return;
  const bool second = kn >= K1;
  // the pointer gemm_nt_block is handed for the second segment: shifted back by K1 columns
  const std::uint64_t shifted2 = p2 - (std::uint64_t) 8 * (std::uint64_t) K1 * (std::uint64_t) ld;
  const std::uint64_t operand = second ? shifted2 : p1;
  for (int wave = 0; wave < NWAVES; ++wave) {
    std::uint64_t piece = operand + (std::uint64_t) 8 * (std::uint64_t) P::base_elems(wave, kn, ld);
    for (int idx = 0; idx < N; ++idx) {
      if (idx > 0)
        piece += (std::uint64_t) P::step_bytes(idx, ld);
      for (int lane = 0; lane < 64; lane += all_lanes ? 1 : 63) {
        const std::uint64_t got = piece + P::lane_bytes(lane, ld);
        const long e = (long) (wave * N + idx) * EPP + lane * P::PER;
        const long row = e % ROWS, col = e / ROWS;
        // in the panel that holds the column: the first, or the second counted from its own column 0
        const __int128 off = (__int128) 8 * ((__int128) ((second ? kn - K1 : kn) + col) * ld + row);
        const std::uint64_t want = (second ? p2 : p1) + (std::uint64_t) off;
        ++g_checks;
        g_past31 += off > ((__int128) 1 << 31) ? 1 : 0;
        g_past32 += off > ((__int128) 1 << 32) ? 1 : 0;
        if (got != want && ++g_failures <= 20)
          std::fprintf(stderr, "FAIL rows=%d n=%d kn=%d K1=%d ld=%lld wave=%d idx=%d lane=%d: got %llx, expected %llx\n",
                       ROWS, N, kn, K1, ld, wave, idx, lane, (unsigned long long) got, (unsigned long long) want);
      }
    }
  }
}

int main() {
  // the second panel lies BELOW the first; both far enough from 0 and 2^64 for every offset of the sweep
  const std::uint64_t p1 = (std::uint64_t) 1 << 60, p2 = ((std::uint64_t) 1 << 59) + 4096;
  const long long lds_all[] = {128, 130, 136, 1024, 65538, 1LL << 20, (1LL << 28) + 2, 1LL << 29, (1LL << 29) + 2,
                               1LL << 30, (1LL << 31) - 2, 1LL << 31};
  const long long lds_few[] = {128, (1LL << 28) + 2, 1LL << 31};
  for (int nk : {1, 2, 3, 128})
    for (int s0 = 0; s0 < nk; ++s0)
      for (int kt = 0; kt < nk; ++kt) {
        const int sn = glds_slab_ahead(kt, 1, nk, s0);
        const int want = slab_expected(kt, 1, nk, s0);
        ++g_slabs;
        if (sn != want && ++g_failures <= 20)
          std::fprintf(stderr, "FAIL slab nk=%d s0=%d kt=%d: got %d, expected %d\n", nk, s0, kt, sn, want);
        // a deeper ring (the panel TRMM runs three stages)
        if (glds_slab_ahead(kt, 2, nk, s0) != slab_expected(kt, 2, nk, s0) && ++g_failures <= 20)
          std::fprintf(stderr, "FAIL slab ahead=2 nk=%d s0=%d kt=%d\n", nk, s0, kt);
        const int kn = sn * BK;
        // every lane and every ld where the slab count is small and, at 128 slabs, along s0 = 0 (every slab once);
        // the other start slabs of 128 repeat those slabs: first and last lane, three leading dimensions
        const bool full = nk <= 3 || s0 == 0;
        for (int K1 : {BK, 3 * BK, 1 << 30}) {
          // (K1 >= K: one segment, as for the caller that has no second panel)
          if (full)
            for (long long ld : lds_all) {
              const long long ldb = ld + 8 <= (1LL << 31) ? ld + 8 : ld - 8;
              check_slab<128, 4>(kn, K1, ld, p1, p2, true);        // operand A of the update kernel (lda)
              check_slab<128, 4>(kn, K1, ldb, p1 + 64, p2, true);  // operand B: another leading dimension (ldb)
              check_slab<64, 2>(kn, K1, ld, p1, p2, true);         // the 64-row operand of the panel TRMM
            }
          else
            for (long long ld : lds_few) {
              const long long ldb = ld + 8 <= (1LL << 31) ? ld + 8 : ld - 8;
              check_slab<128, 4>(kn, K1, ld, p1, p2, false);
              check_slab<128, 4>(kn, K1, ldb, p1 + 64, p2, false);
              check_slab<64, 2>(kn, K1, ld, p1, p2, false);
            }
        }
      }
  std::printf("addresses %ld slabs %ld past2^31 %ld past2^32 %ld failures %ld\n", g_checks, g_slabs, g_past31, g_past32,
              g_failures);
  return g_failures == 0 ? 0 : 1;
}
