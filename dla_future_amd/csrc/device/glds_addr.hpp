// glds_addr.hpp -- where the direct-to-LDS loads of the K loop (gemm_nt_block, mma_core.hpp; real types) read from.
// Plain C++ and nothing from HIP, so that a host program can sweep the arithmetic against its closed form
// (tests/glds_addr/sweep.cpp).
//
// A slab of one operand is the LDS image [k][ROWS], cut into pieces of EPP consecutive elements (one 1 KiB wave
// instruction each); wave w moves pieces w N .. w N + N - 1, lane l of a piece the 16 bytes at element e0 + l PER.
// Element e of the image is row e % ROWS of column k0 + e / ROWS, i.e. byte ELEM_BYTES ((k0 + e / ROWS) ld + e % ROWS)
// of the operand.  With pieces and columns nested that splits into
//   base(wave, k0)  wave-uniform, 64 bit, once per slab and operand: the first element of the wave's piece 0,
//   step(idx)       wave-uniform, 64 bit, does not depend on the slab: from piece idx - 1 to piece idx,
//   lane(l)         32 bit, does not depend on the slab or the piece,
// so a load is two scalar adds on the previous load's address and the instruction's own 32-bit lane offset.
#pragma once

#if defined(__HIPCC__)
#define DLAF_GLDS_HD __host__ __device__
#else
#define DLAF_GLDS_HD
#endif

namespace dlaf_mi355x {

// The slab whose loads iteration kt of the K loop issues: `ahead` slabs in front of the one it consumes, the last one
// again past the end (the UTAIL re-fetch), counted from the start slab s0 with wrap-around.  0 <= s0 < nk.
DLAF_GLDS_HD constexpr int glds_slab_ahead(int kt, int ahead, int nk, int s0) {
  const int t = kt + ahead < nk - 1 ? kt + ahead : nk - 1;
  const int sn = s0 + t;
  return sn >= nk ? sn - nk : sn;
}

template <int ROWS, int EPP, int N, int ELEM_BYTES>
struct GldsPieces {
  static constexpr int CPP = EPP >= ROWS ? EPP / ROWS : 1;  // columns per piece
  static constexpr int PPC = EPP >= ROWS ? 1 : ROWS / EPP;  // pieces per column
  static constexpr int PER = 16 / ELEM_BYTES;               // elements per lane
  static_assert(EPP >= ROWS ? EPP % ROWS == 0 : (ROWS % EPP == 0 && N % PPC == 0),
                "pieces and columns nest, and a wave's run of pieces starts at the top of a column");
  static_assert(EPP == 64 * PER, "one piece = 64 lanes x 16 bytes");

  // first element of the wave's piece 0 of the slab that starts at column k0, from the operand's pointer, in ELEMENTS
  // (the caller adds it to a typed pointer: the scaling to bytes then follows the product as a shift).  Column and ld
  // are both below 2^32 (k0 >= 0; ld <= 2^31 elements), so the product is ONE 32 x 32 -> 64 bit multiply; the byte
  // offset passes 2^31 and 2^32 freely.
  static DLAF_GLDS_HD constexpr long long base_elems(int wave, int k0, long long ld) {
    const unsigned column = (unsigned) (k0 + wave * (N / PPC) * CPP);
    return (long long) ((unsigned long long) column * (unsigned long long) (unsigned) ld);
  }
  // from the first byte of piece idx - 1 to that of piece idx (1 <= idx < N)
  static DLAF_GLDS_HD constexpr long long step_bytes(int idx, long long ld) {
    if (EPP >= ROWS)
      return (long long) ELEM_BYTES * CPP * ld;
    return (long long) ELEM_BYTES * (idx % PPC == 0 ? ld - (long long) (PPC - 1) * EPP : (long long) EPP);
  }
  // the lane's bytes past the first byte of its piece.  ROWS >= EPP: 16 l.  ROWS < EPP: the lanes of a piece spread
  // over CPP columns and the offset holds (CPP - 1) ld, which must fit (lane_fits).
  static DLAF_GLDS_HD constexpr unsigned lane_bytes(int lane, long long ld) {
    return (unsigned) ELEM_BYTES * ((unsigned) ((lane * PER) % ROWS) + (unsigned) ((lane * PER) / ROWS) * (unsigned) ld);
  }
  static DLAF_GLDS_HD constexpr bool lane_fits(long long ld) {
    return (long long) ELEM_BYTES * ((CPP - 1) * ld + ROWS) <= 0x7fffffffLL;
  }
};

}  // namespace dlaf_mi355x
