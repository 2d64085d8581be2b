// mma_core.hpp -- the workgroup-level MFMA GEMM core shared by the trailing-update and the
// panel-TRSM kernels:   acc(BM x BN) += A(BM x K) * B(BN x K)^H
// A, B column-major in global memory; slabs of BK columns are staged global -> registers -> LDS
// (double-buffered, one barrier per slab) and consumed as 16x16x4 MFMA fragments.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "glds_addr.hpp"

namespace dlaf_mi355x {

// PAIRED_ (real types): MFMA tiles 2q and 2q+1 of a wave hold the even / odd rows of a 32-row group,
// so one 16-byte LDS read feeds two fragments and the epilogue moves two consecutive rows per lane
// (16-byte global accesses).  With it the LDS image is unpadded ([k][ROWS], column stride = 0 mod
// 256 B is what ds_read_b128's lane groups want) and, for fp64 with 128-row slabs, a slab column is
// exactly one 1 KiB global_load_lds_dwordx4 -- the direct-to-LDS staging of the fast path.
// STAGES_: LDS slab buffers.  2 = classic double buffering; the direct-to-LDS path uses more so that
// STAGES-1 slabs are in flight (counted s_waitcnt vmcnt + raw s_barrier) and HBM/L2 latency spikes
// do not stall the MFMA stream.
template <class T, int BM_, int BN_, int WM_, int WN_, int BK_, bool PAIRED_ = false, int STAGES_ = 2,
          int THREADS_ = kThreads>
struct BlockCfg {
  using R = real_t<T>;
  static constexpr bool CX = TypeInfo<T>::is_complex;
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, BK = BK_;
  static constexpr int THREADS = THREADS_, NWAVES = THREADS_ / 64;
  static constexpr int TM = WM / 16, TN = WN / 16;
  static constexpr int WAVES_M = BM / WM, WAVES_N = BN / WN;
  static_assert(WAVES_M * WAVES_N == NWAVES, "the wave tiles must cover the block");
  static_assert(BK % 4 == 0 && WM % 16 == 0 && WN % 16 == 0, "MFMA 16x16x4 granularity");
  // For complex types PAIRED_ selects the interleaved LDS image instead ([k][ROWS] of (re, im)): one
  // ds_read_b128 per fragment and, with 64-row granularity, direct-to-LDS staging of 16-byte elements.
  static constexpr bool PAIRED = PAIRED_ && !CX;
  static constexpr bool CXI = PAIRED_ && CX;
  static_assert(!PAIRED || (TM % 2 == 0 && TN % 2 == 0), "paired rows: even tile counts");
  static constexpr int PAD = PAIRED_ ? 0 : kLdsPad;
  static constexpr int LDA = BM + PAD, LDB = BN + PAD;
  // direct-to-LDS staging: one wave instruction (64 lanes x 16 B = 1 KiB, contiguous in LDS) moves one PIECE
  // of the unpadded image [k][ROWS]: EPP consecutive elements = a run of whole columns (ROWS <= EPP) or a
  // part of one column (ROWS > EPP); every wave issues the same number of them per slab
  static constexpr int EPP = CX ? 64 : 1024 / (int) sizeof(T);
  static constexpr int PIECES_A = BK * BM / EPP, PIECES_B = BK * BN / EPP;
  static constexpr bool GLDS =
      (PAIRED && (EPP % BM == 0 || BM % EPP == 0) && (EPP % BN == 0 || BN % EPP == 0) && (BK * BM) % EPP == 0 &&
       (BK * BN) % EPP == 0 && PIECES_A % NWAVES == 0 && PIECES_B % NWAVES == 0) ||
      (CXI && sizeof(T) == 16 && BM % 64 == 0 && BN % 64 == 0 && PIECES_A % NWAVES == 0 && PIECES_B % NWAVES == 0);
  static constexpr int LPS = PIECES_A / NWAVES + PIECES_B / NWAVES;  // direct-to-LDS loads per wave and slab
  static constexpr int A_PLANE = BK * LDA, B_PLANE = BK * LDB;
  static constexpr int A_ELEMS = (CX ? 2 : 1) * A_PLANE, B_ELEMS = (CX ? 2 : 1) * B_PLANE;
  static constexpr int BUF_ELEMS = A_ELEMS + B_ELEMS;
  static constexpr int STAGES = STAGES_;
  static_assert(STAGES >= 2 && STAGES <= 6, "2..6 LDS stages");
  static constexpr int LDS_BYTES = STAGES * BUF_ELEMS * (int) sizeof(R);
};

template <class Cfg>
struct Acc {
  using R = typename Cfg::R;
  using acc_t = typename Mma<R>::acc_t;
  acc_t re[Cfg::TM][Cfg::TN];
  acc_t im[Cfg::CX ? Cfg::TM : 1][Cfg::CX ? Cfg::TN : 1];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j) {
        re[i][j] = acc_t{0, 0, 0, 0};
        if constexpr (Cfg::CX)
          im[i][j] = acc_t{0, 0, 0, 0};
      }
  }
};

// one BK-slab of MFMAs out of the LDS images As ([k][LDA], planes re|im) and Bs ([k][LDB])
struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};

// ---- the rotated slab (fp64, paired rows, 4 x 4 MFMA tiles per wave) -----------------------------------------------
// A k-step of such a wave is 16 MFMAs out of four 16-byte fragment pairs: A0 = rows (0, 1), A1 = rows (2, 3),
// B0 = columns (0, 1), B1 = columns (2, 3).  Read "all four pairs, wait for all, 16 MFMAs" (the generic loop of
// mma_slab as hipcc compiles it) leaves the LDS latency of every step uncovered but for the 64 cycles of the previous
// step's last MFMA.  Here the four quadrants (B pair x A pair, 4 MFMAs each) of a step run in serpentine order, and
// the order of the A pairs alternates from step to step (F = the pair used first and last, S = the one between):
//     Q1 (B0, F)   Q2 (B0, S) -> read B0'   Q3 (B1, S) -> read S'   Q4 (B1, F) -> read F', B1'
//     next step: F := S', S := F'
// so every pair is re-read into the registers it has just vacated, at least 4 MFMAs (256 cycles) before its first
// use: 16 fragment registers, as before.  Every accumulator still receives its products in ascending k from the same
// instruction with the same inputs: the results are bit for bit those of the generic loop.
//
// The reads are inline assembly because hipcc waits for ALL of its own LDS reads before the first MFMA of a step
// (s_waitcnt lgkmcnt(0)), including the two issued a moment ago; the waits here are counted.  LDS reads return in
// order, so with the issue order  B0, F, S, B1  of the pairs a step consumes, "lgkmcnt(2)" before Q1 leaves S and B1
// in flight, "lgkmcnt(1)" before Q2 leaves B1, and before Q3 "lgkmcnt(1)" leaves the B0' issued after Q2 (0 in the
// last step, which reads nothing).  Other LDS or scalar-memory operations of the wave in between only raise the
// counter, i.e. make a wait stricter.  hipcc does not know when such a read lands: each wait names the pairs it
// retires as "+v" operands, so no consumer can be scheduled above it, and the sched_barrier after each quadrant pins
// the reads between the MFMAs.
//
// Invariants of the ring this slab is read from (a violation is a timing-dependent wrong result, not a crash):
//  (i)   a wave's reads of a ring slot have all retired before it enters the barrier after which any wave may issue
//        DMA (or stores) into that slot: the last step of the slab waits with lgkmcnt(0) before its third quadrant and
//        reads nothing afterwards, so the slab returns with no read in flight, whatever the caller waits for;
//  (ii)  no read of the next slab is issued before the barrier that follows every wave's vmcnt wait for that slab: the
//        first read of a slab is the first statement of this function, which the caller reaches only past that barrier
//        (asm volatile statements and the barrier keep their program order);
//  (iii) when hipcc hoists that barrier in front of the MFMAs of the last quadrant (it may: no sched_barrier follows
//        them), those MFMAs read registers only -- all four pairs were retired by (i).
typedef double lds_pair_d __attribute__((ext_vector_type(2)));

template <int OFF>
__device__ __forceinline__ void lds_read_pair_async(lds_pair_d& v, unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536 && OFF % 16 == 0, "ds_read_b128: 16-bit unsigned offset, 16-byte aligned");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
}
// at most N of this wave's LDS reads remain in flight afterwards; x (and y) are the pairs this retires
template <int N>
__device__ __forceinline__ void lds_wait_pairs(lds_pair_d& x, lds_pair_d& y) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(x), "+v"(y) : "i"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lds_wait_pairs(lds_pair_d& x) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(x) : "i"(N) : "memory");
}

template <class Cfg>
inline constexpr bool kRotatedSlab = Cfg::PAIRED && Cfg::TM == 4 && Cfg::TN == 4 && sizeof(typename Cfg::R) == 8 &&
                                     (Cfg::BK / 4) % 2 == 0;

// the 4 MFMAs of quadrant (B pair jp, A pair ip)
template <class Cfg, bool NEG>
__device__ __forceinline__ void mma_quadrant(Acc<Cfg>& acc, int jp, int ip, const lds_pair_d& b, const lds_pair_d& a) {
#pragma unroll
  for (int jj = 0; jj < 2; ++jj)
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      auto& d = acc.re[2 * ip + ii][2 * jp + jj];
      if constexpr (!NEG)
        d = Mma<double>::mma(b[jj], a[ii], d);
      else
        d = Mma<double>::mma_neg(b[jj], a[ii], d);
    }
}

// step K4 of the slab and, recursively, the ones after it.  On entry the reads of b0, a[F], a[S], b1 for this step
// are in flight in that order (F = K4 odd ? 1 : 0, S = 1 - F).  hook(4 K4 + quadrant) keeps the 16 hook points of the
// generic loop.
template <class Cfg, bool NEG, int K4, class Hook>
__device__ __forceinline__ void mma_slab_rotated_step(unsigned a_addr, unsigned b_addr, Acc<Cfg>& acc, lds_pair_d (&a)[2],
                                                      lds_pair_d& b0, lds_pair_d& b1, Hook& hook) {
  constexpr int NS = Cfg::BK / 4;
  constexpr bool NEXT = K4 + 1 < NS;
  constexpr int F = K4 & 1, S = 1 - F;
  // byte offsets of step K4 + 1 from the lane's address of step 0 (image [k][ROWS], 4 k per step, 32 rows per pair)
  constexpr int KN = NEXT ? K4 + 1 : 0;
  constexpr int AOFF = 8 * (KN * 4 * Cfg::LDA), BOFF = 8 * (KN * 4 * Cfg::LDB);

  hook(4 * K4 + 0);
  lds_wait_pairs<2>(b0, a[F]);
  mma_quadrant<Cfg, NEG>(acc, 0, F, b0, a[F]);
  __builtin_amdgcn_sched_barrier(0);

  hook(4 * K4 + 1);
  lds_wait_pairs<1>(a[S]);
  mma_quadrant<Cfg, NEG>(acc, 0, S, b0, a[S]);
  if constexpr (NEXT)
    lds_read_pair_async<BOFF>(b0, b_addr);
  __builtin_amdgcn_sched_barrier(0);

  hook(4 * K4 + 2);
  lds_wait_pairs<NEXT ? 1 : 0>(b1);
  mma_quadrant<Cfg, NEG>(acc, 1, S, b1, a[S]);
  if constexpr (NEXT)
    lds_read_pair_async<AOFF + 8 * 32 * S>(a[S], a_addr);
  __builtin_amdgcn_sched_barrier(0);

  hook(4 * K4 + 3);
  mma_quadrant<Cfg, NEG>(acc, 1, F, b1, a[F]);
  if constexpr (NEXT) {
    lds_read_pair_async<AOFF + 8 * 32 * F>(a[F], a_addr);
    lds_read_pair_async<BOFF + 8 * 32>(b1, b_addr);
    __builtin_amdgcn_sched_barrier(0);
    mma_slab_rotated_step<Cfg, NEG, K4 + 1>(a_addr, b_addr, acc, a, b0, b1, hook);
  }
}

template <class Cfg, bool NEG, class Hook>
__device__ __forceinline__ void mma_slab_rotated(const double* __restrict__ As, const double* __restrict__ Bs,
                                                 Acc<Cfg>& acc, int wm, int wn, int lane, Hook& hook) {
  static_assert(kRotatedSlab<Cfg> && Cfg::PAD == 0, "fp64, paired rows, 4 x 4 tiles, an even number of k-steps");
  const int g = lane >> 4, c = lane & 15;
  // LDS byte addresses of this lane's pair 0 at k-step 0: element [g][wave tile + 2 c]
  const unsigned a_addr = (unsigned) (uintptr_t) (const __attribute__((address_space(3))) double*) As +
                          8u * (unsigned) (g * Cfg::LDA + wm * Cfg::WM + 2 * c);
  const unsigned b_addr = (unsigned) (uintptr_t) (const __attribute__((address_space(3))) double*) Bs +
                          8u * (unsigned) (g * Cfg::LDB + wn * Cfg::WN + 2 * c);
  lds_pair_d a[2], b0, b1;
  lds_read_pair_async<0>(b0, b_addr);
  lds_read_pair_async<0>(a[0], a_addr);
  lds_read_pair_async<8 * 32>(a[1], a_addr);
  lds_read_pair_async<8 * 32>(b1, b_addr);
  __builtin_amdgcn_sched_barrier(0);
  mma_slab_rotated_step<Cfg, NEG, 0>(a_addr, b_addr, acc, a, b0, b1, hook);
}

// hook(p) is called before each group of TM MFMAs (p = k4 * TN + j counts the groups of a slab): the
// direct-to-LDS pipeline issues its loads of a later slab there, one at a time in the shadow of the MFMAs,
// instead of as one block at the head of the iteration (8 x global_load_lds back to back keep the wave from
// issuing MFMAs for ~1k cycles per slab; measured with in-kernel cycle stamps)
// NEG: acc -= A B^H instead of += (the accumulators were preloaded with the block the product is subtracted from)
template <class Cfg, bool NEG = false, class Hook = NoHook>
__device__ __forceinline__ void mma_slab(const typename Cfg::R* __restrict__ As,
                                         const typename Cfg::R* __restrict__ Bs, Acc<Cfg>& acc, int wm,
                                         int wn, int lane, Hook&& hook = Hook{}) {
  using R = typename Cfg::R;
  if constexpr (kRotatedSlab<Cfg>) {
    mma_slab_rotated<Cfg, NEG>(As, Bs, acc, wm, wn, lane, hook);
    return;
  }
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int k4 = 0; k4 < Cfg::BK / 4; ++k4) {
    const int kk = k4 * 4 + g;
    R a_re[Cfg::TM], a_im[Cfg::TM], b_re[Cfg::TN], b_im[Cfg::TN];
    if constexpr (Cfg::CXI) {
      typedef R r2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i) {
        const r2 v = *reinterpret_cast<const r2*>(&As[2 * (kk * Cfg::LDA + wm * Cfg::WM + i * 16 + c)]);
        a_re[i] = v[0];
        a_im[i] = v[1];
      }
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j) {
        const r2 v = *reinterpret_cast<const r2*>(&Bs[2 * (kk * Cfg::LDB + wn * Cfg::WN + j * 16 + c)]);
        b_re[j] = v[0];
        b_im[j] = v[1];
      }
    }
    else if constexpr (Cfg::PAIRED) {
      typedef R r2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int q = 0; q < Cfg::TM / 2; ++q) {
        const r2 v = *reinterpret_cast<const r2*>(&As[kk * Cfg::LDA + wm * Cfg::WM + q * 32 + 2 * c]);
        a_re[2 * q] = v[0];
        a_re[2 * q + 1] = v[1];
      }
#pragma unroll
      for (int q = 0; q < Cfg::TN / 2; ++q) {
        const r2 v = *reinterpret_cast<const r2*>(&Bs[kk * Cfg::LDB + wn * Cfg::WN + q * 32 + 2 * c]);
        b_re[2 * q] = v[0];
        b_re[2 * q + 1] = v[1];
      }
    }
    else {
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i) {
        a_re[i] = As[kk * Cfg::LDA + wm * Cfg::WM + i * 16 + c];
        if constexpr (Cfg::CX)
          a_im[i] = As[Cfg::A_PLANE + kk * Cfg::LDA + wm * Cfg::WM + i * 16 + c];
      }
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j) {
        b_re[j] = Bs[kk * Cfg::LDB + wn * Cfg::WN + j * 16 + c];
        if constexpr (Cfg::CX)
          b_im[j] = Bs[Cfg::B_PLANE + kk * Cfg::LDB + wn * Cfg::WN + j * 16 + c];
      }
    }
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      hook(k4 * Cfg::TN + j);
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i) {
        // D[i' = n][j' = m]: Aop <- B panel fragment, Bop <- A panel fragment
        if constexpr (!NEG) {
          acc.re[i][j] = Mma<R>::mma(b_re[j], a_re[i], acc.re[i][j]);
          if constexpr (Cfg::CX) {
            // (ar + i ai)(br - i bi) = (ar br + ai bi) + i (ai br - ar bi)
            acc.re[i][j] = Mma<R>::mma(b_im[j], a_im[i], acc.re[i][j]);
            acc.im[i][j] = Mma<R>::mma(b_re[j], a_im[i], acc.im[i][j]);
            acc.im[i][j] = Mma<R>::mma_neg(b_im[j], a_re[i], acc.im[i][j]);  // (f64: the MFMA's own negate bit)
          }
        }
        else {
          acc.re[i][j] = Mma<R>::mma_neg(b_re[j], a_re[i], acc.re[i][j]);
          if constexpr (Cfg::CX) {
            acc.re[i][j] = Mma<R>::mma_neg(b_im[j], a_im[i], acc.re[i][j]);
            acc.im[i][j] = Mma<R>::mma_neg(b_re[j], a_im[i], acc.im[i][j]);
            acc.im[i][j] = Mma<R>::mma(b_im[j], a_re[i], acc.im[i][j]);
          }
        }
      }
    }
  }
}

// Row (m) / column (n) inside the wave tile that accumulator element (tile i or j, lane, register v)
// stands for.  m lives on the lane's low 4 bits, n on the MFMA "i" index irow(g, v).
template <class Cfg>
__device__ __forceinline__ int acc_m(int i, int c) {
  if constexpr (Cfg::PAIRED)
    return (i >> 1) * 32 + 2 * c + (i & 1);
  else
    return i * 16 + c;
}
template <class Cfg>
__device__ __forceinline__ int acc_n(int j, int g, int v) {
  using R = typename Cfg::R;
  if constexpr (Cfg::PAIRED)
    return (j >> 1) * 32 + 2 * Mma<R>::irow(g, v) + (j & 1);
  else
    return j * 16 + Mma<R>::irow(g, v);
}

// Direct-to-LDS staging of one BK slab of A and B (Cfg::GLDS): the image of each panel is cut into 1 KiB
// pieces (one global_load_lds_dwordx4 each), wave w moves a contiguous run of them.
template <class Cfg, class T>
__device__ __forceinline__ void stage_glds(const T* __restrict__ A, long lda, const T* __restrict__ B, long ldb, int k0,
                                           typename Cfg::R* __restrict__ buf, int wave, int lane) {
  constexpr int NA = Cfg::PIECES_A / Cfg::NWAVES, NB = Cfg::PIECES_B / Cfg::NWAVES;  // instructions per wave
  constexpr int QA0 = 0, QA1 = NA, QB0 = 0, QB1 = NB;
  if constexpr (Cfg::CXI) {
    // 16-byte elements: one instruction moves 64 rows of one column; wave w takes every NWAVES-th piece
    constexpr int PA = Cfg::BM / 64, PB = Cfg::BN / 64;
#pragma unroll
    for (int idx = QA0; idx < QA1; ++idx) {
      const int piece = wave + Cfg::NWAVES * idx;
      const int k = piece / PA, part = piece % PA;
      const T* ga = A + part * 64 + lane + (long) (k0 + k) * lda;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*) ga,
                                       (__attribute__((address_space(3))) void*) (buf + 2 * (k * Cfg::LDA + part * 64)),
                                       16, 0, 0);
    }
#pragma unroll
    for (int idx = QB0; idx < QB1; ++idx) {
      const int piece = wave + Cfg::NWAVES * idx;
      const int k = piece / PB, part = piece % PB;
      const T* gb = B + part * 64 + lane + (long) (k0 + k) * ldb;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) gb,
          (__attribute__((address_space(3))) void*) (buf + Cfg::A_ELEMS + 2 * (k * Cfg::LDB + part * 64)), 16, 0, 0);
    }
    return;
  }
  constexpr int PER = 16 / (int) sizeof(T);  // elements per lane
  constexpr int EPP = Cfg::EPP;              // elements per piece
#pragma unroll
  for (int q = QA0; q < QA1; ++q) {
    const int e0 = (wave * NA + q) * EPP;    // first element of the piece in the image [k][BM]
    const int e = e0 + lane * PER;
    const T* ga = A + (e % Cfg::BM) + (long) (k0 + e / Cfg::BM) * lda;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*) ga,
                                     (__attribute__((address_space(3))) void*) (buf + e0), 16, 0, 0);
  }
#pragma unroll
  for (int q = QB0; q < QB1; ++q) {
    const int e0 = (wave * NB + q) * EPP;
    const int e = e0 + lane * PER;
    const T* gb = B + (e % Cfg::BN) + (long) (k0 + e / Cfg::BN) * ldb;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*) gb,
                                     (__attribute__((address_space(3))) void*) (buf + Cfg::A_ELEMS + e0), 16, 0, 0);
  }
}

// One direct-to-LDS load of the pipelined loop (real types): 64 lanes x 16 bytes, from `piece` (wave-uniform: a scalar
// register pair) plus the lane's 32-bit byte offset, into the 1 KiB at `dst`.  The address arithmetic is GldsPieces
// (glds_addr.hpp).  The empty statement makes the offset opaque where the load stands, so that its zero-extension is
// formed beside the load instead of once, as a 64-bit value, in front of the K loop: hipcc selects the instruction's
// (scalar base + 32-bit VGPR offset) form only when it finds the extension in the load's own block, and otherwise
// spends a 64-bit vector add and two more registers on every load (profiles/kloop_slab_bases_isa.txt).  The offset
// is passed by reference so that the statement rewrites the caller's register in place: no copy per load.
template <class R>
__device__ __forceinline__ void glds_load_piece(const char* piece, unsigned& lane_off, R* dst) {
  asm volatile("" : "+v"(lane_off));
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*) (piece + lane_off),
                                   (__attribute__((address_space(3))) void*) dst, 16, 0, 0);
}

// The group of MFMAs (hook point p of mma_slab) in front of which the pipelined loop issues the I-th load of a slab.
// Rotated slab: hook point 0 stands in the slab's exposed head -- between the slab barrier and the first MFMA, behind
// the four first-step fragment reads -- so the loads go out in front of groups 1 .. LPS instead of 0 .. LPS - 1.
// Measured (profiles/kloop_slab_bases_ab.txt): one-block-per-workgroup launches +0.65 %, persistent ones unchanged; a
// spread that also avoids the groups followed by two fragment re-reads (1 2 4 5 6 8 9 10) measured the same.
template <class Cfg>
__device__ __host__ constexpr int glds_hook_of(int i) {
  return kRotatedSlab<Cfg> ? i + 1 : i;
}

// acc += A(mrows x K) * B(ncols x K)^H for one BM x BN block.  lds: 2 * BUF_ELEMS of R.
// EDGE: rows >= mrows / ncols and k >= K are zero-filled; otherwise mrows == BM, ncols == BN and
// K % BK == 0 are the caller's promise.  All threads of the workgroup must call it.
// Two-segment form: columns k >= K1 of both operands come from A2 / B2 (same leading dimensions): the
// product of two panels applied in one pass (K = K1 + K2, one epilogue), or the two products of a her2k.
// A2 / B2 are passed already shifted back by K1 columns, K1 is a multiple of BK; K1 >= K: one segment.
// UTAIL (direct-to-LDS path): the K loop issues loads in EVERY iteration -- past the end the last slab is fetched
// again into the ring slot consumed an iteration ago, never read, drained after the loop -- so the loop body has
// no branch around the loads and one wait count.  Measured on the persistent bulk launches (fp64, 480 workgroups):
// 65.7 -> 67.0 TFlop/s at K = 1024, 66.2 -> 67.4 at K = 2048; on one-block-per-workgroup launches it costs 8 %
// (the drain delays the epilogue), so only the bulk instantiation of the update kernel asks for it.
template <class Cfg, class T, bool VEC, bool EDGE, bool UTAIL = false, bool NEG = false>
__device__ __forceinline__ void gemm_nt_block(const T* __restrict__ A, long lda, int mrows,
                                              const T* __restrict__ B, long ldb, int ncols, int K,
                                              typename Cfg::R* __restrict__ lds, Acc<Cfg>& acc, int K1 = 1 << 30,
                                              const T* __restrict__ A2 = nullptr,
                                              const T* __restrict__ B2 = nullptr, int s0 = 0) {
  using R = typename Cfg::R;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar address math
  const int wm = wave % Cfg::WAVES_M, wn = wave / Cfg::WAVES_M;
  const int nk = (K + Cfg::BK - 1) / Cfg::BK;
  if (nk == 0)
    return;
  if constexpr (Cfg::GLDS && VEC && !EDGE) {
    // multi-stage direct-to-LDS pipeline: slabs kt+1 .. kt+STAGES-1 are in flight while slab kt is
    // consumed.  Each wave issues LPS loads per slab; "vmcnt(LPS*(STAGES-2))" therefore means "my share
    // of slab kt+1 has landed", and the raw barrier extends that to every wave's share.
    constexpr int ST = Cfg::STAGES;
    constexpr int LPS = Cfg::LPS;
    static_assert(LPS * (ST - 2) < 64, "vmcnt is a 6-bit counter");
    // s0 (direct-to-LDS path): the slab the sum over k STARTS at; the loop walks s0, s0+1, .., nk-1, 0, .., s0-1.
    // The order of the sum is free, and a caller that starts every block at "the slab the others are at right
    // now" keeps the blocks that share operand strips at the same k -- see update_kernel.  0 <= s0 < nk.
#pragma unroll
    for (int s = 0; s < ST - 1; ++s)
      if (s < nk) {
        int sl = s0 + s;
        sl = sl >= nk ? sl - nk : sl;
        stage_glds<Cfg, T>(sl * Cfg::BK < K1 ? A : A2, lda, sl * Cfg::BK < K1 ? B : B2, ldb, sl * Cfg::BK,
                           lds + s * Cfg::BUF_ELEMS, wave, lane);
      }
    // slab 0 must be complete: everything but the younger (ST-2) slabs
    if (nk >= ST - 1)
      __builtin_amdgcn_s_waitcnt(0x0070 | ((LPS * (ST - 2)) & 0xF) | ((((LPS * (ST - 2)) >> 4) & 0x3) << 14));
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    int cur_i = 0, nxt_i = ST - 1;
    // The loads of slab kt+ST-1 are issued INSIDE the MFMA stream of slab kt, one instruction per group of TM
    // MFMAs over the first groups of the slab, instead of as a block of LPS instructions at the head of the
    // iteration.  Measured (profiles/r02_update_kernel_kloop_ab_timing.txt, fp64): persistent launches 65.7 -> 67.0
    // TFlop/s at K = 1024, 66.2 -> 67.4 at K = 2048, 60.4 -> 61.5 at nb = 512.  The last ST-1 iterations load nothing.
    constexpr bool SPLIT = !Cfg::CXI && LPS <= (Cfg::BK / 4) * Cfg::TN && LPS <= 16;
    if constexpr (!SPLIT) {
      // (complex types, or more loads than MFMA groups: the loads of a slab as one block at the head of the iteration)
      for (int kt = 0; kt < nk; ++kt) {
        R* cur = lds + cur_i * Cfg::BUF_ELEMS;
        const bool load = UTAIL || (kt + ST - 1 < nk);
        int sn = s0 + min(kt + ST - 1, nk - 1);
        sn = sn >= nk ? sn - nk : sn;
        const int kn = sn * Cfg::BK;
        const T* An = kn < K1 ? A : A2;
        const T* Bn = kn < K1 ? B : B2;
        R* nbuf = lds + nxt_i * Cfg::BUF_ELEMS;
        if (load)
          stage_glds<Cfg, T>(An, lda, Bn, ldb, kn, nbuf, wave, lane);
        mma_slab<Cfg, NEG>(cur, cur + Cfg::A_ELEMS, acc, wm, wn, lane);
        // slab kt+1 landed?  still in flight afterwards: the loads of slabs kt+2 .. kt+ST-1 (none in the tail)
        if (load)
          __builtin_amdgcn_s_waitcnt(0x0070 | ((LPS * (ST - 2)) & 0xF) | ((((LPS * (ST - 2)) >> 4) & 0x3) << 14));
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        cur_i = (cur_i + 1 == ST) ? 0 : cur_i + 1;
        nxt_i = (nxt_i + 1 == ST) ? 0 : nxt_i + 1;
      }
    }
    else {
      constexpr int NA = Cfg::PIECES_A / Cfg::NWAVES, NB = Cfg::PIECES_B / Cfg::NWAVES;
      using PA = GldsPieces<Cfg::BM, Cfg::EPP, NA, (int) sizeof(T)>;
      using PB = GldsPieces<Cfg::BN, Cfg::EPP, NB, (int) sizeof(T)>;
      // the one 32-bit part of a load's address: it depends on neither the slab nor the piece
      unsigned lane_a = PA::lane_bytes(lane, lda), lane_b = PB::lane_bytes(lane, ldb);
      // one iteration: slab kt is consumed, slab kt+ST-1 loaded.  `load` is a constant true (no branch around any load)
      // or a flag (one copy of the MFMA stream: it only guards the single instructions, a scalar branch each)
      auto iteration = [&](int kt, auto load) {
        R* cur = lds + cur_i * Cfg::BUF_ELEMS;
        R* nbuf = lds + nxt_i * Cfg::BUF_ELEMS;
        {
          // Addresses once per slab and operand: the wave's first piece, then a 64-bit scalar add from piece to piece
          // (GldsPieces).  Recomputed from kt in every slab, so the wrap past nk, the segment switch at K1 and UTAIL's
          // clamp cannot go stale.  The arithmetic stands at the first load's hook point, not at the loop top: there
          // it sat between the slab barrier and the first-step fragment reads.
          const char* pa = nullptr;
          const char* pb = nullptr;
          mma_slab<Cfg, NEG>(cur, cur + Cfg::A_ELEMS, acc, wm, wn, lane, [&](int p) {
            if (p == glds_hook_of<Cfg>(0)) {
              const int kn = glds_slab_ahead(kt, ST - 1, nk, s0) * Cfg::BK;
              pa = reinterpret_cast<const char*>((kn < K1 ? A : A2) + PA::base_elems(wave, kn, lda));
              pb = reinterpret_cast<const char*>((kn < K1 ? B : B2) + PB::base_elems(wave, kn, ldb));
            }
            // (p is a compile-time constant after unrolling: the chain folds to the one instruction of group p)
#define DLAF_GLDS_AT(I)                                                                              \
  if constexpr (I < LPS)                                                                             \
    if (p == glds_hook_of<Cfg>(I)) {                                                                 \
      if constexpr (I < NA) {                                                                        \
        if (load)                                                                                    \
          glds_load_piece(pa, lane_a, nbuf + (wave * NA + I) * Cfg::EPP);                            \
        if constexpr (I + 1 < NA)                                                                    \
          pa += PA::step_bytes(I + 1, lda);                                                          \
      }                                                                                              \
      else {                                                                                         \
        if (load)                                                                                    \
          glds_load_piece(pb, lane_b, nbuf + Cfg::A_ELEMS + (wave * NB + (I - NA)) * Cfg::EPP);      \
        if constexpr (I + 1 < LPS)                                                                   \
          pb += PB::step_bytes(I + 1 - NA, ldb);                                                     \
      }                                                                                              \
    }
            DLAF_GLDS_AT(0) DLAF_GLDS_AT(1) DLAF_GLDS_AT(2) DLAF_GLDS_AT(3) DLAF_GLDS_AT(4) DLAF_GLDS_AT(5)
            DLAF_GLDS_AT(6) DLAF_GLDS_AT(7) DLAF_GLDS_AT(8) DLAF_GLDS_AT(9) DLAF_GLDS_AT(10) DLAF_GLDS_AT(11)
            DLAF_GLDS_AT(12) DLAF_GLDS_AT(13) DLAF_GLDS_AT(14) DLAF_GLDS_AT(15)
#undef DLAF_GLDS_AT
          });
        }
        // slab kt+1 landed?  still in flight afterwards: the loads of slabs kt+2 .. kt+ST-1 (none in the tail)
        if (load)
          __builtin_amdgcn_s_waitcnt(0x0070 | ((LPS * (ST - 2)) & 0xF) | ((((LPS * (ST - 2)) >> 4) & 0x3) << 14));
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        cur_i = (cur_i + 1 == ST) ? 0 : cur_i + 1;
        nxt_i = (nxt_i + 1 == ST) ? 0 : nxt_i + 1;
      };
      for (int kt = 0; kt < nk; ++kt) {
        if constexpr (UTAIL)
          iteration(kt, std::true_type{});
        else
          iteration(kt, kt + ST - 1 < nk);
      }
    }
    if constexpr (UTAIL) {
      // the re-fetched slabs of the last ST-1 iterations: nobody reads them, but they must have landed (in every
      // wave) before the caller reuses the ring
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    return;
  }
  Slab<T, Cfg::BM, Cfg::BK, VEC, Cfg::LDA, Cfg::CXI, Cfg::THREADS> sa;
  Slab<T, Cfg::BN, Cfg::BK, VEC, Cfg::LDB, Cfg::CXI, Cfg::THREADS> sb;
  // (EDGE: the slab picks its source column by column, K1 need not be a multiple of BK)
  sa.template load<EDGE>(0 < K1 ? A : A2, lda, 0, mrows, K, A2, K1);
  sb.template load<EDGE>(0 < K1 ? B : B2, ldb, 0, ncols, K, B2, K1);
  sa.store(lds);
  sb.store(lds + Cfg::A_ELEMS);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    R* cur = lds + (kt & 1) * Cfg::BUF_ELEMS;
    R* nxt = lds + ((kt + 1) & 1) * Cfg::BUF_ELEMS;
    const bool more = (kt + 1) < nk;
    if (more) {
      const int kn = (kt + 1) * Cfg::BK;
      sa.template load<EDGE>(kn < K1 ? A : A2, lda, kn, mrows, K, A2, K1);
      sb.template load<EDGE>(kn < K1 ? B : B2, ldb, kn, ncols, K, B2, K1);
    }
    mma_slab<Cfg, NEG>(cur, cur + Cfg::A_ELEMS, acc, wm, wn, lane);
    if (more) {
      sa.store(nxt);
      sb.store(nxt + Cfg::A_ELEMS);
    }
    __syncthreads();
  }
}

}  // namespace dlaf_mi355x
