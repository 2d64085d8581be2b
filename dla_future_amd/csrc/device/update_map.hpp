// update_map.hpp -- the map from work items of the grouped update to blocks of tiles, as the launcher builds it on the
// host (build_update_map); the kernel decodes a work item against it (update_block, kernels_update.hip).  Plain C++
// and nothing from HIP, so that a host program can sweep it over every geometry (tests/update_map/sweep.cpp).
// `Args` is UpdateArgs<T> (device_api.hpp) or anything with its geometry fields: il0 il1 jl0 jl1 nb pr ri pc ci nt
// last_rows rect nt_c last_cols.
#pragma once

#if defined(__HIPCC__)
#define DLAF_UPDATE_MAP_FN __host__ __device__ __forceinline__
#else
#define DLAF_UPDATE_MAP_FN inline
#endif

namespace dlaf_mi355x {

constexpr int kMaxPatchCols = 256;

struct UpdateMap {
  int ps;        // patch = (1<<ps) block rows x (1<<psc) block columns, square in ELEMENTS
  int psc;
  int PR;        // patch rows
  int tri;       // != 0: only the patches at/below the block-cyclic diagonal are enumerated, patch column by
                 // patch column, through colstart[] (prefix sums of the valid patches per patch column)
  int PC;        // patch columns
  int colstart[kMaxPatchCols + 1];
  int xcd;       // remap blockIdx so each XCD works on consecutive patches
  int RB, CB;    // block rows / cols of the domain
  int bpt_m, bpt_n;
  long total;    // work items (blocks of the patch enumeration)
  int persist;   // != 0: the grid is smaller than `total`; workgroups pull work items from `counters`
  unsigned* counters;  // persist: 8 (per workgroup-id-mod-8, i.e. per XCD) or 1 dequeue heads, zeroed per launch;
                       // counters[8 + q]: work items of queue q that are finished (lockstep pacing)
  int lockstep;        // persist: the workgroups of a queue start their items in rounds (see update_kernel)
  unsigned kphase_ticks;  // persist: wall-clock ticks per K slab of a block (0: every block starts at slab 0)
  int excl_rank;       // persist: workgroups that find themselves on one of the first `excl_rank` compute units of their
                       // XCD (g_cu_rank) leave at once -- whole compute units stay free for the kernels beside the update
  unsigned excl_budget;  // ... but no more than this many per launch (counters[15] counts them)
  int steal;           // persist: a workgroup whose queue is empty drains the other queues
  int* cu_busy;        // persist: per (XCD, compute unit) count of tile-POTRF strips resident there (null: off) -- a bulk
                       // workgroup that shares its compute unit with a strip pauses between two work items
};

// The geometry part of the map (bpt_*, RB / CB, ps / psc, PR / PC, tri, colstart, total, xcd) for BM x BN blocks;
// the launch form (persist and what follows it) is the launcher's.  false: the domain holds no work item.
template <int BM, int BN, class Args>
inline bool build_update_map(const Args& a, UpdateMap& mp) {
  if (a.il1 <= a.il0 || a.jl1 <= a.jl0 || a.nb <= 0)
    return false;
  mp.bpt_m = (a.nb + BM - 1) / BM;
  mp.bpt_n = (a.nb + BN - 1) / BN;
  mp.RB = (a.il1 - a.il0) * mp.bpt_m;
  mp.CB = (a.jl1 - a.jl0) * mp.bpt_n;
  // patches are square in elements (8 block rows x 8*BM/BN block columns), so the triangular patch
  // enumeration also serves rectangular blocks: without it half of a launch is empty workgroups whose
  // long runs starve the compute units (measured on the complex kernel: SQ busy 54 %)
  static_assert(BM % BN == 0 && ((BM / BN) & (BM / BN - 1)) == 0, "BM = 2^s * BN");
  constexpr int kAspectShift = (BM / BN == 1) ? 0 : (BM / BN == 2) ? 1 : 2;
  const bool big = (mp.RB >= 16 && mp.CB >= 16);
  mp.ps = big ? 3 : 0;
  mp.psc = big ? 3 + kAspectShift : 0;
  mp.PR = (mp.RB + (1 << mp.ps) - 1) >> mp.ps;
  mp.PC = (mp.CB + (1 << mp.psc) - 1) >> mp.psc;
  long npatch = (long) mp.PR * mp.PC;
  mp.tri = 0;
  if (mp.PC <= kMaxPatchCols) {
    // first patch row of every patch column that can hold a tile with global row >= global column
    mp.tri = 1;
    mp.colstart[0] = 0;
    for (int pj = 0; pj < mp.PC; ++pj) {
      const int jl_min = a.jl0 + (pj << mp.psc) / mp.bpt_n;
      const long gj_min = (long) jl_min * a.pc + a.ci;
      long il_first = (gj_min - a.ri + a.pr - 1) / a.pr;  // ceil((gj - ri) / pr) for gj >= ri
      if (gj_min <= a.ri || a.rect)
        il_first = 0;
      if (il_first < a.il0)
        il_first = a.il0;
      int cnt = 0;
      if (il_first < a.il1) {
        const int pi0 = (int) (((il_first - a.il0) * mp.bpt_m) >> mp.ps);
        cnt = mp.PR - pi0;
      }
      mp.colstart[pj + 1] = mp.colstart[pj] + cnt;
    }
    npatch = mp.colstart[mp.PC];
    if (npatch == 0)
      return false;
  }
  mp.total = npatch << (mp.ps + mp.psc);
  mp.xcd = (mp.ps > 0) ? 1 : 0;
  return true;
}

// launch slot v of a one-block-per-workgroup launch -> work item: the 8 XCDs (workgroup id mod 8 under round-robin
// dispatch) get contiguous runs of work items
DLAF_UPDATE_MAP_FN long update_xcd_remap(const UpdateMap& mp, long v) {
  return mp.xcd ? (v & 7) * (mp.total >> 3) + (v >> 3) : v;
}

}  // namespace dlaf_mi355x
