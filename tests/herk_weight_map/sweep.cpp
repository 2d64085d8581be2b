// Sweep of the weight index arithmetic of the weighted rank-k update (csrc/device/herk_map.hpp: herk_weight_slots,
// herk_weight_k, herk_weight_slot) against a brute-force model: the enumeration OpSlab::load (gemm_general.hpp) itself
// uses to give thread t its registers.  For every slab shape the kernels instantiate (ROWS x BK with VE elements per
// 16-byte load over THREADS threads: the four element types) and a few more, every mode, every thread and every register:
// the slot the register takes must hold the k of the element the loader put into that register, every slot index must be
// below the thread's slot count, and the k must lie inside the slab.  Host code only: no HIP.
#include <cstdio>
#include <vector>

#include "herk_map.hpp"

using namespace dlaf_mi355x;

// (row, k) of register r of thread t, as OpSlab::load enumerates them
static void loader_element(int mode, int t, int r, int rows, int bk, int ve, int threads, int& row, int& k) {
  if (mode == 0) {
    const int q = r / ve, e = r % ve, idx = t + threads * q;
    row = (idx % (rows / ve)) * ve + e;
    k = idx / (rows / ve);
  }
  else if (mode == 1) {
    const int q = r / ve, e = r % ve, idx = t + threads * q;
    k = (idx % (bk / ve)) * ve + e;
    row = idx / (bk / ve);
  }
  else {
    const int idx = t + threads * r;
    row = idx % rows;
    k = idx / rows;
  }
}

int main() {
  struct Shape {
    int rows, bk, ve, threads;
  };
  // float, double, complex float, complex double (GenCfg), then other shapes the static_asserts of OpSlab admit
  const Shape shapes[] = {{128, 16, 4, 256}, {128, 16, 2, 256}, {128, 16, 2, 256}, {128, 8, 1, 256}, {64, 8, 1, 256},
                          {64, 16, 4, 256},  {128, 32, 4, 256}, {256, 16, 2, 256}, {128, 16, 4, 128}, {64, 8, 2, 64}};
  long checked = 0, failures = 0;
  for (const Shape& s : shapes)
    for (int mode = 0; mode < 3; ++mode) {
      const int per = s.rows * s.bk / s.threads;
      const int slots = herk_weight_slots(mode, s.rows, s.bk, s.ve, s.threads);
      std::vector<int> seen((size_t) s.rows * s.bk, 0);
      for (int t = 0; t < s.threads; ++t)
        for (int r = 0; r < per; ++r) {
          int row = 0, k = 0;
          loader_element(mode, t, r, s.rows, s.bk, s.ve, s.threads, row, k);
          const int slot = herk_weight_slot(mode, r, s.ve);
          const int wk = (slot >= 0 && slot < slots) ? herk_weight_k(mode, t, slot, s.rows, s.bk, s.ve, s.threads) : -1;
          ++checked;
          if (slot < 0 || slot >= slots || wk != k || k < 0 || k >= s.bk || row < 0 || row >= s.rows) {
            if (failures++ < 10)
              std::printf("shape %d x %d ve %d threads %d mode %d: thread %d register %d is (%d, %d), slot %d of %d has k %d\n",
                          s.rows, s.bk, s.ve, s.threads, mode, t, r, row, k, slot, slots, wk);
          }
          else
            ++seen[(size_t) k * s.rows + row];
        }
      // the loader covers every element of the slab exactly once
      for (int v : seen)
        if (v != 1)
          ++failures;
    }
  std::printf("registers %ld failures %ld\n", checked, failures);
  return failures == 0 ? 0 : 1;
}
